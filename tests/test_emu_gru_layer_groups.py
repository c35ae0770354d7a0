"""The backward recurrence with the (tile, layer) group numbering and the XCD-local hand-over inside a group
(cpc_set_gru_xcd_local bit 1; csrc/persist.h: kPackGroup, csrc/gru.hip: persist_bwd) on the host emulator.

dx and the eight parameter gradients of cpc_gru_backward must be bit-identical with the grouped hand-over on, with it off
(unpacked launch, device-scope stores) and on the per-step wavefront kernels (cpc_set_gru_mode(0)), and no wave may have run out
of its polling budget (cpc_device_error_flags() == 0).  Shapes, each at S = 12, for where the numbering can go wrong:
    B = 16   one batch tile, two groups
    B = 40   three tiles, the last one ragged, six groups
    B = 144  nine tiles: 18 groups, more than the 8 XCDs -- up to three groups one after the other on an XCD
The grouped launch runs twice: with the emulator placing workgroup b on XCD b % 8 (HIPEMU_XCDS=8 -- what the numbering assumes,
every group on one XCD: plain stores inside the group plus layer 1's device-scope copy for layer 0) and with b % 3 (every group
straddles: device-scope stores throughout).

All 32 workgroups per tile of a persistent launch must be resident at once and the emulated device has as many CUs as the
emulator has worker threads, a number fixed per process (64 in the other emulator tests: two tiles).  Nine tiles in the group
numbering need 8 XCDs x 48 slots, so each shape runs in a child process of its own with 384 workers -- this file, run as a
script -- where the host side's own residency check (persist_pack_fits) admits the numbering without it being forced."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS = 384
S = 12


def _child(B):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from cpc_audio_amd import _lib as _L
    from emu_util import P, emu
    from oracle import cpc_oracle as O
    lib = emu()
    nl = 2
    torch.manual_seed(B)
    p = O.make_params(seed=3, n_levels_gru=nl)
    names = [f"gAR.baseNet.{w}_l{l}" for l in range(nl) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    plist = [p[n].contiguous() for n in names]
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    x = torch.randn(B, S, 256)
    dy = torch.randn(B, S, 256)
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_gru_layout(B, S, nl, sizes) == 0
    saved = torch.full((sizes[0],), float("nan"))
    fscr = torch.full((sizes[1],), float("nan"))
    y = torch.full((B, S, 256), float("nan"))
    hN = torch.full((nl, B, 256), float("nan"))
    assert lib.cpc_gru_forward(P(x), None, parr, P(saved), P(fscr), P(y), P(hN), B, S, nl, None) == 0
    assert torch.isfinite(y).all()

    def backward(mode, local, xcds):
        os.environ["HIPEMU_XCDS"] = str(xcds)
        assert lib.cpc_set_gru_mode(mode) == 0 and lib.cpc_set_gru_xcd_local(local) == 0
        try:
            bscr = torch.full((sizes[2],), float("nan"))
            dx = torch.full((B, S, 256), float("nan"))
            grads = [torch.full_like(t, float("nan")) for t in plist]
            garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
            assert lib.cpc_gru_backward(P(x), None, parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, None) == 0
        finally:
            lib.cpc_set_gru_mode(_L.DEFAULT_GRU_MODE)
            lib.cpc_set_gru_xcd_local(_L.DEFAULT_GRU_XCD_LOCAL)
        assert lib.cpc_device_error_flags(1) == 0
        return [dx] + grads

    ref = backward(1, 1, 8)                               # persistent, backward unpacked with device-scope stores
    assert all(torch.isfinite(t).all() for t in ref)
    runs = {"per-step kernels": backward(0, 1, 8),
            "groups, each on one XCD": backward(1, 3, 8),
            "groups, straddling": backward(1, 3, 3)}
    for what, out in runs.items():
        assert len(out) == 9
        for i, (a, b) in enumerate(zip(ref, out)):
            assert torch.equal(a, b), (what, i)
    print(f"layer_groups B={B}: ok")


@pytest.mark.parametrize("B", [16, 40, 144])
def test_backward_layer_groups_change_no_bit_emulated(B):
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    try:
        build_emu.build()                                 # (here, so that a compile error is reported once and in full)
    except FileNotFoundError as e:
        pytest.skip(f"emulator build unavailable: {e}")
    env = dict(os.environ, HIPEMU_THREADS=str(WORKERS))
    env.pop("CPC_EMU_SANITIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(B)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"layer_groups B={B}: ok" in r.stdout, tail


if __name__ == "__main__":
    _child(int(sys.argv[1]))
