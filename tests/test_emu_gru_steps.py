"""The two-layer GRU over the first T of S time steps (cpc_gru_forward_prepare_steps, cpc_gru_forward_coef_prepared_steps,
cpc_gru_backward_streams_steps; csrc/gru.hip: Gru2Fwd::T, Gru2Bwd::T) on the host emulator.

A loss that reads y[:, :T] only has dy[:, T:] == 0: the backward's first S - T steps multiply zeros and the forward's last S - T
steps are read by nobody, and each of them costs a hand-over round trip between workgroups.  The shortened recurrences must give
the values of the full ones.  With S = 20 and T in {S, S - 1, 8, 1}, against a full forward and a full backward on dy with its tail
zeroed:
    * the trimmed backward on the full forward's saved state: dx and the eight gradients torch.equal, dx[:, T:] exactly zero,
      with the backward scratch pre-filled with NaN;
    * the trimmed forward into NaN-filled saved / scratch / y / coefficient buffers: y[:, :T] torch.equal, y[:, T:] == 0, hN left
      alone (T < S); a trimmed backward on top of it gives the same nine tensors, and nothing is NaN;
    * T = 0 and T = S + 1 are argument errors.
Cases: B = 16 (one batch tile) and B = 40 (three tiles, the last ragged), each with the backward's (tile, layer) groups found on
one XCD (HIPEMU_XCDS=8) and straddling (3); B = 24 through the kernels whose workgroups own two batch tiles
(cpc_set_gru_chunk_tiles(1): the smallest batch that takes them); B = 16 on the per-step kernels (cpc_set_gru_mode(0)), whose
bits must equal the persistent exact-f32 path's (mode 1) at every T.

Each case runs in a child process of its own with 384 emulator workers, as tests/test_emu_gru_layer_groups.py does (the group
numbering of three tiles needs more resident workgroups than the 64 of the other emulator tests)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS = 384
S = 20
STEPS = (S, S - 1, 8, 1)
ERR_ARG = 2

CASES = {                    # name: (B, HIPEMU_XCDS, chunk tiles, (gru mode, reference gru mode or None))
    "one-tile": (16, 8, 0, (None, None)),
    "one-tile-straddling": (16, 3, 0, (None, None)),
    "ragged": (40, 8, 0, (None, None)),
    "ragged-straddling": (40, 3, 0, (None, None)),
    "two-tiles-per-workgroup": (24, 8, 1, (None, None)),
    "per-step-kernels": (16, 8, 0, (0, 1)),
}


def _child(name):
    B, xcds, chunk, (mode, ref_mode) = CASES[name]
    os.environ["HIPEMU_XCDS"] = str(xcds)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from cpc_audio_amd import _lib as _L
    from emu_util import P, emu
    from oracle import cpc_oracle as O
    lib = emu()
    nl = 2
    nan = float("nan")
    torch.manual_seed(B)
    p = O.make_params(seed=3, n_levels_gru=nl)
    names = [f"gAR.baseNet.{w}_l{l}" for l in range(nl) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    plist = [p[n].contiguous() for n in names]
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    x = torch.randn(B, S, 256)
    dy_all = torch.randn(B, S, 256)
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_gru_layout(B, S, nl, sizes) == 0
    ncoef = lib.cpc_gru_coef_floats(B, S, nl)
    assert lib.cpc_set_gru_chunk_tiles(chunk) == 0

    def forward(T, gru_mode):
        """T None: the entries without a step count.  Everything the call writes starts as NaN."""
        saved, fscr, coef = torch.full((sizes[0],), nan), torch.full((sizes[1],), nan), torch.full((ncoef,), nan)
        y, hN = torch.full((B, S, 256), nan), torch.full((nl, B, 256), nan)
        if gru_mode is not None:
            assert lib.cpc_set_gru_mode(gru_mode) == 0
        try:
            if T is None:
                assert lib.cpc_gru_forward_coef(P(x), None, parr, P(saved), P(fscr), P(y), P(hN), P(coef), B, S, nl, None) == 0
            else:
                assert lib.cpc_gru_forward_prepare_steps(P(fscr), P(saved), P(y), B, S, T, nl, None) == 0
                assert lib.cpc_gru_forward_coef_prepared_steps(P(x), None, parr, P(saved), P(fscr), P(y), P(hN), P(coef), B, S, T,
                                                               nl, None) == 0
        finally:
            lib.cpc_set_gru_mode(_L.DEFAULT_GRU_MODE)
        assert lib.cpc_device_error_flags(1) == 0
        return saved, y, hN, coef

    def backward(T, state, dy, gru_mode):
        saved, y, _, coef = state
        bscr = torch.full((sizes[2],), nan)
        dx = torch.full((B, S, 256), nan)
        grads = [torch.full_like(t, nan) for t in plist]
        garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
        if gru_mode is not None:
            assert lib.cpc_set_gru_mode(gru_mode) == 0
        try:
            # (the hand-over buffers in `coef` serve one backward call: refilled every time; the coefficients stay)
            assert lib.cpc_gru_backward_coef(None, parr, P(saved), P(y), P(coef), 1, B, S, nl, None) == 0
            if T is None:
                assert lib.cpc_gru_backward_streams(P(x), None, parr, P(saved), P(y), P(dy), P(coef), P(bscr), P(dx), garr, B, S, nl,
                                                    None, None) == 0
            else:
                assert lib.cpc_gru_backward_streams_steps(P(x), None, parr, P(saved), P(y), P(dy), P(coef), P(bscr), P(dx), garr, B,
                                                          S, T, nl, None, None) == 0
        finally:
            lib.cpc_set_gru_mode(_L.DEFAULT_GRU_MODE)
        assert lib.cpc_device_error_flags(1) == 0
        return [dx] + grads

    # ---- argument errors, before anything runs
    scr = forward(None, ref_mode)
    for T in (0, S + 1):
        one = torch.zeros(1)
        assert lib.cpc_gru_forward_prepare_steps(P(one), P(one), P(one), B, S, T, nl, None) == ERR_ARG
        assert lib.cpc_gru_forward_coef_prepared_steps(P(x), None, parr, P(one), P(one), P(one), P(one), None, B, S, T, nl,
                                                       None) == ERR_ARG
        assert lib.cpc_gru_backward_streams_steps(P(x), None, parr, P(one), P(one), P(one), None, P(one), P(one), parr, B, S, T, nl,
                                                  None, None) == ERR_ARG

    full = scr                                           # the full-length forward (reference path of the case)
    assert torch.isfinite(full[1]).all() and torch.isfinite(full[2]).all()
    for T in STEPS:
        dy = dy_all.clone()
        dy[:, T:] = 0
        ref = backward(None, full, dy, ref_mode)         # full-length backward on the zero-tailed dy
        assert all(torch.isfinite(t).all() for t in ref)
        # ---- trimmed backward on the same saved state
        got = backward(T, full, dy, mode)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (name, T, "backward", i)
        assert (got[0][:, T:] == 0).all(), (name, T)
        # ---- trimmed forward into NaN, trimmed backward on top
        part = forward(T, mode)
        assert torch.equal(part[1][:, :T], full[1][:, :T]), (name, T, "y")
        assert (part[1][:, T:] == 0).all(), (name, T, "y tail")
        if T < S:
            assert torch.isnan(part[2]).all(), (name, T, "hN was written")
        else:
            assert torch.equal(part[2], full[2]), (name, T, "hN")
        got = backward(T, part, dy, mode)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.isfinite(b).all(), (name, T, "NaN", i)
            assert torch.equal(a, b), (name, T, "forward + backward", i)
    assert lib.cpc_set_gru_chunk_tiles(0) == 0
    print(f"gru_steps {name}: ok")


@pytest.mark.parametrize("name", list(CASES))
def test_active_steps_change_no_value_emulated(name):
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    try:
        build_emu.build()                                 # (here, so that a compile error is reported once and in full)
    except FileNotFoundError as e:
        pytest.skip(f"emulator build unavailable: {e}")
    env = dict(os.environ, HIPEMU_THREADS=str(WORKERS))
    env.pop("CPC_EMU_SANITIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"gru_steps {name}: ok" in r.stdout, tail


if __name__ == "__main__":
    _child(sys.argv[1])
