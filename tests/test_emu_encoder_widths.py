"""The encoder at any hidden width (cpc_audio_amd/csrc/enc_wide.hip; cpc_encoder_*_c) executed on the host SIMT emulator and compared
with the float64 oracle: padded storage, the overlapping-row GEMM tiles and their ragged edges, the gather-form data gradient, the
unbiased ChannelNorm over the true channels, every one of the 20 gradients -- on CPU.  Every buffer the entries write starts as NaN."""
import ctypes

import pytest
import torch

from emu_util import P, emu, rel_err
from oracle import cpc_oracle as O

NAMES = [f"gEncoder.{n}{i}.{w}" for i in range(5)
         for n, w in (("conv", "weight"), ("conv", "bias"), ("batchNorm", "weight"), ("batchNorm", "bias"))]
SHAPE = 1          # CPC_ERR_SHAPE


def _params(C, seed=0):
    p = O.make_params(seed=seed, hidden_encoder=C)
    return p, [p[n].contiguous() for n in NAMES]


def _oracle64(p, wave, dz, relu_override):
    """O.encoder_forward in float64 with oneDNN off (tests/test_emu_encoder.py says why): z, y0..y3 channels-last, the leaves"""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in p.items() if k.startswith("gEncoder")}
    acts = []
    with torch.backends.mkldnn.flags(enabled=False):
        z = O.encoder_forward(leaves, wave.double(), collect=acts, relu_override=relu_override).permute(0, 2, 1)
        (z * dz.double()).sum().backward()
    return z.detach(), [a.detach().permute(0, 2, 1).contiguous() for a in acts], leaves


def _run(lib, C, B, L, plist, wave, dz=None, fill=float("nan"), backward=True):
    sizes = (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout_c(B, L, C, sizes) == 0
    Ls = [sizes[3 + i] for i in range(5)]
    saved = torch.full((sizes[0],), fill)
    fscr = torch.full((max(1, sizes[1]),), fill)
    z = torch.full((B, Ls[4], C), float("nan"))
    parr = (ctypes.c_void_p * 20)(*[P(t) for t in plist])
    assert lib.cpc_encoder_forward_c(P(wave), parr, P(saved), P(fscr), P(z), B, L, C, None) == 0
    ys = []
    for i in range(4):
        y = torch.full((B, Ls[i], C), float("nan"))
        assert lib.cpc_encoder_saved_activation_c(P(saved), i, P(y), B, L, C, None) == 0
        ys.append(y)
    if not backward:
        return z, ys, None, None
    if dz is None:
        dz = torch.randn(B, Ls[4], C, generator=torch.Generator().manual_seed(11))

    def bwd():
        bscr = torch.full((sizes[2],), fill)
        grads = [torch.full_like(t, float("nan")) for t in plist]
        garr = (ctypes.c_void_p * 20)(*[P(t) for t in grads])
        assert lib.cpc_encoder_backward_c(P(wave), parr, P(saved), P(z), P(dz), P(bscr), garr, B, L, C, None) == 0
        return grads

    return z, ys, dz, bwd


# one 64-column block (3, 12, 13, 30), a block edge (64 / 65), a ragged last block (130, 272), the full eight (512); the one-step
# window (170), the layer-0 step no window of layer 1 touches (978), partial row tiles
CASES = [(3, 2, 1280), (12, 1, 170), (13, 1, 1370), (30, 3, 1290), (64, 2, 978), (65, 1, 1600), (130, 2, 978), (272, 1, 1370),
         (512, 1, 978), (512, 2, 170)]


_DEVICE = {}


def _device(C, B, L):
    """One NaN-prefilled forward + backward per case, shared by the tests below and left unchanged"""
    key = (C, B, L)
    if key not in _DEVICE:
        p, plist = _params(C)
        wave = O.make_waveform(B, L, seed=5)
        z, ys, dz, bwd = _run(emu(), C, B, L, plist, wave)
        _DEVICE[key] = (p, plist, wave, z, ys, dz, bwd, bwd())
    return _DEVICE[key]


@pytest.mark.parametrize("C,B,L", CASES)
def test_encoder_widths_match_the_float64_oracle_emulated(C, B, L):
    """max |delta| < 2e-5 on y0..y3 and z, every gradient within 2e-5 (norm-wise relative) of O.encoder_forward in float64 with the
    device's ReLU masks as the tie override."""
    p, plist, wave, z, ys, dz, bwd, grads = _device(C, B, L)
    O.tie_report()
    z_ref, acts, leaves = _oracle64(p, wave, dz, [(y > 0).permute(0, 2, 1) for y in ys + [z]])
    ties = O.tie_report()
    print(f"relu ties: {ties}")
    assert O.tie_ok(ties) and ties["disagree_outside"] == 0, ties
    assert z_ref.shape == z.shape
    for i in range(4):
        err = (ys[i].double() - acts[i]).abs().max().item()
        print(f"y{i}: max |delta| = {err:.3g}")
        assert err < 2e-5, f"layer {i}"
    err = (z.double() - z_ref).abs().max().item()
    print(f"z: max |delta| = {err:.3g}")
    assert err < 2e-5
    bad = {}
    for n, g in zip(NAMES, grads):
        ref = leaves[n].grad
        e = rel_err(g.double().view_as(ref), ref) if torch.isfinite(g).all() else float("inf")
        print(f"{n}: {e:.3g}")
        if not e < 2e-5:
            bad[n] = e
    assert not bad, bad


@pytest.mark.parametrize("C,B,L", CASES)
def test_workspace_contents_do_not_reach_the_results_emulated(C, B, L):
    """saved and both scratches prefilled with 1e30 instead of NaN: identical bits in z and in all 20 gradients."""
    _, plist, wave, z, _, dz, _, grads = _device(C, B, L)
    z2, _, _, bwd2 = _run(emu(), C, B, L, plist, wave, dz=dz, fill=1e30)
    for a, b in zip([z] + grads, [z2] + bwd2()):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("C,B,L", CASES)
def test_two_backward_calls_give_the_same_bits_emulated(C, B, L):
    _, _, _, _, _, _, bwd, grads = _device(C, B, L)
    for a, b in zip(grads, bwd()):
        assert torch.equal(a, b)


def test_two_channels_run_emulated():
    """C = 2: the norm over two channels amplifies by up to 1 / sqrt(eps), so there is no parity bar; the call returns 0, writes
    every output and leaves no NaN."""
    lib = emu()
    _, plist = _params(2)
    z, ys, _, bwd = _run(lib, 2, 2, 1280, plist, O.make_waveform(2, 1280, seed=5))
    for t in [z] + ys + bwd():
        assert torch.isfinite(t).all()


def test_width_256_delegates_to_the_256_entry_points_emulated():
    lib = emu()
    B, L, C = 2, 1280, 256
    _, plist = _params(C)
    wave = O.make_waveform(B, L, seed=5)
    sizes, old = (ctypes.c_long * 22)(), (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout_c(B, L, C, sizes) == 0 and lib.cpc_encoder_layout(B, L, old) == 0
    assert list(sizes) == list(old)
    z, ys, dz, bwd = _run(lib, C, B, L, plist, wave)
    grads = bwd()
    saved = torch.full((old[0],), float("nan"))
    fscr = torch.full((max(1, old[1]),), float("nan"))
    z0 = torch.full_like(z, float("nan"))
    parr = (ctypes.c_void_p * 20)(*[P(t) for t in plist])
    assert lib.cpc_encoder_forward(P(wave), parr, P(saved), P(fscr), P(z0), B, L, None) == 0
    assert torch.equal(z, z0)
    for i in range(4):
        y = torch.full_like(ys[i], float("nan"))
        assert lib.cpc_encoder_saved_activation(P(saved), i, P(y), B, L, None) == 0
        assert torch.equal(y, ys[i])
    bscr = torch.full((old[2],), float("nan"))
    g0 = [torch.full_like(t, float("nan")) for t in plist]
    garr = (ctypes.c_void_p * 20)(*[P(t) for t in g0])
    assert lib.cpc_encoder_backward(P(wave), parr, P(saved), P(z0), P(dz), P(bscr), garr, B, L, None) == 0
    for a, b in zip(grads, g0):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C", [0, 1, 513])
def test_widths_outside_2_to_512_are_refused_emulated(C):
    lib = emu()
    B, L = 1, 1280
    sizes = (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout_c(B, L, C, sizes) == SHAPE
    assert lib.cpc_encoder_layout_c(B, L, 40, sizes) == 0
    Cb = max(C, 1)
    plist = [torch.zeros(s) for s in ([(Cb, 1, 10), (Cb,), (1, Cb, 1), (1, Cb, 1)] + [(Cb, Cb, 4), (Cb,), (1, Cb, 1), (1, Cb, 1)] * 4)]
    parr = (ctypes.c_void_p * 20)(*[P(t) for t in plist])
    saved, scr = torch.zeros(1 << 20), torch.zeros(1 << 20)
    z = torch.full((B, sizes[7], Cb), float("nan"))
    wave = O.make_waveform(B, L, seed=5)
    assert lib.cpc_encoder_forward_c(P(wave), parr, P(saved), P(scr), P(z), B, L, C, None) == SHAPE
    assert torch.isnan(z).all()
    grads = [torch.full_like(t, float("nan")) for t in plist]
    garr = (ctypes.c_void_p * 20)(*[P(t) for t in grads])
    assert lib.cpc_encoder_backward_c(P(wave), parr, P(saved), P(z), P(z), P(scr), garr, B, L, C, None) == SHAPE
    assert all(torch.isnan(g).all() for g in grads)
    assert lib.cpc_encoder_saved_activation_c(P(saved), 0, P(z), B, L, C, None) == SHAPE
    assert torch.isnan(z).all()
