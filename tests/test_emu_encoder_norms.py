"""The encoder's batchNorm / instanceNorm / ID modes (cpc_audio_amd/csrc/enc_wide.hip; cpc_encoder_*_n) executed on the
host SIMT emulator and compared with the float64 reference of tests/encoder_norms_util.py: the grouped statistics (centred partials,
Chan's formula), batchNorm's running buffers in training and in eval mode, the recomputed layer 0, the padded path at 256 channels,
every gradient -- on CPU.  Every buffer the entries write starts as NaN.

Bars: max |delta| < 2e-5 on y0..y3 and z, 2e-5 norm-wise relative on every gradient (encoder_norms_util.compare has the one
exception, the conv bias gradient where the normalisation removes the mean)."""
import ctypes

import pytest
import torch

import encoder_norms_util as U
from emu_util import emu
from oracle import cpc_oracle as O

BAR = 2e-5
_RUNS = {}


def _run(mode, training, C, B, L, bias_offset=0.0):
    """One NaN-prefilled forward + backward per case, shared by the tests below and left unchanged"""
    key = (mode, training, C, B, L, bias_offset)
    if key not in _RUNS:
        params, running = U.make_params(C, mode, bias_offset=bias_offset)
        wave = O.make_waveform(B, L, seed=5)
        _RUNS[key] = (params, running, wave, U.run_abi(emu(), mode, training, C, B, L, params, running, wave))
    return _RUNS[key]


@pytest.mark.parametrize("C,B,L", U.CASES)
@pytest.mark.parametrize("mode,training", U.VARIANTS)
def test_norm_modes_match_the_float64_reference_emulated(mode, training, C, B, L):
    params, running, wave, res = _run(mode, training, C, B, L)
    run_ref = U.compare(mode, training, params, running, wave, res, BAR)
    if mode != "batchNorm":
        return
    if training:
        # running mean and var after one training call against torch's, relative 1e-5
        for i, (a, b) in enumerate(zip(res["running"], run_ref)):
            e = U.rel_err(a, b)
            print(f"running[{i}]: {e:.3g}")
            assert e < 1e-5, i
    else:
        for a, b in zip(res["running"], running):          # an eval call leaves the buffers bit-unchanged
            assert torch.equal(a, b)


@pytest.mark.parametrize("mode,training", U.VARIANTS)
def test_pad_columns_of_every_saved_activation_are_zero_emulated(mode, training):
    C, B, L = 65, 1, 1370
    _, _, _, res = _run(mode, training, C, B, L)
    sizes, saved = res["sizes"], res["saved"]
    Cp = sizes[26]
    assert Cp == 128
    offsets = [(sizes[8 + i], sizes[3 + i]) for i in range(4)]
    if mode != "ID":
        offsets += [(sizes[11 + i], sizes[3 + i]) for i in range(1, 5)]
    for off, Li in offsets:
        t = saved[off:off + B * Li * Cp].view(B * Li, Cp)
        assert torch.isfinite(t).all() and bool((t[:, C:] == 0).all()) and float(t[:, :C].abs().max()) > 0


def test_instance_norm_with_two_steps_at_the_last_layer_emulated():
    """L = 330 gives L_4 = 2, the least nn.InstanceNorm1d takes.  torch fp32 itself misses half the gradient bar there (5e-5 on a
    gradient, measured on the CPU), so this shape is a forward-only case: y0..y3 and z within the bar."""
    C, B, L = 30, 2, 330
    params, running = U.make_params(C, "instanceNorm")
    wave = O.make_waveform(B, L, seed=5)
    res = U.run_abi(emu(), "instanceNorm", True, C, B, L, params, running, wave, backward=False)
    assert res["sizes"][7] == 2
    U.compare("instanceNorm", True, params, running, wave, res, BAR, check_grads=False)


@pytest.mark.parametrize("mode,training", U.VARIANTS)
def test_a_conv_bias_of_ten_emulated(mode, training):
    """Every conv bias + 10 at (30, 3, 1290): a mean far from zero beside a spread of about one -- what E[x^2] - E[x]^2 loses in
    fp32 and the centred partials keep.  Where torch fp32 itself is above half the bar on this case, the bar is four times torch's
    figure (encoder_norms_util.OFFSET_TORCH_FP32); ID keeps the ordinary bar, batchNorm in eval mode keeps it on the gradients."""
    C, B, L, off = U.OFFSET_CASE
    params, running, wave, res = _run(mode, training, C, B, L, bias_offset=off)
    fwd_bar, grad_bar = U.offset_bars(mode, training, BAR)
    print(f"bars: {fwd_bar:.3g} forward, {grad_bar:.3g} gradients")
    U.compare(mode, training, params, running, wave, res, fwd_bar, grad_bar=grad_bar)


@pytest.mark.parametrize("mode,training", [("batchNorm", True), ("instanceNorm", True)])
def test_workspace_contents_do_not_reach_the_results_emulated(mode, training):
    """saved and both scratches prefilled with 1e30 instead of NaN: identical bits in z, the gradients and the running buffers."""
    C, B, L = 30, 3, 1290
    params, running, wave, res = _run(mode, training, C, B, L)
    res2 = U.run_abi(emu(), mode, training, C, B, L, params, running, wave, dz=res["dz"], fill=1e30)
    assert torch.equal(res["z"], res2["z"])
    for n, g in res["grads"].items():
        assert torch.isfinite(g).all() and torch.equal(g, res2["grads"][n]), n
    for a, b in zip(res["running"] or [], res2["running"] or []):
        assert torch.equal(a, b)


def test_layer_norm_forwards_to_the_c_entries_emulated():
    lib = emu()
    B, L, C = 2, 1280, 40
    sizes, old = (ctypes.c_long * U.SLOTS)(), (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout_n(B, L, C, 0, 1, sizes) == 0 and lib.cpc_encoder_layout_c(B, L, C, old) == 0
    assert list(sizes)[:22] == list(old) and not any(list(sizes)[22:])
    p = O.make_params(seed=0, hidden_encoder=C)
    plist = [p["gEncoder." + n].contiguous() for n in U.NAMES]
    parr = (ctypes.c_void_p * 20)(*[U.P(t) for t in plist])
    wave = O.make_waveform(B, L, seed=5)
    outs = []
    for entry in ("n", "c"):
        saved = torch.full((old[0],), float("nan"))
        fscr = torch.full((max(1, old[1]),), float("nan"))
        z = torch.full((B, old[7], C), float("nan"))
        if entry == "n":
            assert lib.cpc_encoder_forward_n(U.P(wave), parr, None, U.P(saved), U.P(fscr), U.P(z), B, L, C, 0, 1, 0.1, 1e-5, None) == 0
        else:
            assert lib.cpc_encoder_forward_c(U.P(wave), parr, U.P(saved), U.P(fscr), U.P(z), B, L, C, None) == 0
        outs.append(z)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
