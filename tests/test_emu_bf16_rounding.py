"""The bf16-storage encoder (cpc_set_mfma_mode(4)) on the host SIMT emulator against the float64 model of its own roundings
(tests/bf16_model.py): every stored tensor and every gradient element by element, each stage fed the emulated device's own stored
inputs, tolerances from the float32 run of the same model.  All four shapes run the 64-row tiles (the 128- and 256-row tiles
need 25600 rows: tests/test_gpu_bf16_rounding.py); (1, 1370), (2, 978) and (3, 1290) end in ragged tiles, (2, 978) has an input
step of layer 1 that no window covers."""
import pytest
import torch

import bf16_model as M
from cpc_audio_amd import _lib as _L
from emu_util import emu
from oracle import cpc_oracle as O

SHAPES = [(2, 1280), (1, 1370), (2, 978), (3, 1290)]
_runs = {}


def _inputs(B, L):
    p = O.make_params(seed=0)
    return [p[n].contiguous() for n in M.NAMES], O.make_waveform(B, L, seed=5)


def _run(B, L, **switches):
    """One emulated forward + backward in mode 4 (cached per shape when no switch is set); every switch is put back."""
    key = (B, L)
    if not switches and key in _runs:
        return _runs[key]
    lib = emu()
    plist, wave = _inputs(B, L)
    assert lib.cpc_set_mfma_mode(4) == 0
    try:
        if "min_rows" in switches:
            assert lib.cpc_set_wgrad_dma_min_rows(switches["min_rows"]) == 0
            assert lib.cpc_set_wgrad_dma_groups(switches["groups"]) == 0
        if "h2_dx" in switches:
            assert lib.cpc_set_h2_dx(switches["h2_dx"]) == 0
        run = M.run_device(lib, plist, wave, lambda Ls: M.make_dz(B, Ls[4], None, seed=1))
    finally:
        lib.cpc_set_mfma_mode(_L.DEFAULT_MFMA_MODE)
        lib.cpc_set_wgrad_dma_min_rows(512)
        lib.cpc_set_wgrad_dma_groups(256)
        lib.cpc_set_h2_dx(1)
    if not switches:
        _runs[key] = run
    return run


@pytest.mark.parametrize("B,L", SHAPES)
def test_bf16_forward_matches_its_float64_model_emulated(B, L):
    run = _run(B, L)
    rep = M.Report(f"emu ({B}, {L})")
    M.check_forward(run, rep)
    rep.assert_ok()


@pytest.mark.parametrize("B,L", SHAPES)
def test_bf16_backward_matches_its_float64_model_emulated(B, L):
    run = _run(B, L)
    if L == 978:
        assert run["Ls"][0] == 4 * run["Ls"][1] + 3          # layer 0's last step feeds no window of layer 1
    rep = M.Report(f"emu ({B}, {L})")
    M.check_backward(run, rep)
    rep.assert_ok()


@pytest.mark.parametrize("B,L", SHAPES)
def test_bf16_backward_mask_differs_from_the_forward_only_inside_the_rounding_band_emulated(B, L):
    run = _run(B, L)
    rep = M.Report(f"emu ({B}, {L})")
    M.check_mask(run, rep)
    rep.assert_ok()


# (5, 1290), the weight gradients only: 320 / 160 / 80 / 40 rows in layers 1..4 -- with 128-row splits layer 1 gets three
# (128 + 128 + 64) and layer 2 two (128 + 32) of conv_wgrad_dma_bf16_kernel, the last ragged; conv_wgrad_kernel<4> splits layer
# 1 into 256 + 64.  Of the four shapes above (3, 1290) splits layer 1 into 128 + 64; the others are too short for two splits.
@pytest.mark.parametrize("B,L", SHAPES + [(5, 1290)])
@pytest.mark.parametrize("plan", ["dma_splits", "tn_tile"])
def test_bf16_weight_gradient_plans_match_the_float64_model_emulated(B, L, plan):
    """The weight gradients again (a) on conv_wgrad_dma_bf16_kernel with the shortest row splits, (b) on conv_wgrad_kernel<4>
    (cpc_set_h2_dx(2)): each from the run's own dx_i and y_{i-1}."""
    switches = {"min_rows": 128, "groups": 512} if plan == "dma_splits" else {"h2_dx": 2}
    run = _run(B, L, **switches)
    rep = M.Report(f"emu ({B}, {L}) {plan}")
    M.check_backward(run, rep, grads=run["grads"])
    rep.assert_ok()
