"""The bf16-storage encoder (set_activation_storage("bf16"), cpc_set_mfma_mode(4)) on a real MI355X against the float64 model of
its own roundings (tests/bf16_model.py): every stored tensor and every gradient element by element, each stage fed the device's
own stored inputs, tolerances from the float32 run of the same model -- the rules of tests/test_emu_bf16_rounding.py, on the
matrix pipe and on all three tile heights.

bf16_bm (conv_dma.hip) gives 64-row tiles below 25600 rows, 128-row tiles from 25600, 256-row tiles from 51200; the forward
counts B L_i rows, the data gradient of layer i rows x stride with B L_i rows per phase where L_{i-1} = s L_i (dgrad_rows:
"exact"), else B (L_i + 1).
  small shapes: 64-row tiles everywhere; ragged last tiles but at (2, 1280); (2, 978): L0 = 4 L1 + 3, an uncovered step.
  (50, 20480), L = 4096 / 1024 / 512 / 256 / 128, every tile whole:
      forward  layer 1: 51200 rows, 256-row tiles; layer 2: 25600, 128-row; layers 3, 4: 12800 / 6400, 64-row
      dgrad    layer 1: 51200 x 4, 256-row; layer 2: 25600 x 2, 256-row; layer 3: 12800 x 2, 128-row; layer 4: 6400 x 2, 64-row
      wgrad    (conv_wgrad_dma_bf16_kernel) 32 splits of 1600 rows / 50 of 512 / 25 of 512 / 13 of 512, the last 256
  (51, 20474), L = 4095 / 1023 / 511 / 255 / 127, input step 4094 of layer 1 uncovered:
      forward  layer 1: 52173 rows, 256-row tiles, the last 205 rows; layer 2: 26061, 128-row, the last 77; layers 3, 4: 64-row,
               the last 13 / 13
      dgrad    B (L_i + 1) rows, whole tiles whose rows past the input are dropped: layer 1: 52224 x 4, 256-row; layer 2:
               26112 x 2, 256-row; layer 3: 13056 x 2, 128-row; layer 4: 6528 x 2, 64-row
      wgrad    32 splits of 1664 rows, the last 589 / 51 of 512, last 461 / 26 of 512, last 205 / 13 of 512, last 333
At the two large shapes dz is non-zero on three batch items only -- the first, the last and one in the middle, whose rows
contain tile boundaries of layer 1 -- and the CPU reference runs on those: every stage but the weight gradient is independent
per sequence, so the device's dx_i / dy_i must be exactly zero on all other items and the weight gradient is the sum over the
three."""
import ctypes

import pytest
import torch

import bf16_model as M
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

SMALL = [(2, 1280), (1, 1370), (2, 978), (3, 1290)]
LARGE = {(50, 20480): [4096, 1024, 512, 256, 128], (51, 20474): [4095, 1023, 511, 255, 127]}
SHAPES = SMALL + list(LARGE)
_runs = {}


def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from cpc_audio_amd import _lib
    return _lib.get()


def _items(B, L):
    if (B, L) not in LARGE:
        return None
    mid, L1 = B // 2, LARGE[(B, L)][1]
    assert (mid * L1) // 256 < ((mid + 1) * L1 - 1) // 256       # a 256-row tile of layer 1 begins inside the item
    return [0, mid, B - 1]


def _run(B, L, h2_dx=None):
    key = (B, L)
    if h2_dx is None and key in _runs:
        return _runs[key]
    import cpc_audio_amd
    lib = _lib()
    sizes = (ctypes.c_long * 22)()
    p = O.make_params(seed=0)
    plist = [p[n].contiguous() for n in M.NAMES]
    wave = O.make_waveform(B, L, seed=5)
    items = _items(B, L)
    cpc_audio_amd.set_activation_storage("bf16")
    try:
        assert lib.cpc_encoder_layout(B, L, sizes) == 0
        if key in LARGE:
            assert [sizes[3 + i] for i in range(5)] == LARGE[key]
        if h2_dx is not None:
            assert lib.cpc_set_h2_dx(h2_dx) == 0
        run = M.run_device(lib, plist, wave, lambda Ls: M.make_dz(B, Ls[4], items, seed=1), device="cuda:0",
                           stream=torch.cuda.current_stream().cuda_stream, items=items)
    finally:
        lib.cpc_set_h2_dx(1)
        cpc_audio_amd.set_activation_storage("fp32")
    if h2_dx is None:
        _runs[key] = run
    return run


@pytest.mark.parametrize("B,L", SHAPES)
def test_bf16_forward_matches_its_float64_model(B, L):
    run = _run(B, L)
    rep = M.Report(f"gpu ({B}, {L})")
    M.check_forward(run, rep)
    rep.assert_ok()


@pytest.mark.parametrize("B,L", SHAPES)
def test_bf16_backward_matches_its_float64_model(B, L):
    run = _run(B, L)
    if L in (978, 20474):
        assert run["Ls"][0] == 4 * run["Ls"][1] + 3              # layer 0's last step feeds no window of layer 1
    rep = M.Report(f"gpu ({B}, {L})")
    M.check_backward(run, rep)
    rep.assert_ok()


@pytest.mark.parametrize("B,L", SHAPES)
def test_bf16_backward_mask_differs_from_the_forward_only_inside_the_rounding_band(B, L):
    run = _run(B, L)
    rep = M.Report(f"gpu ({B}, {L})")
    M.check_mask(run, rep)
    rep.assert_ok()


@pytest.mark.parametrize("B,L", [(3, 1290), (51, 20474)])
def test_bf16_weight_gradient_on_the_register_staged_tile_matches_the_float64_model(B, L):
    """cpc_set_h2_dx(2): the weight gradients on conv_wgrad_kernel<4> instead of the DMA kernel, from the run's own dx_i, y_{i-1}."""
    run = _run(B, L, h2_dx=2)
    rep = M.Report(f"gpu ({B}, {L}) tn_tile")
    M.check_backward(run, rep, grads=run["grads"])
    rep.assert_ok()


def test_keeping_the_data_gradients_changes_nothing():
    """cpc_encoder_keep_data_gradients only copies: same dx, dy0 and gradients, bit for bit, with and without it."""
    import cpc_audio_amd
    B, L = 2, 978
    kept = _run(B, L)
    lib = _lib()
    p = O.make_params(seed=0)
    cpc_audio_amd.set_activation_storage("bf16")
    try:
        plain = M.run_device(lib, [p[n].contiguous() for n in M.NAMES], O.make_waveform(B, L, seed=5),
                             lambda Ls: M.make_dz(B, Ls[4], None, seed=1), device="cuda:0",
                             stream=torch.cuda.current_stream().cuda_stream, keep_dy=False)
    finally:
        cpc_audio_amd.set_activation_storage("fp32")
    for a, b in zip(kept["grads"] + kept["dx"][1:] + [kept["dy"][0]], plain["grads"] + plain["dx"][1:] + [plain["dy"][0]]):
        assert torch.equal(a, b)
