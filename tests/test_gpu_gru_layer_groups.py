"""The backward recurrence with the (tile, layer) group numbering and the XCD-local hand-over inside a group
(cpc_set_gru_xcd_local bit 1; csrc/persist.h: kPackGroup, csrc/gru.hip: persist_bwd) on a real MI355X.

Where the 16 workgroups of a group sit on one XCD they hand dh over with plain stores through that XCD's L2, and layer 1 adds a
device-scope copy for layer 0 on its other XCD: a matter of memory scope and placement, never of arithmetic.  So dx and the eight
parameter gradients of cpc_gru_backward must be bit-identical with the switch on, with it off (unpacked launch, device-scope
stores) and on the per-step wavefront kernels, at B = 64, S = 16 (four tiles: eight groups, one per XCD) and at B = 24, S = 12
(a ragged second tile, four groups); and one composite train step at B = 64 must give the same losses and the same flat gradient
buffer with the switch on and off.  No wave may run out of its polling budget (cpc_device_error_flags() == 0)."""
import ctypes

import pytest
import torch

from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

GROUPS_ON = 3          # cpc_set_gru_xcd_local: forward per tile (the default) + backward per (tile, layer) group


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda:0")


def P(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("B,S", [(64, 16), (24, 12)])
def test_backward_layer_groups_change_no_bit(B, S):
    dev = _dev()
    from cpc_audio_amd import _lib
    lib = _lib.get()
    nl = 2
    p = O.make_params(seed=3, n_levels_gru=nl)
    names = [f"gAR.baseNet.{w}_l{l}" for l in range(nl) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    plist = [p[n].contiguous().to(dev) for n in names]
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    g = torch.Generator().manual_seed(B * 1000 + S)
    x = torch.randn(B, S, 256, generator=g).to(dev)
    dy = torch.randn(B, S, 256, generator=g).to(dev)
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_gru_layout(B, S, nl, sizes) == 0
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    saved, fscr, y, hN = nan(sizes[0]), nan(sizes[1]), nan(B, S, 256), nan(nl, B, 256)
    torch.cuda.synchronize()
    assert lib.cpc_gru_forward(P(x), None, parr, P(saved), P(fscr), P(y), P(hN), B, S, nl, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()

    def backward(mode, local):
        bscr, dx = nan(sizes[2]), nan(B, S, 256)
        grads = [torch.full_like(t, float("nan")) for t in plist]
        garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
        torch.cuda.synchronize()
        assert lib.cpc_set_gru_mode(mode) == 0 and lib.cpc_set_gru_xcd_local(local) == 0
        try:
            assert lib.cpc_gru_backward(P(x), None, parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, None) == 0
            torch.cuda.synchronize()
        finally:
            lib.cpc_set_gru_mode(_lib.DEFAULT_GRU_MODE)
            lib.cpc_set_gru_xcd_local(_lib.DEFAULT_GRU_XCD_LOCAL)
        assert lib.cpc_device_error_flags(1) == 0
        return [dx] + grads

    ref = backward(1, 1)                                  # persistent, backward unpacked with device-scope stores
    assert all(torch.isfinite(t).all() for t in ref)
    for what, out in (("per-step kernels", backward(0, 1)), ("layer groups", backward(1, GROUPS_ON))):
        assert len(out) == 9
        for i, (a, b) in enumerate(zip(ref, out)):
            assert torch.equal(a, b), (what, i)


def test_train_step_with_layer_groups_changes_no_bit():
    """One composite step (cpc_train_step) at B = 64 -- the recurrence's backward beside the criterion's dz path on the side
    stream -- twice from the same parameters (the optimiser is stubbed out): switch off, switch on."""
    dev = _dev()
    from cpc_audio_amd import _lib, ops
    from cpc_audio_amd.train import Trainer, build_criterion, build_model, load_flat_params
    lib = _lib.get()
    B = 64
    p = O.make_params(seed=32, head_scale=64.0)
    model, crit = build_model().to(dev), build_criterion().to(dev)
    load_flat_params(model, crit, p)
    model.train(); crit.train()
    tr = Trainer(model, crit, fused=True)
    tr.optimizer.step = lambda *a, **k: None              # keep the gradients and the parameters
    tr.optimizer.zero_grad = lambda *a, **k: None
    wave = O.make_waveform(B, 20480, seed=50).to(dev)
    label = torch.zeros(B, dtype=torch.long, device=dev)
    gen = torch.Generator().manual_seed(18)
    bidx, sidx = O.draw_negative_indices(B, 128, 116, 128, generator=gen)
    neg = (bidx.to(dev), sidx.to(dev))
    res = []
    try:
        for local in (_lib.DEFAULT_GRU_XCD_LOCAL & ~2, GROUPS_ON):
            assert lib.cpc_set_gru_xcd_local(local) == 0
            l, a = tr.step(wave, label, negatives=neg)
            tr.join()
            torch.cuda.synchronize()
            assert tr._fused is not None
            ops.check_device_errors()
            res.append((l.cpu().clone(), a.cpu().clone(), tr.allreduce.buf.detach().cpu().clone()))
    finally:
        lib.cpc_set_gru_xcd_local(_lib.DEFAULT_GRU_XCD_LOCAL)
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][2]).all()
    assert float(res[0][2].abs().sum()) > 0.0
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
