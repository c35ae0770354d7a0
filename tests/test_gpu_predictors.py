"""The feed-forward prediction networks on an MI355X (csrc/pred_conv.hip, ``hipPredictors``): the C calls and the autograd
function against this package's torch modules in float64 on the CPU, the reference's stored results
(tests/golden/predictors.npz) through the HIP path, and the criterion end to end against the same criterion with the flag off.

Bars are the project's GPU bars (tests/test_gpu_phone_head.py, tests/test_gpu_lfb.py): rel_err < 1e-5 forward, < 1e-4
gradients, against float64."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from pred_conv_util import (CASES, H, canaries_ok, check_against_oracle, conv_case, oracle, rel_err, run, scale_of,
                            without_relu_ties)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 64
FWD_BAR, GRAD_BAR = 1e-5, 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lib():
    from cpc_audio_amd import _lib as L
    return L.get()


def _on(dev, *ts):
    return tuple(t.to(dev) for t in ts)


@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_causal_conv_matches_shifted_conv_float64(name):
    """Cases a, b, c, e on the device, and f on each: a second call gives the same bits."""
    dev = _dev()
    B, W, G, ks = CASES[name]
    x, w, b, dy = conv_case(B, W, G, ks)
    xd, wd, bd, dyd = _on(dev, x, w, b, dy)
    out = run(_lib(), xd, wd, bd, True, False, dy=dyd, canary=CANARY)
    check_against_oracle(out, x, w, b, dy, True, False, FWD_BAR, GRAD_BAR, show=name)
    canaries_ok(out, CANARY)
    again = run(_lib(), xd, wd, bd, True, False, dy=dyd, canary=CANARY)
    for k in ("y", "dw", "db", "dx"):
        assert torch.equal(out[k], again[k]), k


def test_batch_items_do_not_read_each_other():
    dev = _dev()
    B, W, G, ks = CASES["b_three_items_in_one_tile"]
    x, w, b, dy = conv_case(B, W, G, ks)
    xd, wd, bd, dyd = _on(dev, x, w, b, dy)
    base = run(_lib(), xd, wd, bd, True, False, dy=dyd)
    x2 = xd.clone()
    x2[0] = torch.randn(W, H, generator=torch.Generator().manual_seed(77)).to(dev) * 50.0
    moved = run(_lib(), x2, wd, bd, True, False, dy=dyd)
    y0, y1 = base["y"].view(B, W, G * H), moved["y"].view(B, W, G * H)
    assert torch.equal(y0[1:], y1[1:]) and not torch.equal(y0[0], y1[0])
    alone = run(_lib(), xd[1:2].contiguous(), wd, bd, True, False, dy=dyd[1:2].contiguous())
    assert torch.equal(alone["y"], base["y"][W * G * H:2 * W * G * H])
    assert torch.equal(alone["dx"], base["dx"][W * H:2 * W * H])


@pytest.mark.parametrize("B,W,G", [(2, 6, 3), (2, 70, 2)])
def test_ffd_layers_relu_shared_then_per_head(B, W, G):
    """Case d: lin1 (shared input, ReLU, masked backward), then lin2 (per-head input)."""
    dev = _dev()
    x, w1, b1, dh = conv_case(B, W, G, 1, seed=1)
    _, w2, b2, dy = conv_case(B, W, G, 1, seed=2)
    dh, _ = without_relu_ties(x, w1, b1, True, dh)
    o1 = run(_lib(), *_on(dev, x, w1, b1), True, True, dy=dh.to(dev), canary=CANARY)
    check_against_oracle(o1, x, w1, b1, dh, True, True, FWD_BAR, GRAD_BAR, show="lin1")
    canaries_ok(o1, CANARY)
    h = o1["y"][:B * W * G * H].view(B, W, G * H).clone()
    o2 = run(_lib(), h, *_on(dev, w2, b2), False, False, dy=dy.to(dev), canary=CANARY)
    check_against_oracle(o2, h.cpu(), w2, b2, dy, False, False, FWD_BAR, GRAD_BAR, show="lin2")
    canaries_ok(o2, CANARY)


# the production window and head count for every tap count of the four modes (64 x 64 tiles at B = 2), and shapes that fill the
# chip with the large tile: forward and per-head dx; the shared-input dx over six uneven head groups (11 heads, two per group);
# the shared-input dx of one head on row tiles alone
PRODUCTION = [(2, 116, 12, 1, True), (2, 116, 12, 4, True), (2, 116, 12, 8, True), (2, 116, 12, 12, True),
              (2, 116, 12, 1, False), (32, 116, 7, 2, True), (32, 116, 7, 2, False), (32, 116, 11, 1, True),
              (213, 116, 1, 1, True)]


@pytest.mark.parametrize("B,W,G,ks,shared", PRODUCTION)
def test_function_at_the_production_window(B, W, G, ks, shared):
    """ops.PredConvFunction with autograd (ReLU where ks = 1), in the library's default arithmetic and on the exact-f32 tiles."""
    dev = _dev()
    for exact in (False, True):
        _function_case(dev, B, W, G, ks, shared, exact)


def _function_case(dev, B, W, G, ks, shared, exact):
    lib = _lib()
    mode = lib.cpc_get_mfma_mode()
    try:
        if exact:
            lib.check(lib.cpc_set_mfma_mode(0))
        _function_case_in_mode(dev, B, W, G, ks, shared)
    finally:
        lib.check(lib.cpc_set_mfma_mode(mode))


_ORACLE = {}


def _function_case_in_mode(dev, B, W, G, ks, shared):
    from cpc_audio_amd import ops
    assert ops.pred_conv_supported(B, W, G, ks)
    relu = ks == 1
    x, w, b, dy = conv_case(B, W, G, ks, shared=shared)
    key = (B, W, G, ks, shared)                # the float64 reference is computed once per shape and left unchanged
    if key not in _ORACLE:
        _ORACLE.clear()
        ties = 0
        if relu:
            dy, ties = without_relu_ties(x, w, b, shared, dy)
        _ORACLE[key] = (dy, ties) + tuple(oracle(x, w, b, shared, relu, dy))
    dy, ties, ry, rdw, rdb, rdx = _ORACLE[key]
    xr, wr, br = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    y = ops.PredConvFunction.apply(xr, wr, br, scale_of(ks), relu, shared)
    (y * dy.to(dev)).sum().backward()
    errs = {"y": rel_err(y.detach().cpu().double(), ry), "dw": rel_err(wr.grad.cpu().double(), rdw),
            "db": rel_err(br.grad.cpu().double(), rdb), "dx": rel_err(xr.grad.cpu().double(), rdx)}
    print((B, W, G, ks, shared), {k: f"{e:.3e}" for k, e in errs.items()}, f"relu ties without gradient: {ties} of {dy.numel()}")
    assert errs["y"] < FWD_BAR
    assert errs["dw"] < GRAD_BAR and errs["db"] < GRAD_BAR and errs["dx"] < GRAD_BAR
    # identical calls, identical bits; a frozen context gets no gradient buffer
    x2, w2, b2 = xr.detach(), wr.detach().clone().requires_grad_(True), br.detach().clone().requires_grad_(True)
    y2 = ops.PredConvFunction.apply(x2, w2, b2, scale_of(ks), relu, shared)
    (y2 * dy.to(dev)).sum().backward()
    assert torch.equal(y2, y) and torch.equal(w2.grad, wr.grad) and torch.equal(b2.grad, br.grad)
    ops.check_device_errors()


def test_unsupported_inputs_raise():
    dev = _dev()
    from cpc_audio_amd import ops
    x, w, b, _ = conv_case(1, 2, 2, 1)
    assert not ops.pred_conv_supported(2, 116, 65, 4) and not ops.pred_conv_supported(2, 116, 12, 17)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.PredConvFunction.apply(x, w, b, 1.0, False, True)
    with pytest.raises(NotImplementedError):
        ops.PredConvFunction.apply(x.to(dev), w.to(dev), b.to(dev), 1.0, False, False)       # a per-head input of G*256 columns
    with pytest.raises(ValueError):
        ops.PredConvFunction.apply(x.to(dev), torch.zeros(2, H, H, 17, device=dev), b.to(dev), 1.0, False, True)


@pytest.mark.parametrize("mode", ["ffd", "conv4", "conv8", "conv12"])
def test_reference_fixture_through_the_hip_path(mode):
    """tests/golden/predictors.npz holds what the REFERENCE's PredictionNetwork returned; the same state dict and inputs through
    hipPredictors=True on the device: per-head scores mean_d(pred_k * cand_k) within 2e-6 * max(1, max|ref|), the gradient
    with respect to the context within 1e-4."""
    dev = _dev()
    from cpc_audio_amd.criterion import PredictionNetwork
    from oracle.make_golden_predictors import inputs, seeded_state
    gold = os.path.join(ROOT, "tests", "golden")
    meta = json.load(open(os.path.join(gold, "predictors_meta.json")))
    data = np.load(os.path.join(gold, "predictors.npz"))
    m = meta["modes"][mode]
    net = PredictionNetwork(meta["heads"], 256, 256, rnnMode=mode, dropout=False, sizeInputSeq=meta["window"], hipPredictors=True)
    shapes = {k: tuple(v) for k, v in m["keys"].items()}
    net.load_state_dict(seeded_state(shapes, m["param_seed"]), strict=True)
    net = net.to(dev)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
    c, cand = inputs(m["input_seed"])
    cr = c.to(dev).requires_grad_(True)
    pred = net.predictions(cr)
    assert net.last_path == "hip"
    assert pred.shape == (c.shape[0], c.shape[1], meta["heads"] * 256)
    ref_out, ref_dc = torch.from_numpy(data[f"{mode}:out"]), torch.from_numpy(data[f"{mode}:dc"])
    scores = [(pred[:, :, k * 256:(k + 1) * 256].unsqueeze(1) * cand[k].to(dev)).mean(dim=3) for k in range(meta["heads"])]
    sum(s.sum() for s in scores).backward()
    bar = 2e-6 * max(1.0, ref_out.abs().max().item())
    worst = max((scores[k].detach().cpu() - ref_out[k]).abs().max().item() for k in range(meta["heads"]))
    dc_err = rel_err(cr.grad.cpu(), ref_dc)
    print(mode, f"scores {worst:.3e} (bar {bar:.3e}), dc {dc_err:.3e}")
    assert worst <= bar
    assert dc_err < 1e-4
    # the parameters are still the modules' own: keys, shapes and values survive the stacking
    want = seeded_state(shapes, m["param_seed"])
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), want[k]), k
    for p_ in net.parameters():
        assert p_.grad is not None and tuple(p_.grad.shape) == tuple(p_.shape)


@pytest.mark.parametrize("mode", ["ffd", "conv8"])
def test_criterion_end_to_end_equals_the_flag_off(mode):
    """build_model() + build_criterion(rnnMode, hipPredictors=True) against the same criterion with the flag off: same
    parameters, same supplied negatives.  Bars of test_other_prediction_networks_score_through_the_hip_kernels."""
    dev = _dev()
    from oracle import cpc_oracle as O
    from cpc_audio_amd.train import Trainer, build_criterion, build_model, load_flat_params
    B, K, N, L = 2, 12, 128, 20480
    S = L // 160
    W = S - K
    p = O.make_params(seed=7, head_scale=128.0)
    model = build_model()
    load_flat_params(model, build_criterion(), p)
    torch.manual_seed(3)
    on = build_criterion(rnnMode=mode, hipPredictors=True)
    off = build_criterion(rnnMode=mode)
    off.load_state_dict(copy.deepcopy(on.state_dict()), strict=True)
    model, on, off = model.to(dev), on.to(dev), off.to(dev)
    wave = O.make_waveform(B, L, seed=10).to(dev)
    bi, si = O.draw_negative_indices(B, S, W, N, generator=torch.Generator().manual_seed(5))
    res = {}
    for name, crit in (("on", on), ("off", off)):
        model.zero_grad(set_to_none=True)
        c, z, _ = model(wave, None)
        losses, acc = crit(c, z, None, negatives=(bi.to(dev), si.to(dev)))
        losses.sum().backward()
        res[name] = (losses.detach().cpu(), acc.detach().cpu(), [q.grad.cpu().clone() for q in crit.wPrediction.parameters()],
                     model.gAR.baseNet.weight_hh_l1.grad.cpu().clone(), model.gEncoder.conv4.weight.grad.cpu().clone())
    assert on.wPrediction.last_path == "hip" and off.wPrediction.last_path == "torch"
    a, b = res["on"], res["off"]
    assert (a[0] - b[0]).abs().max().item() < 1e-4
    assert (a[1] - b[1]).abs().max().item() < 2e-3
    for (name, _), ga, gb in zip(on.wPrediction.named_parameters(), a[2], b[2]):
        assert rel_err(ga, gb) < 2e-4, name
    assert rel_err(a[3], b[3]) < 2e-4
    assert rel_err(a[4], b[4]) < 5e-3
    # one Trainer step with the flag on
    tr = Trainer(model, on)
    losses, _ = tr.step(wave, None)
    assert torch.isfinite(losses).all() and on.wPrediction.last_path == "hip"


def test_more_than_sixteen_heads_and_prediction_dropout():
    """K > 16 slices one predictions tensor per head group; the --dropout option sits behind predictions(): both untouched."""
    dev = _dev()
    from cpc_audio_amd.criterion import PredictionNetwork
    torch.manual_seed(11)
    on = PredictionNetwork(17, 256, 256, "conv4", dropout=True, hipPredictors=True).to(dev).eval()
    off = PredictionNetwork(17, 256, 256, "conv4", dropout=True).to(dev).eval()
    off.load_state_dict(on.state_dict())
    c = torch.randn(2, 9, 256, device=dev)
    a, b = on.predictions(c), off.predictions(c)
    assert on.last_path == "hip" and off.last_path == "torch"
    assert rel_err(a.double(), b.double()) < 1e-5
    on.train()
    assert isinstance(on.dropout, torch.nn.Dropout) and bool((on.predictions(c) == 0).any())
    # a foreign predictor, or FFNetwork with dropout, stays on torch
    mixed = PredictionNetwork(3, 256, 256, "conv4", hipPredictors=True).to(dev)
    mixed.predictors[1] = torch.nn.Linear(256, 256).to(dev)
    mixed.predictions(c)
    assert mixed.last_path == "torch"
    ffd = PredictionNetwork(3, 256, 256, "ffd", hipPredictors=True).to(dev)
    ffd.predictors[0].drop.p = 0.1
    ffd.predictions(c)
    assert ffd.last_path == "torch"
    ffd.predictors[0].drop.p = 0.0
    ffd.predictions(c)
    assert ffd.last_path == "hip"
