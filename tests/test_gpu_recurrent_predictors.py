"""The recurrent prediction networks and the RNN autoregressor on an MI355X: ops.LstmGroupFunction (csrc/lstm.hip) and
ops.RnnFunction (csrc/rnn.hip) against torch.nn.LSTM / torch.nn.RNN in float64 on the CPU, the reference's stored results
(tests/golden/predictors.npz, modes RNN and LSTM) through the HIP path, the criterion end to end against the same criterion with
the flag off, and CPCAR(mode="RNN", rnnKernel=True).

Bars: tests/test_gpu_lstm.py (|dy| < 1e-4, rel < 1e-4 against float64) and tests/test_gpu_predictors.py (fixture, flag on / off)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _no_device_errors():
    yield
    if torch.cuda.is_available():
        from cpc_audio_amd import ops
        ops.check_device_errors()                       # raises on any flagged device error


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _stack(mods):
    return [torch.cat([m.weight_ih_l0.detach() for m in mods]), torch.stack([m.weight_hh_l0.detach() for m in mods]),
            torch.cat([m.bias_ih_l0.detach() for m in mods]), torch.cat([m.bias_hh_l0.detach() for m in mods])]


def _group_oracle(mods, x, dy):
    """G one-layer cells in float64 on the CPU: y with head g at columns g*256.., the summed dx, the stacked gradients"""
    refs = [copy.deepcopy(m).double() for m in mods]
    xr = x.double().requires_grad_(True)
    y = torch.cat([m(xr)[0] for m in refs], dim=2)
    (y * dy.double()).sum().backward()
    grads = [torch.cat([m.weight_ih_l0.grad for m in refs]), torch.stack([m.weight_hh_l0.grad for m in refs]),
             torch.cat([m.bias_ih_l0.grad for m in refs]), torch.cat([m.bias_hh_l0.grad for m in refs])]
    return y.detach(), xr.grad, grads


def _group_case(dev, cell, B, W, G):
    """The function on its default path twice and on the per-step path: same bits; against float64."""
    from cpc_audio_amd import ops
    torch.manual_seed(0)
    mods = [torch.nn.LSTM(H, H, batch_first=True) if cell == "LSTM" else torch.nn.RNN(H, H) for _ in range(G)]
    g = torch.Generator().manual_seed(1)
    x, dy = torch.randn(B, W, H, generator=g), torch.randn(B, W, G * H, generator=g)
    assert ops.lstm_group_supported(B, W, G) if cell == "LSTM" else ops.rnn_supported(B, W, G, 1)

    def run(per_step):
        params = [p.to(dev).requires_grad_(True) for p in _stack(mods)]
        xd = x.to(dev).requires_grad_(True)
        if cell == "LSTM":
            y = ops.LstmGroupFunction.apply(xd, per_step, *params)
        else:
            y, hN = ops.RnnFunction.apply(xd, None, True, per_step, *params)
            assert hN is None
        (y * dy.to(dev)).sum().backward()
        torch.cuda.synchronize()
        return [y.detach().cpu(), xd.grad.cpu()] + [p.grad.cpu() for p in params]

    a, again, steps = run(False), run(False), run(True)
    for k, (u, v, w) in enumerate(zip(a, again, steps)):
        assert torch.equal(u, v), ("second call", k)
        assert torch.equal(u, w), ("per-step path", k)
    yr, dxr, gr = _group_oracle(mods, x, dy)
    y, dx, *grads = a
    errs = {"y": (y.double() - yr).abs().max().item(), "dx": _rel(dx, dxr)}
    errs.update({n: _rel(gq, w) for n, gq, w in zip(NAMES, grads, gr)})
    print(cell, (B, W, G), {k: f"{e:.3e}" for k, e in errs.items()})
    assert not torch.isnan(y).any()
    assert all(e < 1e-4 for e in errs.values()), errs


@pytest.mark.parametrize("B,W,G", [(2, 116, 12), (40, 116, 12)])
def test_lstm_group_function_matches_float64_and_paths_agree(B, W, G):
    """The production window and head count; B = 40: three row tiles, the last one partial, 576 workgroups."""
    _group_case(_dev(), "LSTM", B, W, G)


@pytest.mark.parametrize("B,W,G", [(2, 116, 12), (40, 116, 12)])
def test_rnn_function_time_major_matches_float64_and_paths_agree(B, W, G):
    """The predictors' shape: the recurrence walks the batch axis (T = B), R = W = 116 rows in eight row tiles, 12 heads."""
    _group_case(_dev(), "RNN", B, W, G)


@pytest.mark.parametrize("mode", ["RNN", "LSTM"])
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
    dc_err = _rel(cr.grad.cpu(), ref_dc)
    print(mode, f"scores {worst:.3e} (bar {bar:.3e}), dc {dc_err:.3e}")
    assert worst <= bar
    assert dc_err < 1e-4
    # the parameters are still the modules' own: keys, shapes and values survive the stacking
    want = seeded_state(shapes, m["param_seed"])
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), want[k]), k
    for p_ in net.parameters():
        assert p_.grad is not None and tuple(p_.grad.shape) == tuple(p_.shape)


@pytest.mark.parametrize("mode", ["RNN", "LSTM"])
def test_criterion_end_to_end_equals_the_flag_off(mode):
    """build_model() + build_criterion(rnnMode, hipPredictors=True) against the same criterion with the flag off: same
    parameters, same supplied negatives.  Thresholds of tests/test_gpu_predictors.py."""
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
        assert _rel(ga, gb) < 2e-4, name
    assert _rel(a[3], b[3]) < 2e-4
    assert _rel(a[4], b[4]) < 5e-3
    # one Trainer step with the flag on
    tr = Trainer(model, on)
    losses, _ = tr.step(wave, None)
    assert torch.isfinite(losses).all() and on.wPrediction.last_path == "hip"


def test_what_the_kernels_do_not_compute_stays_on_torch():
    dev = _dev()
    from cpc_audio_amd.criterion import PredictionNetwork
    torch.manual_seed(11)
    c = torch.randn(2, 9, 256, device=dev)
    for mode in ("LSTM", "RNN"):
        on = PredictionNetwork(3, 256, 256, mode, hipPredictors=True).to(dev)
        off = PredictionNetwork(3, 256, 256, mode).to(dev)
        off.load_state_dict(on.state_dict())
        a, b = on.predictions(c), off.predictions(c)
        assert on.last_path == "hip" and off.last_path == "torch"
        assert (a - b).abs().max().item() < 1e-4
        # a foreign module among the heads: the torch modules run, on the parameters the HIP call left stacked
        on.predictors[1] = torch.nn.GRU(256, 256, batch_first=True).to(dev)
        assert on.predictions(c).shape == (2, 9, 3 * 256) and on.last_path == "torch"
        # fp64 input
        on = PredictionNetwork(3, 256, 256, mode, hipPredictors=True).to(dev).double()
        on.predictions(c.double())
        assert on.last_path == "torch"
    two = PredictionNetwork(3, 256, 256, "LSTM", hipPredictors=True).to(dev)
    two.predictors[0] = torch.nn.LSTM(256, 256, num_layers=2, batch_first=True).to(dev)
    two.predictions(c)
    assert two.last_path == "torch"
    relu = PredictionNetwork(3, 256, 256, "RNN", hipPredictors=True).to(dev)
    relu.predictors[2] = torch.nn.RNN(256, 256, nonlinearity="relu").to(dev)
    relu.predictions(c)
    assert relu.last_path == "torch"
    first = PredictionNetwork(3, 256, 256, "RNN", hipPredictors=True).to(dev)
    first.predictors[0] = torch.nn.RNN(256, 256, batch_first=True).to(dev)
    first.predictions(c)
    assert first.last_path == "torch"


# ------------------------------------------------------------------ CPCAR(mode="RNN", rnnKernel=True)
def _oracle_rnn(net):
    ref = torch.nn.RNN(H, H, num_layers=net.num_layers, batch_first=True).double()
    with torch.no_grad():
        for l in range(net.num_layers):
            for n in NAMES:
                getattr(ref, f"{n}_l{l}").copy_(getattr(net, f"{n}_l{l}").detach().cpu().double())
    return ref


@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("B", [2, 64])
def test_rnn_autoregressor_matches_torch_float64(B, nl, state):
    """S = 128: y, the kept state, dx and every parameter gradient against nn.RNN in float64."""
    dev = _dev()
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(4)
    ar = CPCAR(256, 256, True, nl, mode="RNN", rnnKernel=True).to(dev)
    assert ar.hip_rnn and not ar.hip and not ar.hip_lstm
    ref = _oracle_rnn(ar.baseNet)
    g = torch.Generator().manual_seed(7)
    x, dy = torch.randn(B, 128, H, generator=g), torch.randn(B, 128, H, generator=g)
    h0 = 0.5 * torch.randn(nl, B, H, generator=g) if state else None
    ar.hidden = None if h0 is None else h0.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = ar(xd)
    assert out._cpc_abs_bound == 1.0
    (out * dy.to(dev)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr, hr = ref(xr, None if h0 is None else h0.double())
    (yr * dy.double()).sum().backward()
    assert (out.detach().cpu().double() - yr).abs().max().item() < 1e-4
    assert not ar.hidden.requires_grad and (ar.hidden.cpu().double() - hr).abs().max().item() < 1e-4
    assert _rel(xd.grad.cpu(), xr.grad) < 1e-4
    bad = {}
    for l in range(nl):
        for n in NAMES:
            e = _rel(getattr(ar.baseNet, f"{n}_l{l}").grad.cpu(), getattr(ref, f"{n}_l{l}").grad)
            if not e < 1e-4:
                bad[f"{n}_l{l}"] = e
    assert not bad, bad


def test_rnn_keep_hidden_carries_the_state_like_the_reference():
    """keepHidden: three calls, each starting from the previous call's detached state -- as nn.RNN does when handed it."""
    dev = _dev()
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(4)
    ar = CPCAR(256, 256, True, 1, mode="RNN", rnnKernel=True).to(dev)
    ref = _oracle_rnn(ar.baseNet)
    state = None
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        x = torch.randn(8, 128, H, generator=g)
        out = ar(x.to(dev))
        assert torch.is_tensor(ar.hidden) and not ar.hidden.requires_grad
        with torch.no_grad():
            yr, state = ref(x.double(), state)
        assert (out.detach().cpu().double() - yr).abs().max().item() < 1e-4
        assert (ar.hidden.cpu().double() - state).abs().max().item() < 1e-4


def test_rnn_reverse_mode_and_the_module_without_the_keyword():
    dev = _dev()
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(5)
    ar = CPCAR(256, 256, False, 2, mode="RNN", reverse=True, rnnKernel=True).to(dev)
    ref = _oracle_rnn(ar.baseNet)
    x = torch.randn(4, 128, H, generator=torch.Generator().manual_seed(2))
    xd = x.to(dev).requires_grad_(True)
    out = ar(xd)
    out.square().sum().backward()
    xr = x.double().requires_grad_(True)
    yr = torch.flip(ref(torch.flip(xr, [1]))[0], [1])
    yr.square().sum().backward()
    assert (out.detach().cpu().double() - yr).abs().max().item() < 1e-4
    assert _rel(xd.grad.cpu(), xr.grad) < 1e-4
    assert _rel(ar.baseNet.weight_hh_l1.grad.cpu(), ref.weight_hh_l1.grad) < 1e-4
    assert ar.hidden is None
    # without the keyword: baseNet's own forward, bit for bit
    plain = CPCAR(256, 256, False, 2, mode="RNN", reverse=True).to(dev)
    plain.load_state_dict(ar.state_dict())
    assert not plain.hip_rnn
    with torch.no_grad():
        want = torch.flip(plain.baseNet(torch.flip(x.to(dev), [1]))[0], [1])
        got = plain(x.to(dev))
    assert torch.equal(got, want) and not hasattr(got, "_cpc_abs_bound")
