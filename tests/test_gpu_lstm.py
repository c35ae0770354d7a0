"""The HIP LSTM autoregressor (csrc/lstm.hip, ops.LstmFunction, CPCAR(mode="LSTM", lstmKernel=True)) on the MI355X against
torch.nn.LSTM in float64 on the CPU -- what the reference's CPCAR runs for its default --arMode LSTM (cpc/model.py:167-169)."""
import pytest
import torch

from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

H = 256
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _oracle_lstm(net):
    ref = torch.nn.LSTM(H, H, num_layers=net.num_layers, batch_first=True).double()
    with torch.no_grad():
        for l in range(net.num_layers):
            for n in NAMES:
                getattr(ref, f"{n}_l{l}").copy_(getattr(net, f"{n}_l{l}").detach().cpu().double())
    return ref


def _run_function(dev, B, S, nl, per_step, state, seed=0):
    from cpc_audio_amd.ops import LstmFunction
    torch.manual_seed(seed)
    net = torch.nn.LSTM(H, H, num_layers=nl, batch_first=True)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, S, H, generator=g)
    st = (0.5 * torch.randn(nl, B, H, generator=g), torch.randn(nl, B, H, generator=g)) if state else None
    dy = torch.randn(B, S, H, generator=g)
    params = [getattr(net, f"{n}_l{l}").detach().to(dev).requires_grad_(True) for l in range(nl) for n in NAMES]
    xd = x.to(dev).requires_grad_(True)
    y, hN, cN = LstmFunction.apply(xd, None if st is None else tuple(t.to(dev) for t in st), per_step, *params)
    (y * dy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    outs = [y.detach().cpu(), hN.cpu(), cN.cpu(), xd.grad.cpu()] + [p.grad.cpu() for p in params]
    return net, (x, st, dy), outs


@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("B", [2, 64, 256])
def test_lstm_matches_torch_float64_and_paths_agree_bit_for_bit(B, nl, state):
    """S = 128 (20480 samples / 160): y, hN, cN, dx and every parameter gradient against nn.LSTM in float64; the persistent
    recurrence and the per-step kernels (CPC_LSTM_PER_STEP) give the same bits."""
    dev = _dev()
    from cpc_audio_amd import ops
    ops.check_device_errors(clear=True)
    S = 128
    net, (x, st, dy), a = _run_function(dev, B, S, nl, False, state)
    _, _, b = _run_function(dev, B, S, nl, True, state)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
    ref = _oracle_lstm(net)
    xr = x.double().requires_grad_(True)
    yr, (hr, cr) = ref(xr, None if st is None else tuple(t.double() for t in st))
    (yr * dy.double()).sum().backward()
    y, hN, cN, dx, *grads = a
    assert (y.double() - yr).abs().max().item() < 1e-4
    assert (hN.double() - hr).abs().max().item() < 1e-4
    assert (cN.double() - cr).abs().max().item() < 1e-4
    assert _rel(dx, xr.grad) < 1e-4
    want = [getattr(ref, f"{n}_l{l}").grad for l in range(nl) for n in NAMES]
    bad = {k: _rel(g, w) for k, (g, w) in enumerate(zip(grads, want)) if not _rel(g, w) < 1e-4}
    assert not bad, bad
    ops.check_device_errors(clear=True)                 # raises on any flagged device error


def test_keep_hidden_carries_h_and_c_like_the_reference():
    """keepHidden: three calls, each starting from the previous call's detached (h, c) -- as nn.LSTM does when handed it."""
    dev = _dev()
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(4)
    ar = CPCAR(256, 256, True, 1, mode="LSTM", lstmKernel=True).to(dev)
    assert ar.hip_lstm and not ar.hip
    ref = _oracle_lstm(ar.baseNet)
    state = None
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        x = torch.randn(8, 128, H, generator=g)
        out = ar(x.to(dev))
        assert out._cpc_abs_bound == 1.0
        assert isinstance(ar.hidden, tuple) and len(ar.hidden) == 2 and not ar.hidden[0].requires_grad
        with torch.no_grad():
            yr, state = ref(x.double(), state)
        assert (out.detach().cpu().double() - yr).abs().max().item() < 1e-4
        assert (ar.hidden[0].cpu().double() - state[0]).abs().max().item() < 1e-4
        assert (ar.hidden[1].cpu().double() - state[1]).abs().max().item() < 1e-4


def test_reverse_mode_matches_the_flipped_reference():
    dev = _dev()
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(5)
    ar = CPCAR(256, 256, False, 2, mode="LSTM", reverse=True, lstmKernel=True).to(dev)
    ref = _oracle_lstm(ar.baseNet)
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


def test_trainer_step_with_the_lstm_kernel_matches_nn_lstm():
    """One Trainer step of the reference-default model (LSTM, one level, 256 / 256, linear criterion) at B = 8 with the HIP LSTM
    against the same model on nn.LSTM: loss, every parameter gradient, and the parameters after Adam."""
    dev = _dev()
    from cpc_audio_amd import ops
    from cpc_audio_amd.model import CPCAR, CPCEncoder, CPCModel
    from cpc_audio_amd.train import Trainer, build_criterion
    B = 8
    torch.manual_seed(11)
    base = CPCModel(CPCEncoder(256), CPCAR(256, 256, False, 1, mode="LSTM"))
    crit0 = build_criterion()
    wave = O.make_waveform(B, 20480, seed=5).to(dev)
    bi, si = O.draw_negative_indices(B, 128, 116, 128, generator=torch.Generator().manual_seed(6))
    neg = (bi.to(dev), si.to(dev))
    runs = {}
    for kernel in (True, False):
        model = CPCModel(CPCEncoder(256), CPCAR(256, 256, False, 1, mode="LSTM", lstmKernel=kernel))
        model.load_state_dict(base.state_dict())
        crit = build_criterion()
        crit.load_state_dict(crit0.state_dict())
        model, crit = model.to(dev), crit.to(dev)
        assert model.gAR.hip_lstm == kernel and not model.gAR.hip
        tr = Trainer(model, crit)
        seen = {}
        step = tr.optimizer.step

        def snap(*a, **kw):
            for n, p in list(model.named_parameters()) + list(crit.named_parameters()):
                seen[n] = p.grad.detach().cpu().clone()
            return step(*a, **kw)

        tr.optimizer.step = snap
        losses, _ = tr.step(wave, None, negatives=neg)
        torch.cuda.synchronize()
        state = dict(model.state_dict())
        state.update({"crit." + k: v for k, v in crit.state_dict().items()})
        runs[kernel] = (losses.cpu(), seen, {k: v.detach().cpu().clone() for k, v in state.items()})
    (la, ga, pa), (lb, gb, pb) = runs[True], runs[False]
    assert (la - lb).abs().max().item() < 1e-4
    assert ga.keys() == gb.keys() and len(ga) > 0
    bad = {k: _rel(ga[k], gb[k]) for k in ga if not _rel(ga[k], gb[k]) < 1e-4}
    assert not bad, bad
    bad = {k: _rel(pa[k], pb[k]) for k in pa if not _rel(pa[k], pb[k]) < 1e-4}
    assert not bad, bad
    ops.check_device_errors(clear=True)                 # raises on any flagged device error
