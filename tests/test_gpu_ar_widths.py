"""model.CPCAR with inputKernel=True on an MI355X: the GRU, LSTM and RNN autoregressors behind an encoder of another width than
256 (layer 0's input projection in csrc/in_proj.hip, the 256-wide HIP recurrences behind it) against torch.nn.GRU / nn.LSTM /
nn.RNN in float64 on the CPU.  Bar (tests/test_gpu_lstm.py): max |delta| < 1e-4 on the outputs, norm-wise relative error
< 1e-4 on dx and every parameter gradient."""
import copy

import pytest
import torch

from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

BAR = 1e-4
NL = {"GRU": 2, "LSTM": 1, "RNN": 1}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _ar(mode, D, nl, dev, seed=0, **kw):
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(seed)
    ar = CPCAR(D, 256, kw.pop("keepHidden", False), nl, mode=mode, inputKernel=True, lstmKernel=True, rnnKernel=True, **kw).to(dev)
    assert ar.hip_in and not ar.hip and not ar.hip_lstm and not ar.hip_rnn
    return ar, copy.deepcopy(ar.baseNet).cpu().double()


def _forward_backward(ar, ref, x, dy, dev):
    """One forward + backward on the device and through the float64 copy -> (y, dx, grads), (y, dx, grads) of the reference."""
    ar.zero_grad()
    ref.zero_grad()
    xd = x.to(dev).requires_grad_(True)
    y = ar(xd)
    assert getattr(y, "_cpc_abs_bound", None) == 1.0
    (y * dy.to(dev)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr, _ = ref(xr)
    (yr * dy.double()).sum().backward()
    return (y, xd.grad, {n: p.grad for n, p in ar.baseNet.named_parameters()}), \
        (yr.detach(), xr.grad, {n: p.grad for n, p in ref.named_parameters()})


def _compare(got, want):
    assert (got[0].detach().double().cpu() - want[0]).abs().max().item() < BAR
    assert rel_err(got[1], want[1]) < BAR
    assert set(got[2]) == set(want[2])
    bad = {n: rel_err(g, want[2][n]) for n, g in got[2].items() if not rel_err(g, want[2][n]) < BAR}
    assert not bad, bad


@pytest.mark.parametrize("D", [13, 40, 512])
@pytest.mark.parametrize("B,S", [(2, 33), (20, 33)])
@pytest.mark.parametrize("mode", ["GRU", "LSTM", "RNN"])
def test_autoregressors_at_other_input_widths_against_float64(mode, B, S, D):
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(mode, D, NL[mode], dev, seed=D)
    g = torch.Generator().manual_seed(B + D)
    x, dy = torch.randn(B, S, D, generator=g), torch.randn(B, S, 256, generator=g)
    got, want = _forward_backward(ar, ref, x, dy, dev)
    assert tuple(got[1].shape) == (B, S, D) and tuple(got[2]["weight_ih_l0"].shape) == (ref.weight_ih_l0.shape[0], D)
    _compare(got, want)
    ops.check_device_errors(clear=True)


def test_gru_at_the_workload_s_grid():
    """B = 64, S = 128, D = 40: the persistent launches at the flagship batch, the projection at 8192 rows (32 row splits of dW),
    inputs of MFCC size (x scaled by 30)."""
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar("GRU", 40, 2, dev, seed=1)
    g = torch.Generator().manual_seed(7)
    x, dy = 30.0 * torch.randn(64, 128, 40, generator=g), torch.randn(64, 128, 256, generator=g)
    got, want = _forward_backward(ar, ref, x, dy, dev)
    _compare(got, want)
    again, _ = _forward_backward(ar, ref, x, dy, dev)               # no float atomics on the way: the same bits
    assert torch.equal(again[1], got[1]) and torch.equal(again[2]["weight_ih_l0"], got[2]["weight_ih_l0"])
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("mode", ["GRU", "LSTM", "RNN"])
def test_keep_hidden_carries_the_state_over_three_calls(mode):
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(mode, 40, NL[mode], dev, seed=3, keepHidden=True)
    g = torch.Generator().manual_seed(4)
    state = None
    for call in range(3):
        x = torch.randn(3, 17, 40, generator=g)
        with torch.no_grad():
            y = ar(x.to(dev))
            yr, state = ref(x.double(), state)
        assert (y.double().cpu() - yr).abs().max().item() < BAR, call
        kept = ar.hidden if isinstance(ar.hidden, tuple) else (ar.hidden,)
        for a, b in zip(kept, state if isinstance(state, tuple) else (state,)):
            assert (a.double().cpu() - b).abs().max().item() < BAR, call
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("mode", ["GRU", "LSTM", "RNN"])
def test_reverse_runs_the_sequence_back_to_front(mode):
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(mode, 13, NL[mode], dev, seed=5, reverse=True)
    g = torch.Generator().manual_seed(6)
    x, dy = torch.randn(3, 21, 13, generator=g), torch.randn(3, 21, 256, generator=g)
    xd = x.to(dev).requires_grad_(True)
    y = ar(xd)
    (y * dy.to(dev)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr = torch.flip(ref(torch.flip(xr, [1]))[0], [1])
    (yr * dy.double()).sum().backward()
    assert (y.detach().double().cpu() - yr.detach()).abs().max().item() < BAR
    assert rel_err(xd.grad, xr.grad) < BAR
    for n, p in ar.baseNet.named_parameters():
        assert rel_err(p.grad, dict(ref.named_parameters())[n].grad) < BAR, n
    ops.check_device_errors(clear=True)


def test_rnn_function_takes_the_time_major_layout_at_another_width():
    """ops.RnnFunction(time_major=True) on x (T,R,40): nn.RNN without batch_first in float64."""
    dev = _dev()
    from cpc_audio_amd import ops
    torch.manual_seed(8)
    net = torch.nn.RNN(40, 256, 1).to(dev)
    ref = copy.deepcopy(net).cpu().double()
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(21, 5, 40, generator=g), torch.randn(21, 5, 256, generator=g)
    xd = x.to(dev).requires_grad_(True)
    y, hN = ops.RnnFunction.apply(xd, None, True, False, *[getattr(net, n) for n in net._flat_weights_names])
    (y * dy.to(dev)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr, hr = ref(xr)
    (yr * dy.double()).sum().backward()
    assert (y.detach().double().cpu() - yr.detach()).abs().max().item() < BAR
    assert (hN.double().cpu() - hr.detach()).abs().max().item() < BAR
    assert rel_err(xd.grad, xr.grad) < BAR
    for n, p in net.named_parameters():
        assert rel_err(p.grad, dict(ref.named_parameters())[n].grad) < BAR, n
    ops.check_device_errors(clear=True)


def test_functions_reject_widths_they_do_not_take():
    dev = _dev()
    from cpc_audio_amd import ops
    gru = torch.nn.GRU(600, 256, 1, batch_first=True).to(dev)
    with pytest.raises(NotImplementedError):
        ops.GruFunction.apply(torch.zeros(2, 3, 600, device=dev), None, *[getattr(gru, n) for n in gru._flat_weights_names])
    gru = torch.nn.GRU(40, 256, 1, batch_first=True).to(dev)
    with pytest.raises(NotImplementedError):                       # x and weight_ih_l0 disagree
        ops.GruFunction.apply(torch.zeros(2, 3, 44, device=dev), None, *[getattr(gru, n) for n in gru._flat_weights_names])
    ops.check_device_errors(clear=True)


def test_the_mfcc_model_end_to_end():
    """build_model(mfcc, 40 coefficients, inputKernel=True) + the criterion at that width, B = 2, L = 4000: the loss and every
    gradient against the same model with the torch GRU in the middle; the fused step still declines the configuration."""
    dev = _dev()
    from cpc_audio_amd import ops, train
    K, N, B, L = 5, 16, 2, 4000
    torch.manual_seed(11)
    m = train.build_model(encoder_type="mfcc", hiddenEncoder=40, mfccKernel=True, inputKernel=True).to(dev)
    crit = train.build_criterion(hiddenEncoder=40, nPredicts=K, negativeSamplingExt=N, sizeWindow=L).to(dev)
    assert m.gAR.hip_in and not m.gAR.hip
    m0 = train.build_model(encoder_type="mfcc", hiddenEncoder=40, mfccKernel=True).to(dev)
    m0.load_state_dict(m.state_dict(), strict=True)
    crit0 = copy.deepcopy(crit)
    wave = (0.1 * torch.randn(B, 1, L, generator=torch.Generator().manual_seed(5))).clamp_(-1, 1).to(dev)
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    S = (L - 1) // 160 + 1                                          # MFCCEncoder's frames
    bi, si = O.draw_negative_indices(B, S, S - K, N, generator=torch.Generator().manual_seed(9))
    neg = (bi.to(dev), si.to(dev))
    out = []
    for model, cr in ((m, crit), (m0, crit0)):
        c, z, _ = model(wave, None)
        assert tuple(c.shape) == (B, S, 256) and tuple(z.shape) == (B, S, 40)
        losses, acc = cr(c, z, None, negatives=neg)
        losses.sum().backward()
        out.append(losses.detach())
    l1, l0 = out
    print("losses", l1.tolist(), l0.tolist())
    assert bool(((l1 - l0).abs() <= BAR * l0.abs().clamp_min(1.0)).all()), (l1, l0)
    pairs = list(zip(m.named_parameters(), m0.parameters())) + list(zip(crit.named_parameters(), crit0.parameters()))
    assert len(pairs) >= 8 + K                                     # the GRU's eight tensors and the K prediction heads
    errs = {n: rel_err(p.grad, q.grad) for (n, p), q in pairs}
    print("gradient errors", errs)
    assert all(e < BAR for e in errs.values()), errs
    ops.check_device_errors(clear=True)
