"""The LSTM at any hidden width on an MI355X (csrc/lstm.hip: cpc_lstm_*_h; ops.LstmHiddenFunction): model.CPCAR with
hiddenKernel=True, the model + criterion at --hiddenGar 512 and the PER classifier's front against torch.nn.LSTM.
Bar (tests/test_gpu_lstm.py, tests/test_gpu_ar_widths.py): max |delta| < 1e-4 on the outputs, norm-wise relative error < 1e-4
on dx and every parameter gradient, against nn.LSTM in float64 on the CPU."""
import copy

import pytest
import torch

from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

BAR = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _ar(D, H, nl, dev, seed=0, **kw):
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(seed)
    ar = CPCAR(D, H, kw.pop("keepHidden", False), nl, mode="LSTM", lstmKernel=True, hiddenKernel=True, **kw).to(dev)
    assert ar.hip_hidden and not ar.hip and not ar.hip_lstm and not ar.hip_in and not ar.hip_rnn
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


CASES = [(D, H, B, 1) for D, H in [(13, 13), (256, 64), (40, 130), (256, 272), (256, 512), (512, 512)] for B in (2, 20)] + \
    [(40, 130, 2, 2), (40, 130, 20, 2), (256, 512, 2, 2), (256, 512, 20, 2)]


@pytest.mark.parametrize("D,H,B,nl", CASES)
def test_lstm_at_other_hidden_widths_against_float64(D, H, B, nl):
    dev = _dev()
    from cpc_audio_amd import ops
    S = 33
    ar, ref = _ar(D, H, nl, dev, seed=D + H)
    g = torch.Generator().manual_seed(B + D)
    x, dy = torch.randn(B, S, D, generator=g), torch.randn(B, S, H, generator=g)
    got, want = _forward_backward(ar, ref, x, dy, dev)
    assert tuple(got[0].shape) == (B, S, H) and tuple(got[1].shape) == (B, S, D)
    assert tuple(got[2]["weight_ih_l0"].shape) == (4 * H, D) and tuple(got[2]["weight_hh_l0"].shape) == (4 * H, H)
    _compare(got, want)
    ops.check_device_errors(clear=True)


def test_lstm_512_at_the_workload_s_grid():
    """B = 64, S = 128, (256, 512): 32 unit tiles x 4 batch tiles = 128 workgroups, resident together on the 256 CUs, so both
    recurrences are the persistent kernels; run twice, dx and weight_hh_l0.grad are the same bits (no float atomics)."""
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(256, 512, 1, dev, seed=1)
    g = torch.Generator().manual_seed(7)
    x, dy = torch.randn(64, 128, 256, generator=g), torch.randn(64, 128, 512, generator=g)
    ops.lstm_hidden_paths(clear=True)
    got, want = _forward_backward(ar, ref, x, dy, dev)
    paths = ops.lstm_hidden_paths(clear=True)
    if torch.cuda.get_device_properties(dev).multi_processor_count >= 256:
        assert paths == {"persistent"}, paths
    _compare(got, want)
    again, _ = _forward_backward(ar, ref, x, dy, dev)
    assert torch.equal(again[1], got[1]) and torch.equal(again[2]["weight_hh_l0"], got[2]["weight_hh_l0"])
    ops.check_device_errors(clear=True)


def test_keep_hidden_carries_the_state_over_three_calls():
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(40, 130, 1, dev, seed=3, keepHidden=True)
    g = torch.Generator().manual_seed(4)
    state = None
    for call in range(3):
        x = torch.randn(3, 17, 40, generator=g)
        with torch.no_grad():
            y = ar(x.to(dev))
            yr, state = ref(x.double(), state)
        assert (y.double().cpu() - yr).abs().max().item() < BAR, call
        for a, b in zip(ar.hidden, state):
            assert tuple(a.shape) == (1, 3, 130)
            assert (a.double().cpu() - b).abs().max().item() < BAR, call
    ops.check_device_errors(clear=True)


def test_reverse_runs_the_sequence_back_to_front():
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(13, 13, 1, dev, seed=5, reverse=True)
    g = torch.Generator().manual_seed(6)
    x, dy = torch.randn(3, 21, 13, generator=g), torch.randn(3, 21, 13, generator=g)
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


def test_per_step_equals_the_persistent_path_bit_for_bit():
    dev = _dev()
    from cpc_audio_amd import ops
    D, H, B, S = 40, 130, 20, 9
    torch.manual_seed(8)
    net = torch.nn.LSTM(D, H, 2, batch_first=True).to(dev)
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(B, S, D, generator=g).to(dev), torch.randn(B, S, H, generator=g).to(dev)
    state = (0.5 * torch.randn(2, B, H, generator=g).to(dev), torch.randn(2, B, H, generator=g).to(dev))
    params = [getattr(net, n) for n in net._flat_weights_names]
    out = []
    for per_step in (False, True):
        net.zero_grad()
        ops.lstm_hidden_paths(clear=True)
        xd = x.clone().requires_grad_(True)
        y, hN, cN = ops.LstmHiddenFunction.apply(xd, state, per_step, *params)
        (y * dy).sum().backward()
        assert ops.lstm_hidden_paths(clear=True) == ({"per_step"} if per_step else {"persistent"})
        out.append([y.detach(), hN, cN, xd.grad] + [p.grad.clone() for p in params])
    for k, (u, v) in enumerate(zip(*out)):
        assert torch.equal(u, v), k
    ops.check_device_errors(clear=True)


def test_the_model_at_hidden_gar_512_end_to_end():
    """build_model(hiddenGar=512, LSTM, hiddenKernel=True) + the criterion at that context width, B = 2, one window: the loss
    and every gradient against the same weights with the torch LSTM in the middle; the fused step still declines."""
    dev = _dev()
    from cpc_audio_amd import ops, train
    K, N, B, L = 5, 16, 2, 20480
    torch.manual_seed(11)
    kw = dict(hiddenGar=512, arMode="LSTM", nLevelsGRU=1, lstmKernel=True)
    m = train.build_model(hiddenKernel=True, **kw).to(dev)
    crit = train.build_criterion(hiddenGar=512, nPredicts=K, negativeSamplingExt=N).to(dev)
    assert m.gAR.hip_hidden and not m.gAR.hip_lstm
    m0 = train.build_model(**kw).to(dev)
    assert not m0.gAR.hip_hidden
    m0.load_state_dict(m.state_dict(), strict=True)
    crit0 = copy.deepcopy(crit)
    wave = (0.1 * torch.randn(B, 1, L, generator=torch.Generator().manual_seed(5))).clamp_(-1, 1).to(dev)
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    S = L // 160
    bi, si = O.draw_negative_indices(B, S, S - K, N, generator=torch.Generator().manual_seed(9))
    neg = (bi.to(dev), si.to(dev))
    out = []
    for model, cr in ((m, crit), (m0, crit0)):
        c, z, _ = model(wave, None)
        assert tuple(c.shape) == (B, S, 512) and tuple(z.shape) == (B, S, 256)
        losses, acc = cr(c, z, None, negatives=neg)
        losses.sum().backward()
        out.append(losses.detach())
    l1, l0 = out
    print("losses", l1.tolist(), l0.tolist())
    assert bool(((l1 - l0).abs() <= BAR * l0.abs().clamp_min(1.0)).all()), (l1, l0)
    pairs = list(zip(m.named_parameters(), m0.parameters())) + list(zip(crit.named_parameters(), crit0.parameters()))
    assert len(pairs) >= 4 + K
    errs = {n: rel_err(p.grad, q.grad) for (n, p), q in pairs}
    print("gradient errors", errs)
    assert all(e < BAR for e in errs.values()), errs
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("D", [13, 64])
def test_the_per_front_runs_its_lstm_on_the_kernels(D):
    """CTCphone_criterion(D, 41, LSTM, seqNorm) with hipFront, wideKernel and hiddenKernel against the same module with the torch
    front: ragged lengths, the loss and every parameter gradient."""
    dev = _dev()
    from cpc_audio_amd import common_voices_eval as CV
    from cpc_audio_amd import ops
    B, S = 3, 50
    torch.manual_seed(D)
    crit = CV.CTCphone_criterion(D, 41, LSTM=True, seqNorm=True, dropout=False, hipFront=True, wideKernel=True,
                                 hiddenKernel=True).to(dev)
    ref = CV.CTCphone_criterion(D, 41, LSTM=True, seqNorm=True, dropout=False, hipFront=False, wideKernel=True).to(dev)
    ref.load_state_dict(crit.state_dict())
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, S, D, generator=g).to(dev)
    sizes = torch.tensor([50, 37, 44], device=dev)
    label = torch.randint(0, 41, (B, 4), generator=g).to(dev)
    label_size = torch.tensor([4, 2, 3], device=dev)
    loss = crit(x, sizes, label, label_size)
    assert crit.last_front == "hip" and crit.last_lstm == "hip"
    loss.sum().backward()
    want = ref(x, sizes, label, label_size)
    assert ref.last_front == "torch" and ref.last_lstm == "torch"
    want.sum().backward()
    assert bool(((loss - want).abs() <= BAR * want.abs()).all()), (loss, want)
    errs = {n: rel_err(p.grad, dict(ref.named_parameters())[n].grad) for n, p in crit.named_parameters()}
    assert all(e < BAR for e in errs.values()), errs
    off = CV.CTCphone_criterion(D, 41, LSTM=True, seqNorm=True, hipFront=True, wideKernel=True).to(dev)
    off(x, sizes, label, label_size)
    assert off.last_lstm == "torch"                        # without the keyword the recurrence stays where it was
    ops.check_device_errors(clear=True)
