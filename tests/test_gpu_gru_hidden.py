"""The GRU at any hidden width on an MI355X (csrc/gru.hip: cpc_gru_*_h; ops.GruHiddenFunction): model.CPCAR in mode GRU with
hiddenKernel=True and the model + criterion at --hiddenGar 512 against torch.nn.GRU.
Bar (tests/test_gpu_lstm_hidden.py, tests/test_gpu_ar_widths.py): max |delta| < 1e-4 on the outputs, norm-wise relative error
< 1e-4 on dx and every parameter gradient, against nn.GRU in float64 on the CPU."""
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
    ar = CPCAR(D, H, kw.pop("keepHidden", False), nl, mode="GRU", hiddenKernel=True, **kw).to(dev)
    assert ar.hip_gru_hidden and not ar.hip and not ar.hip_hidden and not ar.hip_lstm and not ar.hip_in and not ar.hip_rnn
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
def test_gru_at_other_hidden_widths_against_float64(D, H, B, nl):
    dev = _dev()
    from cpc_audio_amd import ops
    S = 33
    ar, ref = _ar(D, H, nl, dev, seed=D + H)
    g = torch.Generator().manual_seed(B + D)
    x, dy = torch.randn(B, S, D, generator=g), torch.randn(B, S, H, generator=g)
    got, want = _forward_backward(ar, ref, x, dy, dev)
    assert tuple(got[0].shape) == (B, S, H) and tuple(got[1].shape) == (B, S, D)
    assert tuple(got[2]["weight_ih_l0"].shape) == (3 * H, D) and tuple(got[2]["weight_hh_l0"].shape) == (3 * H, H)
    assert tuple(got[2]["bias_ih_l0"].shape) == (3 * H,) and tuple(got[2]["bias_hh_l0"].shape) == (3 * H,)
    if nl == 2:
        assert tuple(got[2]["weight_ih_l1"].shape) == (3 * H, H)
    _compare(got, want)
    ops.check_device_errors(clear=True)


def test_gru_512_at_the_workload_s_grid():
    """B = 64, S = 128, (256, 512), two layers: 32 unit tiles x 4 batch tiles = 128 workgroups, resident together on the 256
    CUs, so all four recurrences are the persistent kernels; run twice, dx and weight_hh_l0.grad are the same bits (no float
    atomics)."""
    dev = _dev()
    from cpc_audio_amd import ops
    ar, ref = _ar(256, 512, 2, dev, seed=1)
    g = torch.Generator().manual_seed(7)
    x, dy = torch.randn(64, 128, 256, generator=g), torch.randn(64, 128, 512, generator=g)
    ops.gru_hidden_paths(clear=True)
    got, want = _forward_backward(ar, ref, x, dy, dev)
    paths = ops.gru_hidden_paths(clear=True)
    if torch.cuda.get_device_properties(dev).multi_processor_count >= 256:
        assert paths == {"persistent"}, paths
    _compare(got, want)
    again, _ = _forward_backward(ar, ref, x, dy, dev)
    assert torch.equal(again[1], got[1]) and torch.equal(again[2]["weight_hh_l0"], got[2]["weight_hh_l0"])
    ops.check_device_errors(clear=True)


def test_keep_hidden_carries_the_state_over_three_calls():
    """From zero and then from the module's own last state: the bound tag is there on every call; a state assigned from outside
    carries none."""
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
        assert getattr(y, "_cpc_abs_bound", None) == 1.0, call
        assert (y.double().cpu() - yr).abs().max().item() < BAR, call
        assert tuple(ar.hidden.shape) == (1, 3, 130)
        assert (ar.hidden.double().cpu() - state).abs().max().item() < BAR, call
    outside = 3.0 * torch.randn(1, 3, 130, generator=g)
    ar.hidden = outside.to(dev)
    with torch.no_grad():
        y = ar(x.to(dev))
        yr, _ = ref(x.double(), outside.double())
    assert not hasattr(y, "_cpc_abs_bound")
    assert (y.double().cpu() - yr).abs().max().item() < BAR
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
    net = torch.nn.GRU(D, H, 2, batch_first=True).to(dev)
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(B, S, D, generator=g).to(dev), torch.randn(B, S, H, generator=g).to(dev)
    h0 = (0.5 * torch.randn(2, B, H, generator=g)).to(dev)
    params = [getattr(net, n) for n in net._flat_weights_names]
    out = []
    for per_step in (False, True):
        net.zero_grad()
        ops.gru_hidden_paths(clear=True)
        xd = x.clone().requires_grad_(True)
        y, hN = ops.GruHiddenFunction.apply(xd, h0, per_step, *params)
        (y * dy).sum().backward()
        assert ops.gru_hidden_paths(clear=True) == ({"per_step"} if per_step else {"persistent"})
        out.append([y.detach(), hN, xd.grad] + [p.grad.clone() for p in params])
    for k, (u, v) in enumerate(zip(*out)):
        assert torch.equal(u, v), k
    ops.check_device_errors(clear=True)


def test_the_model_at_hidden_gar_512_end_to_end():
    """build_model(hiddenGar=512, hiddenKernel=True) -- the package's default GRU of two layers -- + the criterion at that context
    width, B = 2, one window: the loss and every gradient against the same weights with the torch GRU in the middle; the fused
    step still declines."""
    dev = _dev()
    from cpc_audio_amd import ops, train
    K, N, B, L = 5, 16, 2, 20480
    torch.manual_seed(11)
    m = train.build_model(hiddenGar=512, hiddenKernel=True).to(dev)
    crit = train.build_criterion(hiddenGar=512, nPredicts=K, negativeSamplingExt=N).to(dev)
    assert m.gAR.hip_gru_hidden and not m.gAR.hip and m.gAR.baseNet.num_layers == 2
    m0 = train.build_model(hiddenGar=512).to(dev)
    assert not m0.gAR.hip_gru_hidden
    m0.load_state_dict(m.state_dict(), strict=True)
    crit0 = copy.deepcopy(crit)
    wave = (0.1 * torch.randn(B, 1, L, generator=torch.Generator().manual_seed(5))).clamp_(-1, 1).to(dev)
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    S = L // 160
    bi, si = O.draw_negative_indices(B, S, S - K, N, generator=torch.Generator().manual_seed(9))
    neg = (bi.to(dev), si.to(dev))
    out = []
    ops.gru_hidden_paths(clear=True)
    for model, cr in ((m, crit), (m0, crit0)):
        c, z, _ = model(wave, None)
        assert tuple(c.shape) == (B, S, 512) and tuple(z.shape) == (B, S, 256)
        losses, acc = cr(c, z, None, negatives=neg)
        losses.sum().backward()
        out.append(losses.detach())
    assert ops.gru_hidden_paths(clear=True)                  # the kernels ran (forward and backward of the first model)
    l1, l0 = out
    print("losses", l1.tolist(), l0.tolist())
    assert bool(((l1 - l0).abs() <= BAR * l0.abs().clamp_min(1.0)).all()), (l1, l0)
    pairs = list(zip(m.named_parameters(), m0.parameters())) + list(zip(crit.named_parameters(), crit0.parameters()))
    assert len(pairs) >= 8 + K
    errs = {n: rel_err(p.grad, q.grad) for (n, p), q in pairs}
    print("gradient errors", errs)
    assert all(e < BAR for e in errs.values()), errs
    ops.check_device_errors(clear=True)
