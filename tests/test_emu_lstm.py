"""LSTM kernels (csrc/lstm.hip) on the host SIMT emulator against torch.nn.LSTM in float64 on the CPU -- what the reference's
CPCAR runs for its default --arMode LSTM (cpc/model.py:167-169)."""
import ctypes

import pytest
import torch

from emu_util import P, emu, rel_err

H = 256
PER_STEP = 1        # CPC_LSTM_PER_STEP


def _params(nl, seed):
    """4*nl tensors in torch.nn.LSTM state-dict order, with nn.LSTM's own initialisation (U(-1/16, 1/16))."""
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(H, H, num_layers=nl, batch_first=True)
    return [getattr(ref, f"{w}_l{l}").detach().clone().contiguous()
            for l in range(nl) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _oracle(plist, x, state, dy):
    nl = len(plist) // 4
    ref = torch.nn.LSTM(H, H, num_layers=nl, batch_first=True).double()
    with torch.no_grad():
        for l in range(nl):
            for k, w in enumerate(("weight_ih", "weight_hh", "bias_ih", "bias_hh")):
                getattr(ref, f"{w}_l{l}").copy_(plist[4 * l + k].double())
    xr = x.double().clone().requires_grad_(True)
    st = None if state is None else tuple(t.double() for t in state)
    y, (hN, cN) = ref(xr, st)
    (y * dy.double()).sum().backward()
    grads = [getattr(ref, f"{w}_l{l}").grad for l in range(nl) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return y.detach(), hN.detach(), cN.detach(), xr.grad, grads


def _run(lib, B, S, nl, use_state, flags=0, seed=0):
    plist = _params(nl, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, S, H, generator=g)
    state = (0.5 * torch.randn(nl, B, H, generator=g), torch.randn(nl, B, H, generator=g)) if use_state else None
    dy = torch.randn(B, S, H, generator=g)
    h0, c0 = (None, None) if state is None else state
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_lstm_layout(B, S, nl, sizes) == 0
    saved = torch.full((sizes[0],), float("nan"))
    fscr = torch.full((sizes[1],), float("nan"))
    y = torch.full((B, S, H), float("nan"))
    hN = torch.full((nl, B, H), float("nan"))
    cN = torch.full((nl, B, H), float("nan"))
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    assert lib.cpc_lstm_forward(P(x), P(h0), P(c0), parr, P(saved), P(fscr), P(y), P(hN), P(cN), B, S, nl, flags, None) == 0
    bscr = torch.full((sizes[2],), float("nan"))
    dx = torch.full((B, S, H), float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in plist]
    garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
    assert lib.cpc_lstm_backward(P(x), P(h0), P(c0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, flags,
                                 None) == 0
    return (plist, x, state, dy), [y, hN, cN, dx] + grads


def _check(inputs, outs):
    plist, x, state, dy = inputs
    yr, hr, cr, dxr, gr = _oracle(plist, x, state, dy)
    y, hN, cN, dx, *grads = outs
    assert (y.double() - yr).abs().max().item() < 1e-5
    assert (hN.double() - hr).abs().max().item() < 1e-5
    assert (cN.double() - cr).abs().max().item() < 1e-5
    assert rel_err(dx.double(), dxr) < 1e-5
    bad = {k: rel_err(g.double(), r) for k, (g, r) in enumerate(zip(grads, gr)) if not rel_err(g.double(), r) < 1e-5}
    assert not bad, bad


@pytest.mark.parametrize("use_state", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("S", [1, 7, 33])
@pytest.mark.parametrize("B", [1, 5, 16, 20])
def test_lstm_forward_backward_match_torch_float64_emulated(B, S, nl, use_state):
    """y, hN, cN, dx and all 4*nl parameter gradients of the persistent path against nn.LSTM in float64."""
    lib = emu()
    inputs, outs = _run(lib, B, S, nl, use_state)
    _check(inputs, outs)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("B,S,nl,use_state", [(5, 7, 1, False), (20, 9, 2, True), (16, 33, 1, True), (1, 1, 2, False)])
def test_persistent_and_per_step_paths_agree_bit_for_bit_emulated(B, S, nl, use_state):
    """The persistent recurrence and the one-launch-per-step kernels (CPC_LSTM_PER_STEP) use the same MFMAs and the same
    summation order: every output and gradient is bit-identical."""
    lib = emu()
    inputs, a = _run(lib, B, S, nl, use_state, flags=0)
    _, b = _run(lib, B, S, nl, use_state, flags=PER_STEP)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
    _check(inputs, b)


def test_shape_and_argument_errors_are_returned_before_any_launch_emulated():
    lib = emu()
    B, S, nl = 3, 4, 1
    sizes = (ctypes.c_long * 3)()
    for bad in [(0, S, 1), (B, 0, 1), (B, S, 0), (B, S, 9), (1 << 12, 1 << 10, 1)]:
        assert lib.cpc_lstm_layout(*bad, sizes) == 1, bad          # CPC_ERR_SHAPE
    assert lib.cpc_lstm_layout(B, S, 8, sizes) == 0
    assert lib.cpc_lstm_layout(B, S, nl, None) == 2                # CPC_ERR_ARG
    assert lib.cpc_lstm_layout(B, S, nl, sizes) == 0
    plist = _params(nl, 0)
    parr = (ctypes.c_void_p * 4)(*[P(t) for t in plist])
    x = torch.randn(B, S, H)
    h0 = torch.zeros(nl, B, H)
    saved, fscr, bscr = (torch.full((sizes[k],), 7.0) for k in range(3))
    y = torch.full((B, S, H), 7.0)
    hN, cN = torch.full((nl, B, H), 7.0), torch.full((nl, B, H), 7.0)
    dx = torch.full((B, S, H), 7.0)
    grads = [torch.full_like(t, 7.0) for t in plist]
    garr = (ctypes.c_void_p * 4)(*[P(t) for t in grads])

    short = (ctypes.c_void_p * 8)(*[P(t) for t in plist], None, None, None, None)

    def fwd(**kw):
        a = dict(x=P(x), h0=None, c0=None, params=parr, saved=P(saved), scratch=P(fscr), y=P(y), hN=P(hN), cN=P(cN), B=B, S=S,
                 nl=nl, flags=0)
        a.update(kw)
        return lib.cpc_lstm_forward(*a.values(), None)

    def bwd(**kw):
        a = dict(x=P(x), h0=None, c0=None, params=parr, saved=P(saved), y=P(y), dy=P(y), scratch=P(bscr), dx=P(dx),
                 grads=garr, B=B, S=S, nl=nl, flags=0)
        a.update(kw)
        return lib.cpc_lstm_backward(*a.values(), None)

    for call in (fwd, bwd):
        assert call(B=0) == 1 and call(S=0) == 1 and call(nl=9) == 1
        assert call(nl=2, params=short) == 2                       # 8 parameter pointers expected, 4 of them NULL
        assert call(flags=2) == 2                                  # unknown flag bit
        assert call(x=None) == 2
        assert call(h0=P(h0)) == 2                                 # h0 without c0
        assert call(c0=P(h0)) == 2
        assert call(params=None) == 2
    assert fwd(y=None) == 2 and fwd(hN=None) == 2 and fwd(cN=None) == 2 and fwd(saved=None) == 2 and fwd(scratch=None) == 2
    assert bwd(dy=None) == 2 and bwd(dx=None) == 2 and bwd(grads=None) == 2 and bwd(scratch=None) == 2
    nulls = (ctypes.c_void_p * 4)(garr[0], garr[1], None, garr[3])
    assert bwd(grads=nulls) == 2
    # nothing was launched: every output still holds its fill
    for t in [saved, fscr, bscr, y, hN, cN, dx] + grads:
        assert bool((t == 7.0).all())
