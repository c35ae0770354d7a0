"""The grouped LSTM recurrence (cpc_lstm_group_*, csrc/lstm.hip) and the Elman RNN (cpc_rnn_*, csrc/rnn.hip) on the host SIMT
emulator against torch.nn.LSTM / torch.nn.RNN in float64 on the CPU -- what the reference's --rnnMode LSTM / RNN predictors
(cpc/criterion/criterion.py:62-68) and its --arMode RNN (cpc/model.py:177-180) run.

The emulated device has 64 CUs and an occupancy query of 1 (emu_util), so 64 workgroups are resident: an LSTM head takes
16 * ceil(B/16) of them, an RNN head 4 * ceil(R/16), and the shapes below cover one persistent launch for all heads, heads split
over several launches, and the per-step kernels where not even one head fits.

Bars (tests/test_emu_lstm.py): |dy| < 1e-5 on outputs, rel < 1e-5 on gradients against float64."""
import ctypes

import pytest
import torch

from emu_util import P, emu, rel_err

H = 256
PER_STEP = 1        # CPC_LSTM_PER_STEP, CPC_RNN_PER_STEP
TIME_MAJOR = 2      # CPC_RNN_TIME_MAJOR
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
NAN = float("nan")
PAD = 64            # canary floats on either side of every buffer the library writes


class Guarded:
    """A tensor of ``shape`` inside a NaN-filled block with PAD canaries in front and behind."""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.block = torch.full((n + 2 * PAD,), NAN)
        self.t = self.block[PAD:PAD + n].view(*shape)

    def intact(self):
        return bool(torch.isnan(self.block[:PAD]).all()) and bool(torch.isnan(self.block[-PAD:]).all())


def _heads(cls, G, nl, seed, **kw):
    """G modules of ``cls`` with torch's own initialisation (U(-1/16, 1/16))."""
    torch.manual_seed(seed)
    return [cls(H, H, num_layers=nl, **kw) for _ in range(G)]


def _stack(mods, nl):
    """per layer: weight_ih (G*n,256), weight_hh (G,n,256), bias_ih, bias_hh (G*n): the heads' tensors one behind the other"""
    out = []
    for l in range(nl):
        wi = torch.cat([getattr(m, f"weight_ih_l{l}").detach() for m in mods]).contiguous()
        wh = torch.stack([getattr(m, f"weight_hh_l{l}").detach() for m in mods]).contiguous()
        bi = torch.cat([getattr(m, f"bias_ih_l{l}").detach() for m in mods]).contiguous()
        bh = torch.cat([getattr(m, f"bias_hh_l{l}").detach() for m in mods]).contiguous()
        out += [wi, wh, bi, bh]
    return out


def _oracle(mods, nl, x, dy, h0=None):
    """float64: y with head g at columns g*256.., hN of head 0, dx summed over the heads, the stacked parameter gradients"""
    xr = x.double().clone().requires_grad_(True)
    ys, hN = [], None
    refs = [m.double() for m in mods]
    for m in refs:
        m.zero_grad()
        out, st = m(xr) if h0 is None else m(xr, h0.double())
        ys.append(out)
        hN = st[0] if isinstance(st, tuple) else st
    y = torch.cat(ys, dim=2)
    (y * dy.double()).sum().backward()
    grads = []
    for l in range(nl):
        grads += [torch.cat([getattr(m, f"weight_ih_l{l}").grad for m in refs]),
                  torch.stack([getattr(m, f"weight_hh_l{l}").grad for m in refs]),
                  torch.cat([getattr(m, f"bias_ih_l{l}").grad for m in refs]),
                  torch.cat([getattr(m, f"bias_hh_l{l}").grad for m in refs])]
    return y.detach(), hN.detach(), xr.grad, grads


def _check(outs, ref, with_hN):
    y, hN, dx, grads = outs
    yr, hr, dxr, gr = ref
    assert (y.double() - yr).abs().max().item() < 1e-5
    if with_hN:
        assert (hN.double() - hr).abs().max().item() < 1e-5
    assert rel_err(dx.double(), dxr) < 1e-5
    bad = {k: rel_err(g.double(), r.reshape(g.shape)) for k, (g, r) in enumerate(zip(grads, gr))
           if not rel_err(g.double(), r.reshape(g.shape)) < 1e-5}
    assert not bad, bad


# ------------------------------------------------------------------ LSTM group
def _lstm_group(lib, B, S, G, flags=0, seed=0, mods=None):
    mods = mods or _heads(torch.nn.LSTM, G, 1, seed, batch_first=True)
    params = _stack(mods, 1)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, S, H, generator=g)
    dy = torch.randn(B, S, G * H, generator=g)
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_lstm_group_layout(B, S, G, sizes) == 0
    saved, fscr, bscr = Guarded(sizes[0]), Guarded(sizes[1]), Guarded(sizes[2])
    y, dx = Guarded(B, S, G * H), Guarded(B, S, H)
    grads = [Guarded(*p.shape) for p in params]
    assert lib.cpc_lstm_group_forward(P(x), *[P(p) for p in params], P(saved.t), P(fscr.t), P(y.t), B, S, G, flags, None) == 0
    assert lib.cpc_lstm_group_backward(P(x), P(params[0]), P(params[1]), P(saved.t), P(y.t), P(dy), P(bscr.t), P(dx.t),
                                       *[P(q.t) for q in grads], B, S, G, flags, None) == 0
    for q in [saved, fscr, bscr, y, dx] + grads:
        assert q.intact()
    return (mods, x, dy), (y.t, None, dx.t, [q.t for q in grads])


LSTM_SHAPES = [(1, 1, 1), (5, 7, 3), (16, 2, 2), (20, 7, 3), (70, 3, 2)]


@pytest.mark.parametrize("B,S,G", LSTM_SHAPES)
def test_lstm_group_matches_torch_float64_emulated(B, S, G):
    """y, the summed dx and the four stacked parameter gradients of G heads against G nn.LSTM in float64: one persistent launch
    (with a partial row tile), heads split over two launches (20, 7, 3) and the per-step fallback (70, 3, 2: 80 workgroups a head)."""
    lib = emu()
    (mods, x, dy), outs = _lstm_group(lib, B, S, G)
    assert not torch.isnan(outs[0]).any() and not torch.isnan(outs[2]).any()
    _check(outs, _oracle(mods, 1, x, dy), False)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("B,S,G", [(5, 7, 3), (20, 7, 3)])
def test_lstm_group_per_step_flag_gives_the_same_bits_emulated(B, S, G):
    lib = emu()
    _, a = _lstm_group(lib, B, S, G, flags=0)
    _, b = _lstm_group(lib, B, S, G, flags=PER_STEP)
    for u, v in zip([a[0], a[2]] + a[3], [b[0], b[2]] + b[3]):
        assert torch.equal(u, v)


def test_lstm_group_of_one_gives_the_bits_of_cpc_lstm_emulated():
    """The existing cpc_lstm_* entry points run the same kernels with G = 1: every output and gradient is bit-identical."""
    lib = emu()
    B, S = 5, 7
    (mods, x, dy), g = _lstm_group(lib, B, S, 1)
    plist = [getattr(mods[0], f"{w}_l0").detach().contiguous() for w in NAMES]
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_lstm_layout(B, S, 1, sizes) == 0
    saved, fscr, bscr = (torch.full((sizes[k],), NAN) for k in range(3))
    y, hN, cN, dx = torch.full((B, S, H), NAN), torch.full((1, B, H), NAN), torch.full((1, B, H), NAN), torch.full((B, S, H), NAN)
    grads = [torch.full_like(t, NAN) for t in plist]
    parr = (ctypes.c_void_p * 4)(*[P(t) for t in plist])
    garr = (ctypes.c_void_p * 4)(*[P(t) for t in grads])
    assert lib.cpc_lstm_forward(P(x), None, None, parr, P(saved), P(fscr), P(y), P(hN), P(cN), B, S, 1, 0, None) == 0
    assert lib.cpc_lstm_backward(P(x), None, None, parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, 1, 0, None) == 0
    assert torch.equal(y, g[0]) and torch.equal(dx, g[2])
    assert torch.equal(hN[0], y[:, -1])
    for u, v in zip(grads, g[3]):
        assert torch.equal(u, v.reshape(u.shape))


def test_lstm_group_heads_are_independent_emulated():
    """Changing one head's weights leaves every other head's y bit-identical."""
    lib = emu()
    B, S, G = 5, 7, 3
    mods = _heads(torch.nn.LSTM, G, 1, 0, batch_first=True)
    _, a = _lstm_group(lib, B, S, G, mods=mods)
    with torch.no_grad():
        mods[1].weight_hh_l0.mul_(1.5)
        mods[1].bias_ih_l0.add_(0.25)
    _, b = _lstm_group(lib, B, S, G, mods=mods)
    for g in (0, 2):
        assert torch.equal(a[0][..., g * H:(g + 1) * H], b[0][..., g * H:(g + 1) * H])
    assert not torch.equal(a[0][..., H:2 * H], b[0][..., H:2 * H])


# ------------------------------------------------------------------ Elman RNN
def _rnn(lib, T, R, G, nl, time_major, use_h0=False, flags=0, seed=0, mods=None):
    mods = mods or _heads(torch.nn.RNN, G, nl, seed, batch_first=not time_major)
    params = _stack(mods, nl)
    g = torch.Generator().manual_seed(seed + 1)
    shape = (T, R) if time_major else (R, T)
    x = torch.randn(*shape, H, generator=g)
    dy = torch.randn(*shape, G * H, generator=g)
    h0 = 0.5 * torch.randn(nl, R, H, generator=g) if use_h0 else None
    flags |= TIME_MAJOR if time_major else 0
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_rnn_layout(T, R, G, nl, sizes) == 0
    saved, fscr, bscr = Guarded(sizes[0]), Guarded(sizes[1]), Guarded(sizes[2])
    y, dx = Guarded(*shape, G * H), Guarded(*shape, H)
    hN = Guarded(nl, R, H) if G == 1 else None
    grads = [Guarded(*p.shape) for p in params]
    parr = (ctypes.c_void_p * (4 * nl))(*[P(p) for p in params])
    garr = (ctypes.c_void_p * (4 * nl))(*[P(q.t) for q in grads])
    assert lib.cpc_rnn_forward(P(x), P(h0), parr, P(saved.t), P(fscr.t), P(y.t), None if hN is None else P(hN.t), T, R, G, nl,
                               flags, None) == 0
    assert lib.cpc_rnn_backward(P(x), P(h0), parr, P(saved.t), P(y.t), P(dy), P(bscr.t), P(dx.t), garr, T, R, G, nl, flags,
                                None) == 0
    for q in [saved, fscr, bscr, y, dx] + grads + ([hN] if hN is not None else []):
        assert q.intact()
    return (mods, x, dy, h0), (y.t, None if hN is None else hN.t, dx.t, [q.t for q in grads])


# the last two: 20 workgroups a head and 4 heads (split 3 + 1), and 68 workgroups for one head (per-step kernels)
RNN_TM_SHAPES = [(1, 1, 1), (2, 6, 3), (7, 20, 3), (3, 70, 2), (3, 70, 4), (2, 260, 1)]


@pytest.mark.parametrize("T,R,G", RNN_TM_SHAPES)
def test_rnn_time_major_matches_torch_float64_emulated(T, R, G):
    """The predictors' shape: G nn.RNN(256, 256) without batch_first on (T, R, 256), y (T, R, G*256)."""
    lib = emu()
    (mods, x, dy, _), outs = _rnn(lib, T, R, G, 1, True)
    assert not torch.isnan(outs[0]).any() and not torch.isnan(outs[2]).any()
    _check(outs, _oracle(mods, 1, x, dy), G == 1)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("use_h0", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("R,T", [(5, 7), (20, 33)])
def test_rnn_batch_first_matches_torch_float64_emulated(R, T, nl, use_h0):
    """The autoregressor's shape: nn.RNN(256, 256, nl, batch_first=True) with an optional carried h0; y, hN, dx and 4*nl gradients."""
    lib = emu()
    (mods, x, dy, h0), outs = _rnn(lib, T, R, 1, nl, False, use_h0)
    _check(outs, _oracle(mods, nl, x, dy, h0), True)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("T,R,G,nl,tm,use_h0", [(7, 20, 3, 1, True, False), (2, 6, 3, 1, True, False), (33, 20, 1, 2, False, True),
                                               (7, 5, 1, 2, True, True)])
def test_rnn_per_step_flag_gives_the_same_bits_emulated(T, R, G, nl, tm, use_h0):
    lib = emu()
    inputs, a = _rnn(lib, T, R, G, nl, tm, use_h0)
    _, b = _rnn(lib, T, R, G, nl, tm, use_h0, flags=PER_STEP)
    for u, v in zip([a[0], a[2]] + a[3], [b[0], b[2]] + b[3]):
        assert torch.equal(u, v)
    if G == 1:
        assert torch.equal(a[1], b[1])
    mods, x, dy, h0 = inputs
    _check(b, _oracle(mods, nl, x, dy, h0), G == 1)


def test_rnn_heads_are_independent_emulated():
    lib = emu()
    T, R, G = 2, 6, 3
    mods = _heads(torch.nn.RNN, G, 1, 0)
    _, a = _rnn(lib, T, R, G, 1, True, mods=mods)
    with torch.no_grad():
        mods[1].weight_hh_l0.mul_(1.5)
        mods[1].bias_ih_l0.add_(0.25)
    _, b = _rnn(lib, T, R, G, 1, True, mods=mods)
    for g in (0, 2):
        assert torch.equal(a[0][..., g * H:(g + 1) * H], b[0][..., g * H:(g + 1) * H])
    assert not torch.equal(a[0][..., H:2 * H], b[0][..., H:2 * H])
