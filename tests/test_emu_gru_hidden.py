"""The GRU at any hidden width (csrc/gru.hip: cpc_gru_*_h) on the host SIMT emulator against torch.nn.GRU(D, H, nl) in
float64 on the CPU, with nn.GRU's own initialisation.

Every buffer the entries write -- saved, both scratch buffers, the outputs and the gradients -- starts out as NaN: padding read
before it is written, or an output left unwritten, shows as a NaN in a result.  Bars: max |d| < 1e-5 on y and hN, norm-wise
relative error < 1e-5 on dx and every parameter gradient (the project's emulator bars, tests/test_emu_lstm_hidden.py)."""
import ctypes

import pytest
import torch

from emu_util import P, emu, rel_err

PER_STEP = 1        # CPC_GRU_PER_STEP
ARG = 2             # CPC_ERR_ARG
WIDTHS = [(1, 1), (13, 13), (40, 40), (256, 64), (40, 130), (256, 272), (512, 512)]
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _params(D, H, nl, seed):
    """4*nl tensors in torch.nn.GRU state-dict order, with nn.GRU's own initialisation (U(-1/sqrt(H), 1/sqrt(H)))."""
    torch.manual_seed(seed)
    ref = torch.nn.GRU(D, H, num_layers=nl, batch_first=True)
    return [getattr(ref, f"{w}_l{l}").detach().clone().contiguous() for l in range(nl) for w in NAMES]


_oracles = {}


def _oracle(key, D, H, plist, x, h0, dy):
    """float64 nn.GRU on the CPU; computed once per case and left unchanged."""
    if key not in _oracles:
        nl = len(plist) // 4
        ref = torch.nn.GRU(D, H, num_layers=nl, batch_first=True).double()
        with torch.no_grad():
            for l in range(nl):
                for k, w in enumerate(NAMES):
                    getattr(ref, f"{w}_l{l}").copy_(plist[4 * l + k].double())
        xr = x.double().clone().requires_grad_(True)
        y, hN = ref(xr, None if h0 is None else h0.double())
        (y * dy.double()).sum().backward()
        grads = [getattr(ref, f"{w}_l{l}").grad for l in range(nl) for w in NAMES]
        _oracles[key] = (y.detach(), hN.detach(), xr.grad, grads)
    return _oracles[key]


def _inputs(D, H, B, S, nl, use_state, seed=0):
    plist = _params(D, H, nl, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, S, D, generator=g)
    h0 = 0.5 * torch.randn(nl, B, H, generator=g) if use_state else None
    dy = torch.randn(B, S, H, generator=g)
    return plist, x, h0, dy


def _run(lib, D, H, B, S, nl, use_state, flags=0, fill=float("nan"), entry="h"):
    """entry "h": cpc_gru_*_h; "in": cpc_gru_*_in (H == 256 only; it takes no flags)."""
    plist, x, h0, dy = _inputs(D, H, B, S, nl, use_state)
    sizes = (ctypes.c_long * 3)()
    dims = (B, S, nl, D, H, flags) if entry == "h" else (B, S, nl, D)
    layout, fwd, bwd = (getattr(lib, f"cpc_gru_{k}_{entry}") for k in ("layout", "forward", "backward"))
    assert layout(*dims[:5], sizes) == 0
    saved = torch.full((sizes[0],), fill)
    fscr = torch.full((sizes[1],), fill)
    y = torch.full((B, S, H), float("nan"))
    hN = torch.full((nl, B, H), float("nan"))
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    assert fwd(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), *dims, None) == 0
    bscr = torch.full((sizes[2],), fill)
    dx = torch.full((B, S, D), float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in plist]
    garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
    assert bwd(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, *dims, None) == 0
    assert lib.cpc_device_error_flags(1) == 0
    return (plist, x, h0, dy), [y, hN, dx] + grads, list(sizes)


def _check(key, D, H, inputs, outs):
    plist, x, h0, dy = inputs
    yr, hr, dxr, gr = _oracle(key, D, H, plist, x, h0, dy)
    y, hN, dx, *grads = outs
    assert (y.double() - yr).abs().max().item() < 1e-5
    assert (hN.double() - hr).abs().max().item() < 1e-5
    assert rel_err(dx.double(), dxr) < 1e-5
    bad = {k: rel_err(g.double(), r) for k, (g, r) in enumerate(zip(grads, gr)) if not rel_err(g.double(), r) < 1e-5}
    assert not bad, bad


@pytest.mark.parametrize("use_state", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("B", [1, 5, 20])
@pytest.mark.parametrize("D,H", WIDTHS)
def test_gru_hidden_forward_backward_match_torch_float64_emulated(D, H, B, S, nl, use_state):
    """y, hN, dx and all 4*nl parameter gradients of the persistent path against nn.GRU(D, H, nl) in float64: H below one unit
    tile, H % 4 != 0, one unit past a 128 boundary, the first tile past 256, the widest; B = 20 is a full batch tile plus a
    ragged one; nl = 2 has a layer whose input width is H."""
    lib = emu()
    inputs, outs, _ = _run(lib, D, H, B, S, nl, use_state)
    _check((D, H, B, S, nl, use_state), D, H, inputs, outs)


@pytest.mark.parametrize("use_state", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("B", [1, 5, 20])
@pytest.mark.parametrize("D,H", [(13, 13), (40, 130)])
def test_gru_hidden_long_sequence_matches_torch_float64_emulated(D, H, B, nl, use_state):
    """S = 33 at the two narrow widths."""
    lib = emu()
    inputs, outs, _ = _run(lib, D, H, B, 33, nl, use_state)
    _check((D, H, B, 33, nl, use_state), D, H, inputs, outs)


@pytest.mark.parametrize("D,H", [(13, 13), (40, 130), (512, 512)])
def test_gru_hidden_persistent_and_per_step_agree_bit_for_bit_emulated(D, H):
    """Same MFMAs in the same order: every output and gradient of CPC_GRU_PER_STEP equals the persistent path's bit for bit."""
    lib = emu()
    B, S, nl = 20, 9, 2
    lib.cpc_gru_paths_h(1)
    inputs, a, _ = _run(lib, D, H, B, S, nl, True, flags=0)
    assert lib.cpc_gru_paths_h(1) == 1
    _, b, _ = _run(lib, D, H, B, S, nl, True, flags=PER_STEP)
    assert lib.cpc_gru_paths_h(1) == 2
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
    _check((D, H, B, S, nl, True), D, H, inputs, b)


@pytest.mark.parametrize("D", [40, 256])
def test_hidden_256_is_the_input_width_entry_emulated(D):
    """H == 256: cpc_gru_layout_h reports cpc_gru_layout_in's sizes and forward / backward give cpc_gru_*_in's bits (nl = 2 with
    D = 256 is the two-layer 256 path); CPC_GRU_PER_STEP is refused there, before any launch."""
    lib = emu()
    B, S, nl = 5, 7, 2
    _, a, sa = _run(lib, D, 256, B, S, nl, True, entry="h")
    _, b, sb = _run(lib, D, 256, B, S, nl, True, entry="in")
    assert sa == sb
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
    plist, x, h0, dy = _inputs(D, 256, B, S, nl, True)
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    saved, fscr, bscr = (torch.full((n,), 7.0) for n in sa)
    y, hN, dx = torch.full((B, S, 256), 7.0), torch.full((nl, B, 256), 7.0), torch.full((B, S, D), 7.0)
    grads = [torch.full_like(t, 7.0) for t in plist]
    garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
    assert lib.cpc_gru_forward_h(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), B, S, nl, D, 256, PER_STEP, None) == ARG
    assert lib.cpc_gru_backward_h(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, D, 256, PER_STEP,
                                  None) == ARG
    for t in [saved, fscr, bscr, y, hN, dx] + grads:
        assert bool((t == 7.0).all())


@pytest.mark.parametrize("use_state", [False, True])
def test_zero_padding_is_exact_emulated(use_state):
    """(40, 130) pads 130 units to 256.  The results do not depend on what the saved and scratch buffers held before the call:
    NaN or 1e30, y, hN, dx and the gradients are the same bits, all finite (a padded unit contributes exactly 0).  The run with a
    carried h0 is the GRU's own trap: a padded unit computes h' = h_prev / 2, so it is zero only because the padded h0 is
    written as zeros -- left as scratch it would decay through y as 2^-t and 1e30 would reach the real units' gradients."""
    lib = emu()
    _, a, _ = _run(lib, 40, 130, 5, 7, 2, use_state, fill=float("nan"))
    _, b, _ = _run(lib, 40, 130, 5, 7, 2, use_state, fill=1e30)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
        assert bool(torch.isfinite(u).all()), k
