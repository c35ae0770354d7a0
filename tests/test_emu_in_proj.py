"""The width-generic input projection (csrc/in_proj.hip) and the cells' cpc_*_in entries on the host SIMT emulator, against
float64 matmuls and torch.nn.GRU / nn.LSTM / nn.RNN in float64 on the CPU.  Bars as tests/test_emu_lstm.py: max |delta| < 1e-5 on
y, hN, cN; norm-wise relative error < 1e-5 on dx and every parameter gradient."""
import ctypes

import pytest
import torch

from cpc_audio_amd import _lib as _L
from emu_util import P, emu, rel_err

H = 256
NAN = float("nan")
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


# ---------------------------------------------------------------------------------------------- the projection alone
def _proj(lib, M, N, D, scale=1.0, pitch=None, seed=0, guard=64):
    """Runs forward and backward on NaN-filled outputs; x and dx rows `pitch` floats apart, dx with `guard` floats behind its last
    row.  -> inputs, (out, dx buffer, dw)."""
    pitch = D if pitch is None else pitch
    g = torch.Generator().manual_seed(seed + 1000 * D + M)
    xbuf = torch.full((M * pitch,), NAN)
    x = xbuf.view(M, pitch)[:, :D]
    x.copy_(scale * torch.randn(M, D, generator=g))
    w = torch.randn(N, D, generator=g) / 16
    bias = torch.randn(N, generator=g)
    dg = torch.randn(M, N, generator=g)
    n = lib.cpc_in_proj_scratch_floats(M, N, D)
    assert n > 0
    scratch = torch.full((n,), NAN)
    out = torch.full((M, N), NAN)
    assert lib.cpc_in_proj_forward(P(xbuf), pitch, P(w), P(bias), P(scratch), P(out), M, N, D, None) == 0
    scratch.fill_(NAN)
    dxbuf = torch.full((M * pitch + guard,), NAN)
    dw = torch.full((N, D), NAN)
    assert lib.cpc_in_proj_backward(P(xbuf), pitch, P(w), P(dg), P(scratch), P(dxbuf), P(dw), M, N, D, None) == 0
    return (x, w, bias, dg), (out, dxbuf, dw)


def _check_proj(inputs, outs, M, D, pitch, guard=64):
    x, w, bias, dg = (t.double() for t in inputs)
    out, dxbuf, dw = outs
    assert rel_err(out.double(), x @ w.t() + bias) < 1e-5
    body = dxbuf[:M * pitch].view(M, pitch)
    assert rel_err(body[:, :D].double(), dg @ w) < 1e-5
    assert rel_err(dw.double(), dg.t() @ x) < 1e-5
    # nothing behind the D columns of a row, nothing behind the last row
    assert bool(torch.isnan(body[:, D:]).all()) and bool(torch.isnan(dxbuf[M * pitch:]).all())
    assert dxbuf[M * pitch:].numel() == guard


@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("D", [1, 13, 40, 64, 255, 257, 512])
def test_projection_matches_float64_at_every_width_emulated(D, N):
    """Forward, dx and dW for partial row tiles (M = 1, 15, 35: inside one tile of every kernel; 130: one row past a 32-row tile
    and two past a 64-row one), widths off and on the aligned path, every output pre-filled with NaN."""
    lib = emu()
    for M in (1, 15, 35, 130):
        inputs, outs = _proj(lib, M, N, D)
        _check_proj(inputs, outs, M, D, D)


@pytest.mark.parametrize("D,pitch", [(13, 16), (13, 17), (40, 44), (40, 43), (255, 259)])
def test_projection_leaves_the_guard_band_untouched_emulated(D, pitch):
    """x and dx with rows `pitch` > D floats apart: the columns behind D and the floats behind the last row keep their NaN fill
    (pitch % 4 == 0 with D % 4 == 0 is the 16-byte path, everything else the 4-byte one)."""
    lib = emu()
    for M in (35, 130):
        inputs, outs = _proj(lib, M, 256, D, pitch=pitch)
        _check_proj(inputs, outs, M, D, pitch)


def test_projection_takes_large_inputs_emulated():
    """x scaled by 100 (MFCC coefficients reach the hundreds): exact-f32 products, so the relative error does not move."""
    lib = emu()
    inputs, outs = _proj(lib, 130, 768, 40, scale=100.0)
    _check_proj(inputs, outs, 130, 40, 40)
    assert inputs[0].abs().max().item() > 200


@pytest.mark.parametrize("M,D", [(130, 13), (700, 40)])
def test_weight_gradient_is_bit_identical_between_runs_emulated(M, D):
    """dW is a fixed-order sum over the row splits (700 rows: three splits): two runs give the same bits."""
    lib = emu()
    _, a = _proj(lib, M, 256, D)
    _, b = _proj(lib, M, 256, D)
    assert torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_either_backward_product_may_be_left_out_emulated():
    lib = emu()
    M, N, D = 35, 256, 13
    (x, w, _, dg), (_, dxbuf, dw) = _proj(lib, M, N, D, guard=0)
    x = x.contiguous()
    scratch = torch.full((lib.cpc_in_proj_scratch_floats(M, N, D),), NAN)
    dx1, dw1 = torch.full((M, D), NAN), torch.full((N, D), NAN)
    assert lib.cpc_in_proj_backward(P(x), D, P(w), P(dg), P(scratch), P(dx1), None, M, N, D, None) == 0
    assert lib.cpc_in_proj_backward(P(x), D, P(w), P(dg), P(scratch), None, P(dw1), M, N, D, None) == 0
    assert torch.equal(dx1, dxbuf.view(M, D)) and torch.equal(dw1, dw)


def test_projection_errors_are_returned_before_any_launch_emulated():
    lib = emu()
    M, N, D = 5, 256, 40
    assert lib.cpc_in_proj_scratch_floats(M, N, 0) == 0 and lib.cpc_in_proj_scratch_floats(M, N, 513) == 0
    assert lib.cpc_in_proj_scratch_floats(M, 200, D) == 0 and lib.cpc_in_proj_scratch_floats(0, N, D) == 0
    x, w, bias, dg = torch.randn(M, D), torch.randn(N, D), torch.randn(N), torch.randn(M, N)
    scratch = torch.full((lib.cpc_in_proj_scratch_floats(M, N, D),), 7.0)
    out, dx, dw = torch.full((M, N), 7.0), torch.full((M, D), 7.0), torch.full((N, D), 7.0)

    def fwd(**kw):
        a = dict(x=P(x), ldx=D, w=P(w), bias=P(bias), scratch=P(scratch), out=P(out), M=M, N=N, D=D)
        a.update(kw)
        return lib.cpc_in_proj_forward(*a.values(), None)

    def bwd(**kw):
        a = dict(x=P(x), ldx=D, w=P(w), dg=P(dg), scratch=P(scratch), dx=P(dx), dw=P(dw), M=M, N=N, D=D)
        a.update(kw)
        return lib.cpc_in_proj_backward(*a.values(), None)

    for call in (fwd, bwd):
        assert call(D=0) == 1 and call(D=513) == 1 and call(M=0) == 1 and call(N=200) == 1 and call(ldx=D - 1) == 1
        assert call(x=None) == 2 and call(w=None) == 2 and call(scratch=None) == 2
        assert call(scratch=P(scratch) + 4) == 2                    # not 16-byte aligned
    assert fwd(out=None) == 2 and fwd(out=P(out) + 8) == 2
    assert bwd(dg=None) == 2 and bwd(dx=None, dw=None) == 2 and bwd(dg=P(dg) + 4) == 2      # (dx or dw alone may be NULL)
    for t in (scratch, out, dx, dw):
        assert bool((t == 7.0).all())


# ---------------------------------------------------------------------------------------------- the cells
CELLS = {"gru": (torch.nn.GRU, 3), "lstm": (torch.nn.LSTM, 4), "rnn": (torch.nn.RNN, 1)}


def _params(cell, D, nl, seed):
    torch.manual_seed(seed)
    ref = CELLS[cell][0](D, H, num_layers=nl, batch_first=True)
    return [getattr(ref, f"{w}_l{l}").detach().clone().contiguous() for l in range(nl) for w in NAMES]


def _oracle(cell, plist, x, state, dy):
    nl = len(plist) // 4
    ref = CELLS[cell][0](x.shape[2], H, num_layers=nl, batch_first=True).double()
    with torch.no_grad():
        for l in range(nl):
            for k, w in enumerate(NAMES):
                getattr(ref, f"{w}_l{l}").copy_(plist[4 * l + k].double())
    xr = x.double().clone().requires_grad_(True)
    st = None if state is None else (tuple(t.double() for t in state) if cell == "lstm" else state[0].double())
    y, hN = ref(xr, st)
    (y * dy.double()).sum().backward()
    grads = [getattr(ref, f"{w}_l{l}").grad for l in range(nl) for w in NAMES]
    finals = [t.detach() for t in hN] if cell == "lstm" else [hN.detach()]
    return [y.detach()] + finals, xr.grad, grads


def _run(lib, cell, B, S, nl, D, use_state, per_step=False, old_entries=False, seed=0, gru_mode=None):
    """One forward + backward through cpc_<cell>_forward_in / _backward_in (old_entries: the plain 256-wide entries) on NaN-filled
    buffers -> inputs, [y, hN(, cN), dx, 4 nl gradients].  gru_mode: the persistent GRU's cpc_set_gru_mode (default: the library's)."""
    plist = _params(cell, D, nl, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, S, D, generator=g)
    state = None
    if use_state:
        state = (0.5 * torch.randn(nl, B, H, generator=g), torch.randn(nl, B, H, generator=g))
    dy = torch.randn(B, S, H, generator=g)
    h0, c0 = (None, None) if state is None else state
    sizes = (ctypes.c_long * 3)()
    if old_entries:
        assert D == H
        lay = {"gru": lambda: lib.cpc_gru_layout(B, S, nl, sizes), "lstm": lambda: lib.cpc_lstm_layout(B, S, nl, sizes),
               "rnn": lambda: lib.cpc_rnn_layout(S, B, 1, nl, sizes)}[cell]
    else:
        lay = {"gru": lambda: lib.cpc_gru_layout_in(B, S, nl, D, sizes), "lstm": lambda: lib.cpc_lstm_layout_in(B, S, nl, D, sizes),
               "rnn": lambda: lib.cpc_rnn_layout_in(S, B, nl, D, sizes)}[cell]
    assert lay() == 0
    saved, fscr, bscr = (torch.full((sizes[k],), NAN) for k in range(3))
    y = torch.full((B, S, H), NAN)
    hN, cN = torch.full((nl, B, H), NAN), torch.full((nl, B, H), NAN)
    dx = torch.full((B, S, D), NAN)
    grads = [torch.full_like(t, NAN) for t in plist]
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
    flags = 1 if per_step else 0                     # CPC_LSTM_PER_STEP / CPC_RNN_PER_STEP
    if cell == "gru":
        assert lib.cpc_set_gru_mode(0 if per_step else (_L.DEFAULT_GRU_MODE if gru_mode is None else gru_mode)) == 0
        try:
            if old_entries:
                assert lib.cpc_gru_forward(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), B, S, nl, None) == 0
                assert lib.cpc_gru_backward(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, None) == 0
            else:
                assert lib.cpc_gru_forward_in(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), B, S, nl, D, None) == 0
                assert lib.cpc_gru_backward_in(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, D,
                                               None) == 0
        finally:
            lib.cpc_set_gru_mode(_L.DEFAULT_GRU_MODE)
        outs = [y, hN]
    elif cell == "lstm":
        if old_entries:
            assert lib.cpc_lstm_forward(P(x), P(h0), P(c0), parr, P(saved), P(fscr), P(y), P(hN), P(cN), B, S, nl, flags, None) == 0
            assert lib.cpc_lstm_backward(P(x), P(h0), P(c0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, flags,
                                         None) == 0
        else:
            assert lib.cpc_lstm_forward_in(P(x), P(h0), P(c0), parr, P(saved), P(fscr), P(y), P(hN), P(cN), B, S, nl, D, flags,
                                           None) == 0
            assert lib.cpc_lstm_backward_in(P(x), P(h0), P(c0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, B, S, nl, D,
                                            flags, None) == 0
        outs = [y, hN, cN]
    else:
        if old_entries:
            assert lib.cpc_rnn_forward(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), S, B, 1, nl, flags, None) == 0
            assert lib.cpc_rnn_backward(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, S, B, 1, nl, flags,
                                        None) == 0
        else:
            assert lib.cpc_rnn_forward_in(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), S, B, nl, D, flags, None) == 0
            assert lib.cpc_rnn_backward_in(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, S, B, nl, D, flags,
                                           None) == 0
        outs = [y, hN]
    return (plist, x, state, dy), outs + [dx] + grads


def _check(cell, inputs, outs):
    plist, x, state, dy = inputs
    ref_outs, dxr, gr = _oracle(cell, plist, x, state, dy)
    n = len(ref_outs)
    for k in range(n):
        assert (outs[k].double() - ref_outs[k]).abs().max().item() < 1e-5, k
    assert rel_err(outs[n].double(), dxr) < 1e-5
    bad = {k: rel_err(g.double(), r) for k, (g, r) in enumerate(zip(outs[n + 1:], gr)) if not rel_err(g.double(), r) < 1e-5}
    assert not bad, bad


@pytest.mark.parametrize("use_state", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("B,S", [(1, 1), (5, 7), (20, 9)])
@pytest.mark.parametrize("D", [13, 40, 512])
@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_cells_match_torch_float64_at_other_input_widths_emulated(cell, D, B, S, nl, use_state):
    """Every output, dx (B,S,D) and all 4 nl parameter gradients -- weight_ih_l0 is (3|4|1 x 256, D) -- against float64."""
    lib = emu()
    inputs, outs = _run(lib, cell, B, S, nl, D, use_state)
    _check(cell, inputs, outs)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("cell,B,S,nl,D,use_state", [("gru", 5, 7, 2, 40, False), ("gru", 20, 9, 2, 13, True), ("gru", 3, 4, 3, 40, True),
                                                     ("lstm", 5, 7, 1, 40, False), ("lstm", 20, 9, 2, 512, True),
                                                     ("rnn", 5, 7, 1, 13, True), ("rnn", 20, 9, 2, 40, False)])
def test_persistent_and_per_step_paths_agree_bit_for_bit_emulated(cell, B, S, nl, D, use_state):
    """The persistent recurrence and the one-launch-per-step kernels behind the same projection: every output and gradient is
    bit-identical (GRU: cpc_set_gru_mode(0) against mode 1, the persistent recurrence on exact-f32 products -- the default mode 2
    runs the forward's recurrent products on fp16 pieces when no state is carried, which cannot give the same bits)."""
    lib = emu()
    inputs, a = _run(lib, cell, B, S, nl, D, use_state, gru_mode=1)
    _, b = _run(lib, cell, B, S, nl, D, use_state, per_step=True)
    _check(cell, inputs, b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k


@pytest.mark.parametrize("T,R,nl,D,use_h0,per_step", [(7, 5, 1, 13, False, False), (9, 20, 2, 40, True, False), (4, 3, 1, 512, True, True)])
def test_rnn_in_entries_take_the_time_major_layout_emulated(T, R, nl, D, use_h0, per_step):
    """CPC_RNN_TIME_MAJOR through cpc_rnn_forward_in / _backward_in: x, dx (T,R,D), y, dy (T,R,256) -- the projection works row by
    row, so the flag means what it means at 256 -- against nn.RNN without batch_first in float64."""
    lib = emu()
    plist = _params("rnn", D, nl, 2)
    g = torch.Generator().manual_seed(T + D)
    x, dy = torch.randn(T, R, D, generator=g), torch.randn(T, R, H, generator=g)
    h0 = 0.5 * torch.randn(nl, R, H, generator=g) if use_h0 else None
    flags = 2 | (1 if per_step else 0)
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_rnn_layout_in(T, R, nl, D, sizes) == 0
    saved, fscr, bscr = (torch.full((sizes[k],), NAN) for k in range(3))
    y, hN, dx = torch.full((T, R, H), NAN), torch.full((nl, R, H), NAN), torch.full((T, R, D), NAN)
    grads = [torch.full_like(t, NAN) for t in plist]
    parr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in plist])
    garr = (ctypes.c_void_p * (4 * nl))(*[P(t) for t in grads])
    assert lib.cpc_rnn_forward_in(P(x), P(h0), parr, P(saved), P(fscr), P(y), P(hN), T, R, nl, D, flags, None) == 0
    assert lib.cpc_rnn_backward_in(P(x), P(h0), parr, P(saved), P(y), P(dy), P(bscr), P(dx), garr, T, R, nl, D, flags, None) == 0
    # the batch-first oracle on the transposed problem
    state = None if h0 is None else (h0, h0)
    ref, dxr, gr = _oracle("rnn", plist, x.transpose(0, 1).contiguous(), state, dy.transpose(0, 1).contiguous())
    assert (y.double() - ref[0].transpose(0, 1)).abs().max().item() < 1e-5
    assert (hN.double() - ref[1]).abs().max().item() < 1e-5
    assert rel_err(dx.double(), dxr.transpose(0, 1)) < 1e-5
    bad = {k: rel_err(a.double(), r) for k, (a, r) in enumerate(zip(grads, gr)) if not rel_err(a.double(), r) < 1e-5}
    assert not bad, bad
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("cell,B,S,nl,use_state", [("gru", 5, 7, 2, False), ("gru", 3, 4, 1, True), ("gru", 20, 3, 2, True),
                                                   ("lstm", 5, 7, 1, False), ("lstm", 20, 3, 2, True),
                                                   ("rnn", 5, 7, 1, True), ("rnn", 20, 3, 2, False)])
def test_width_256_through_the_in_entries_is_the_old_path_bit_for_bit_emulated(cell, B, S, nl, use_state, per_step):
    lib = emu()
    _, a = _run(lib, cell, B, S, nl, H, use_state, per_step=per_step)
    _, b = _run(lib, cell, B, S, nl, H, use_state, per_step=per_step, old_entries=True)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
    sizes, old = (ctypes.c_long * 3)(), (ctypes.c_long * 3)()
    assert lib.cpc_gru_layout_in(B, S, nl, H, sizes) == 0 and lib.cpc_gru_layout(B, S, nl, old) == 0 and tuple(sizes) == tuple(old)
    assert lib.cpc_lstm_layout_in(B, S, nl, H, sizes) == 0 and lib.cpc_lstm_layout(B, S, nl, old) == 0 and tuple(sizes) == tuple(old)
    assert lib.cpc_rnn_layout_in(S, B, nl, H, sizes) == 0 and lib.cpc_rnn_layout(S, B, 1, nl, old) == 0 and tuple(sizes) == tuple(old)


@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_cell_errors_are_returned_before_any_launch_emulated(cell):
    lib = emu()
    B, S, nl, D = 3, 4, 1, 40
    sizes = (ctypes.c_long * 3)()
    lay = {"gru": lib.cpc_gru_layout_in, "lstm": lib.cpc_lstm_layout_in,
           "rnn": lambda b, s, n, d, out: lib.cpc_rnn_layout_in(s, b, n, d, out)}[cell]
    assert lay(B, S, nl, 0, sizes) == 1 and lay(B, S, nl, 513, sizes) == 1 and lay(B, S, nl, -3, sizes) == 1     # CPC_ERR_SHAPE
    assert lay(0, S, nl, D, sizes) == 1 and lay(B, S, 9, D, sizes) == 1
    assert lay(B, S, nl, D, None) == 2                                                                          # CPC_ERR_ARG
    assert lay(B, S, nl, D, sizes) == 0
    plist = _params(cell, D, nl, 0)
    parr = (ctypes.c_void_p * 4)(*[P(t) for t in plist])
    x = torch.randn(B, S, D)
    saved, fscr, bscr = (torch.full((sizes[k],), 7.0) for k in range(3))
    y = torch.full((B, S, H), 7.0)
    hN, cN = torch.full((nl, B, H), 7.0), torch.full((nl, B, H), 7.0)
    dx = torch.full((B, S, D), 7.0)
    grads = [torch.full_like(t, 7.0) for t in plist]
    garr = (ctypes.c_void_p * 4)(*[P(t) for t in grads])

    def fwd(**kw):
        a = dict(x=P(x), params=parr, saved=P(saved), scratch=P(fscr), y=P(y), hN=P(hN), cN=P(cN), D=D)
        a.update(kw)
        if cell == "gru":
            return lib.cpc_gru_forward_in(a["x"], None, a["params"], a["saved"], a["scratch"], a["y"], a["hN"], B, S, nl, a["D"], None)
        if cell == "lstm":
            return lib.cpc_lstm_forward_in(a["x"], None, None, a["params"], a["saved"], a["scratch"], a["y"], a["hN"], a["cN"], B, S,
                                           nl, a["D"], 0, None)
        return lib.cpc_rnn_forward_in(a["x"], None, a["params"], a["saved"], a["scratch"], a["y"], a["hN"], S, B, nl, a["D"], 0, None)

    def bwd(**kw):
        a = dict(x=P(x), params=parr, saved=P(saved), y=P(y), dy=P(y), scratch=P(bscr), dx=P(dx), grads=garr, D=D)
        a.update(kw)
        if cell == "gru":
            return lib.cpc_gru_backward_in(a["x"], None, a["params"], a["saved"], a["y"], a["dy"], a["scratch"], a["dx"], a["grads"],
                                           B, S, nl, a["D"], None)
        if cell == "lstm":
            return lib.cpc_lstm_backward_in(a["x"], None, None, a["params"], a["saved"], a["y"], a["dy"], a["scratch"], a["dx"],
                                            a["grads"], B, S, nl, a["D"], 0, None)
        return lib.cpc_rnn_backward_in(a["x"], None, a["params"], a["saved"], a["y"], a["dy"], a["scratch"], a["dx"], a["grads"],
                                       S, B, nl, a["D"], 0, None)

    for call in (fwd, bwd):
        assert call(D=0) == 1 and call(D=513) == 1
        assert call(x=None) == 2 and call(params=None) == 2 and call(saved=None) == 2 and call(scratch=None) == 2
    assert fwd(y=None) == 2
    assert bwd(dy=None) == 2 and bwd(dx=None) == 2 and bwd(grads=None) == 2
    for t in [saved, fscr, bscr, y, hN, cN, dx] + grads:
        assert bool((t == 7.0).all())
