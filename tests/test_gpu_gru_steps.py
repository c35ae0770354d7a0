"""The recurrence over the time steps the loss reads, on a real MI355X: the comparisons of tests/test_emu_gru_steps.py (the
two-layer GRU over the first T of S steps against the full recurrence on a zero-tailed dy; persistent kernels) at (B, S) = (24, 20),
T in {S, 8}, and of tests/test_emu_train_step_steps.py (cpc_train_step with the forward bit 32 against the step without it) at
B = 16 on four distinct streams.  No wave may have run out of its polling budget (ops.check_device_errors)."""
import ctypes

import pytest
import torch

from emu_util import P
from oracle import cpc_oracle as O
from test_emu_train_step import ENC, GRU, _composite, _setup

pytestmark = pytest.mark.gpu

B, S = 24, 20


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gru_case():
    """Parameters, inputs and the full-length forward: computed once, left unchanged."""
    dev = _dev()
    from cpc_audio_amd import _lib
    lib = _lib.get()
    with torch.cuda.device(dev):
        p = O.make_params(seed=3, n_levels_gru=2)
        names = [f"gAR.baseNet.{w}_l{l}" for l in range(2) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        plist = [p[n].contiguous().to(dev) for n in names]
        g = torch.Generator().manual_seed(B)
        x, dy = torch.randn(B, S, 256, generator=g).to(dev), torch.randn(B, S, 256, generator=g).to(dev)
        sizes = (ctypes.c_long * 3)()
        assert lib.cpc_gru_layout(B, S, 2, sizes) == 0
        case = dict(lib=lib, dev=dev, plist=plist, x=x, dy=dy, sizes=sizes, ncoef=lib.cpc_gru_coef_floats(B, S, 2),
                    parr=(ctypes.c_void_p * 8)(*[P(t) for t in plist]))
        case["full"] = _forward(case, None)
        torch.cuda.synchronize(dev)
        assert torch.isfinite(case["full"][1]).all()
    return case


def _forward(k, T):
    lib, dev, nan = k["lib"], k["dev"], float("nan")
    saved, fscr = torch.full((k["sizes"][0],), nan, device=dev), torch.full((k["sizes"][1],), nan, device=dev)
    coef = torch.full((k["ncoef"],), nan, device=dev)
    y, hN = torch.full((B, S, 256), nan, device=dev), torch.full((2, B, 256), nan, device=dev)
    if T is None:
        assert lib.cpc_gru_forward_coef(P(k["x"]), None, k["parr"], P(saved), P(fscr), P(y), P(hN), P(coef), B, S, 2, None) == 0
    else:
        assert lib.cpc_gru_forward_prepare_steps(P(fscr), P(saved), P(y), B, S, T, 2, None) == 0
        assert lib.cpc_gru_forward_coef_prepared_steps(P(k["x"]), None, k["parr"], P(saved), P(fscr), P(y), P(hN), P(coef), B, S, T, 2,
                                                       None) == 0
    torch.cuda.synchronize(dev)
    return saved, y, hN, coef, fscr


def _backward(k, T, state, dy):
    lib, dev, nan = k["lib"], k["dev"], float("nan")
    saved, y, _, coef = state[:4]
    bscr = torch.full((k["sizes"][2],), nan, device=dev)
    dx = torch.full((B, S, 256), nan, device=dev)
    grads = [torch.full_like(t, nan) for t in k["plist"]]
    garr = (ctypes.c_void_p * 8)(*[P(t) for t in grads])
    assert lib.cpc_gru_backward_coef(None, k["parr"], P(saved), P(y), P(coef), 1, B, S, 2, None) == 0
    if T is None:
        assert lib.cpc_gru_backward_streams(P(k["x"]), None, k["parr"], P(saved), P(y), P(dy), P(coef), P(bscr), P(dx), garr, B, S, 2,
                                            None, None) == 0
    else:
        assert lib.cpc_gru_backward_streams_steps(P(k["x"]), None, k["parr"], P(saved), P(y), P(dy), P(coef), P(bscr), P(dx), garr, B,
                                                  S, T, 2, None, None) == 0
    torch.cuda.synchronize(dev)
    return [dx] + grads


@pytest.mark.parametrize("T", [S, 8])
def test_active_steps_change_no_value(gru_case, T):
    k = gru_case
    from cpc_audio_amd import ops
    with torch.cuda.device(k["dev"]):
        full = k["full"]
        dy = k["dy"].clone()
        dy[:, T:] = 0
        ref = _backward(k, None, full, dy)
        assert all(torch.isfinite(t).all() for t in ref)
        got = _backward(k, T, full, dy)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (T, "backward", i)
        assert (got[0][:, T:] == 0).all()
        part = _forward(k, T)
        assert torch.equal(part[1][:, :T], full[1][:, :T])
        assert (part[1][:, T:] == 0).all()
        if T < S:
            assert torch.isnan(part[2]).all()
        else:
            assert torch.equal(part[2], full[2])
        got = _backward(k, T, part, dy)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.isfinite(b).all(), (T, "NaN", i)
            assert torch.equal(a, b), (T, "forward + backward", i)
        ops.check_device_errors()


def test_step_with_the_forward_bit_changes_only_what_nobody_reads():
    dev = _dev()
    from cpc_audio_amd import _lib, ops
    lib = _lib.get()
    Bs, L, K, N = 16, 2560, 12, 16
    W = 16 - K
    _, wave, Sx, bidx, sidx, plist = _setup(Bs, L, K, N)
    assert Sx == 16
    with torch.cuda.device(dev):
        pool = [torch.cuda.Stream(dev) for _ in range(4)]
        handles = tuple(s.cuda_stream for s in pool)
        assert len(set(handles)) == 4
        runs = []
        for phases in (3, 3 | 32):
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(pool[0]):
                runs.append(_composite(lib, wave, bidx, sidx, None, 1.0, plist, Bs, L, K, N, phases=(phases,), streams=handles,
                                       device=dev))
        ops.check_device_errors()
    (out, hN, grads, z, c), (out2, hN2, grads2, z2, c2) = runs
    assert torch.isfinite(out).all() and torch.isfinite(hN).all() and torch.isfinite(c).all()
    assert torch.equal(out, out2) and torch.equal(z, z2)
    assert torch.equal(c[:, :W], c2[:, :W])
    assert (c2[:, W:] == 0).all()
    assert torch.isnan(hN2).all()
    for n, a, b in zip(ENC + GRU + ["wall"], grads, grads2):
        assert torch.isfinite(b).all(), n
        assert torch.equal(a, b), n
