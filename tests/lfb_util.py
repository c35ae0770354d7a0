"""Shared by the learned-filter-bank tests: seeded cases, the float64 CPU oracle (the reference's formula, cpc/model.py:125-152,
in torch ops with autograd for the gradients) and the calls through the C ABI -- on host tensors for the emulator library, on
device tensors for the product library."""
import ctypes
import json
import os

import numpy as np
import torch
import torch.nn.functional as Fnn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAPS, HOP, PAD = 400, 160, 350
CANARY = 64
FILL = 7.0

# (N, L) at D = 32: one conv position; the frame-count steps 2 -> 3 (418 / 419) and 3 -> 4 (578 / 579); frames whose window hangs
# over both ends; several 32-position tiles and hops with a ragged last one
ENERGY_CASES_D32 = [(2, 400), (3, 418), (3, 419), (1, 578), (2, 579), (3, 1040), (2, 2000)]
INPUT_VARIANTS = ["small", "loud", "dc", "bigw"]
LOGNORM_CASES = [(3, 2, 32), (2, 3, 32), (2, 12, 32), (1, 128, 256)]


def P(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    return ((a.double().cpu() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def frames(L):
    return (L - 99) // HOP + 1


def energy_case(N, L, D, seed, variant=None):
    """x (N, L), W (2D, 400), b (2D), han (400), gs (N, F, D), all fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(N, L, generator=g)).clamp_(-1, 1)
    bound = 1.0 / TAPS ** 0.5                                  # nn.Conv1d's default initialisation range
    W = (torch.rand(2 * D, TAPS, generator=g) * 2 - 1) * bound
    b = (torch.rand(2 * D, generator=g) * 2 - 1) * bound
    gs = torch.randn(N, frames(L), D, generator=g)
    if variant == "small":
        x = x * 1e-3
    elif variant == "loud":
        x = x * (30.0 / x.abs().max())
    elif variant == "dc":
        x = x + 0.5
    elif variant == "bigw":
        W = W * 100
    return x, W, b, torch.hann_window(TAPS), gs


def energy_oracle(x, W, b, han, gs=None):
    """float64: s (N, F, D) and, with gs, dW and db.  The conv is a matrix product over the unfolded waveform (what a BLAS does
    with 16 threads in a second where a float64 conv1d takes ten at (2, 20480, 256))."""
    Wd = W.double().clone().requires_grad_(gs is not None)
    bd = b.double().clone().requires_grad_(gs is not None)
    D = W.shape[0] // 2
    N = x.shape[0]
    ss = []
    for n in range(N):                                            # window by window: the unfolded copy is 64 MB at L = 20480
        y = Wd @ x[n].double().unfold(0, TAPS, 1).t() + bd[:, None]
        e = (y * y).view(D, 2, -1).sum(1)
        ss.append(Fnn.conv1d(e[:, None, :], han.double().view(1, 1, TAPS), stride=HOP, padding=PAD)[:, 0, :].t())
    s = torch.stack(ss)
    out = {"s": s.detach()}
    if gs is not None:
        (s * gs.double()).sum().backward()
        out.update(dW=Wd.grad, db=bd.grad)
    return out


def lognorm_case(N, F, D, seed, offset=False):
    """s >= 0 (N, F, D) and dy; offset: log(1 + s) has a mean 30 times its spread over the frames."""
    g = torch.Generator().manual_seed(seed)
    if offset:
        z = torch.randn(N, F, D, generator=g, dtype=torch.float64)           # every (n, d): spread exactly 0.2 around 6
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
        s = torch.expm1(6.0 + 0.2 * z)
    else:
        s = torch.rand(N, F, D, generator=g) * torch.exp(3 * torch.randn(N, 1, D, generator=g))
    return s.float(), torch.randn(N, F, D, generator=g)


def lognorm_oracle(s, dy=None, normalise=True):
    sd = s.double().clone().requires_grad_(dy is not None)
    u = torch.log(1 + sd.abs())
    out = {}
    if normalise:
        m = u.mean(1, keepdim=True)
        v = u.var(1, unbiased=False, keepdim=True)
        y = (u - m) / torch.sqrt(v + 1e-5)
        out.update(m=m.detach()[:, 0], r=(1 / torch.sqrt(v + 1e-5)).detach()[:, 0])
    else:
        y = u
    out["y"] = y.detach()
    if dy is not None:
        (y * dy.double()).sum().backward()
        out["ds"] = sd.grad
    return out


def layout(lib, N, L, D):
    sizes = (ctypes.c_long * 3)()
    rc = lib.cpc_lfb_layout(N, L, D, sizes)
    return rc, list(sizes)


def _out(n, device, canary=CANARY):
    return torch.full((n + canary,), FILL, device=device)


def tail_ok(buf, n):
    tail = buf[n:]
    return tail.numel() == CANARY and bool((tail == FILL).all())


def run_energy_forward(lib, x, W, b, han, stream=None):
    """-> s flat with CANARY spare floats (view the first N F D as (N, F, D))."""
    N, L = x.shape
    D = W.shape[0] // 2
    rc, (F, fwd_bytes, _) = layout(lib, N, L, D)
    assert rc == 0
    s = _out(N * F * D, x.device)
    ws = _out(fwd_bytes // 4, x.device)
    assert lib.cpc_lfb_energy_forward(P(x), P(W), P(b), P(han), P(s), P(ws), N, L, D, stream) == 0
    assert tail_ok(ws, fwd_bytes // 4)
    return s


def run_energy_backward(lib, x, W, b, han, gs, stream=None):
    """-> (dW, db) flat with CANARY spare floats each; the workspace's canary is checked here."""
    N, L = x.shape
    D = W.shape[0] // 2
    rc, (F, _, bwd_bytes) = layout(lib, N, L, D)
    assert rc == 0 and tuple(gs.shape) == (N, F, D)
    dW, db = _out(2 * D * TAPS, x.device), _out(2 * D, x.device)
    ws = _out(bwd_bytes // 4, x.device)
    assert lib.cpc_lfb_energy_backward(P(x), P(W), P(b), P(han), P(gs), P(dW), P(db), P(ws), N, L, D, stream) == 0
    assert tail_ok(ws, bwd_bytes // 4)
    return dW, db


def run_lognorm_forward(lib, s, normalise=True, want_stats=True, stream=None):
    N, F, D = s.shape
    y = _out(N * F * D, s.device)
    stats = _out(N * 2 * D, s.device) if want_stats else None
    assert lib.cpc_lfb_lognorm_forward(P(s), P(y), P(stats), N, F, D, int(normalise), stream) == 0
    return y, stats


def run_lognorm_backward(lib, s, stats, dy, normalise=True, stream=None):
    N, F, D = s.shape
    ds = _out(N * F * D, s.device)
    assert lib.cpc_lfb_lognorm_backward(P(s), P(stats), P(dy), P(ds), N, F, D, int(normalise), stream) == 0
    return ds


def check_energy(lib, case, device="cpu", stream=None, report=""):
    """Forward and backward of one case against float64 at the project's bars (1e-5 / 1e-4 norm-relative), with the canaries, the
    inputs' bits and run-to-run identity."""
    ref = energy_oracle(*case)
    x, W, b, han, gs = (t.to(device).contiguous() for t in case)
    keep = [t.clone() for t in (x, W, b, han, gs)]
    N, L = x.shape
    D = W.shape[0] // 2
    F = frames(L)
    s = run_energy_forward(lib, x, W, b, han, stream)
    dW, db = run_energy_backward(lib, x, W, b, han, gs, stream)
    s2 = run_energy_forward(lib, x, W, b, han, stream)
    dW2, db2 = run_energy_backward(lib, x, W, b, han, gs, stream)
    if device != "cpu":
        torch.cuda.synchronize()
    errs = (rel_err(s[:N * F * D].view(N, F, D), ref["s"]), rel_err(dW[:2 * D * TAPS].view(2 * D, TAPS), ref["dW"]),
            rel_err(db[:2 * D], ref["db"]))
    print(f"{report} N={N} L={L} D={D}: s {errs[0]:.3g} dW {errs[1]:.3g} db {errs[2]:.3g}")
    assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4, errs
    assert tail_ok(s, N * F * D) and tail_ok(dW, 2 * D * TAPS) and tail_ok(db, 2 * D)
    assert torch.equal(s, s2) and torch.equal(dW, dW2) and torch.equal(db, db2)
    assert all(torch.equal(a, k) for a, k in zip((x, W, b, han, gs), keep))


def check_lognorm(lib, N, F, D, normalise, offset, device="cpu", stream=None):
    """Both lognorm calls against float64 (1e-5 / 1e-4), canaries, the input's bits, run-to-run identity.  The gradient of the
    offset input is not compared at F = 2 with the norm on: two frames normalise to +-(1 - 1.25e-4) whatever they are, the true
    gradient is that 1e-4 remainder of a cancellation and a relative error measures the rounding of the fp32 statistics only."""
    s, dy = lognorm_case(N, F, D, seed=N + F + D, offset=offset)
    ref = lognorm_oracle(s, dy, normalise)
    s, dy = s.to(device), dy.to(device)
    s0 = s.clone()
    y, stats = run_lognorm_forward(lib, s, normalise, stream=stream)
    ds = run_lognorm_backward(lib, s, stats, dy, normalise, stream=stream)
    y2, _ = run_lognorm_forward(lib, s, normalise, want_stats=False, stream=stream)
    n = N * F * D
    ey, eds = rel_err(y[:n].view(N, F, D), ref["y"]), rel_err(ds[:n].view(N, F, D), ref["ds"])
    print(f"lognorm N={N} F={F} D={D} normalise={normalise} offset={offset}: y {ey:.3g} ds {eds:.3g}")
    assert ey < 1e-5
    assert eds < 1e-4 or (offset and normalise and F == 2)
    assert bool(torch.isfinite(ds[:n]).all())
    assert tail_ok(y, n) and tail_ok(ds, n) and tail_ok(stats, N * 2 * D) and torch.equal(y, y2) and torch.equal(s, s0)
    if normalise:
        st = stats[:N * 2 * D].view(N, 2, D)
        assert rel_err(st[:, 0], ref["m"]) < 1e-5 and rel_err(st[:, 1], ref["r"]) < 1e-5
    else:
        assert bool((stats == FILL).all())
    assert torch.equal(ds, run_lognorm_backward(lib, s, stats, dy, normalise, stream=stream))


# ---- the reference fixture (tools/make_golden_lfb.py)
def golden():
    with open(os.path.join(GOLDEN, "lfb_meta.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN, "lfb.npz"))), meta


def golden_state(arrays, meta, tag):
    """The fixture's state dict in the reference's key order: seeded conv parameters, the stored window."""
    from oracle.make_golden_predictors import seeded_state
    c = meta["cases"][tag]
    state = seeded_state({k: tuple(v) for k, v in c["shapes"].items()}, c["seed"])
    state["han"] = torch.from_numpy(arrays[f"{tag}_han"])
    return {k: state[k] for k in c["keys"]}


def check_against_golden(enc, arrays, meta, tag, device, y_tol, grad_tol):
    """enc (already loaded) on the fixture's input: y within y_tol * max|y| (None: norm-relative 1e-5), gradients norm-relative."""
    c = meta["cases"][tag]
    x = torch.from_numpy(arrays[f"{tag}_x"]).to(device)
    want = torch.from_numpy(arrays[f"{tag}_y"])
    y = enc(x)
    assert tuple(y.shape) == tuple(want.shape)
    if y_tol is None:
        assert rel_err(y.detach(), want) < 1e-5
    else:
        assert float((y.detach().cpu() - want).abs().max()) <= y_tol * float(want.abs().max())
    if c["grads"]:
        (y * torch.from_numpy(arrays[f"{tag}_dy"]).to(device)).sum().backward()
        assert rel_err(enc.conv.weight.grad, torch.from_numpy(arrays[f"{tag}_dweight"])) < grad_tol
        assert rel_err(enc.conv.bias.grad, torch.from_numpy(arrays[f"{tag}_dbias"])) < grad_tol
