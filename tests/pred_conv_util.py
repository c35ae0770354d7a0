"""Shared by the prediction-network tests (csrc/pred_conv.hip): seeded cases, the float64 CPU oracle built from this package's
own torch modules (criterion.ShiftedConv / FFNetwork, ``.double()``) and the calls through the C ABI (the emulator library on
the CPU, the product library on the GPU)."""
import ctypes
import math

import torch

H = 256

# name -> (B, W, G, ks): the smallest shapes at which the kernels can go wrong
CASES = {
    "a_window_shorter_than_taps": (2, 6, 3, 12),      # whole leading taps are padding
    "b_three_items_in_one_tile": (3, 6, 1, 4),        # item b must read nothing of item b - 1
    "c_ragged_row_tiles": (2, 70, 2, 4),              # rows cross a tile boundary, the last tile is ragged, three dW row slabs
    "e_more_heads_than_a_score_group": (1, 6, 17, 4),
}


def P(t):
    return None if t is None else t.data_ptr()


def layout(lib, B, W, G, ks):
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_pred_conv_layout(B, W, G, ks, sizes) == 0
    return tuple(sizes)          # wr floats, backward scratch floats, y floats


def scale_of(ks):
    """The equalized layer's constant (custom_layers.py:33-42): sqrt(2 / fan_in)."""
    return math.sqrt(2.0 / (H * ks))


def conv_case(B, W, G, ks, shared=True, seed=0):
    """x, the stacked weight (G, 256, 256, ks), the stacked bias (G, 256) and an output gradient."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + 10 * W + G + ks)
    x = torch.randn(B, W, H if shared else G * H, generator=g)
    w = torch.randn(G, H, H, ks, generator=g)
    b = torch.randn(G, H, generator=g)
    dy = torch.randn(B, W, G * H, generator=g)
    return x, w, b, dy


def oracle(x, w, b, shared, relu, dy=None):
    """float64: head g is criterion.ShiftedConv(256, 256, ks) carrying (w[g], b[g]) on its input (x, or columns g*256.. of x),
    followed by ReLU when ``relu``; the heads one behind the other along the last axis.  With dy: (y, dw, db, dx)."""
    from cpc_audio_amd.criterion import ShiftedConv
    G, ks = w.shape[0], w.shape[3]
    xr = x.double().clone().requires_grad_(True)
    heads = []
    for g in range(G):
        m = ShiftedConv(H, H, ks).double()
        with torch.no_grad():
            m.module.module.weight.copy_(w[g].double())
            m.module.module.bias.copy_(b[g].double())
        heads.append(m)
    outs = []
    for g, m in enumerate(heads):
        o = m(xr if shared else xr[:, :, g * H:(g + 1) * H])
        outs.append(torch.relu(o) if relu else o)
    y = torch.cat(outs, dim=2)
    if dy is None:
        return y.detach()
    (y * dy.double()).sum().backward()
    dw = torch.stack([m.module.module.weight.grad for m in heads])
    db = torch.stack([m.module.module.bias.grad for m in heads])
    return y.detach(), dw, db, xr.grad


def without_relu_ties(x, w, b, shared, dy, eps=1e-5):
    """dy with zeros where the float64 pre-activation lies within eps of zero.  There the ReLU's derivative is not defined by the
    arithmetic: fp32 rounding (~1e-7 here) decides the sign, the kernels mask by their own y > 0 and the float64 oracle by its
    own, and ONE such element among n moves a gradient's rel_err by about 1 / sqrt(n) -- 3e-4 at 10^7 outputs, where about one
    is expected.  Those elements take no gradient in the comparison; every other one is held to the bar."""
    pre = oracle(x, w, b, shared, False)
    ties = pre.abs() < eps
    return dy.masked_fill(ties, 0.0), int(ties.sum())


def run(lib, x, w, b, shared, relu, dy=None, need_dx=True, canary=0, fill=7.0):
    """cpc_pred_conv_forward (+ _backward with dy) on the tensors' device; outputs carry `canary` spare floats."""
    B, W, _ = x.shape
    G, ks = w.shape[0], w.shape[3]
    wr_n, scr_n, y_n = layout(lib, B, W, G, ks)
    assert y_n == B * W * G * H and wr_n == G * ks * H * H
    dev = x.device
    x, w, b = x.contiguous(), w.contiguous(), b.contiguous()
    s = scale_of(ks)
    wr = torch.full((wr_n + canary,), fill, device=dev)
    y = torch.full((y_n + canary,), fill, device=dev)
    assert lib.cpc_pred_conv_forward(P(x), P(w), P(b), P(wr), P(y), B, W, G, ks, int(shared), s, int(relu), None) == 0
    out = dict(wr=wr, y=y, n=dict(wr=wr_n, y=y_n, scratch=scr_n, dw=w.numel(), db=b.numel(), dx=x.numel()))
    if dy is not None:
        dy = dy.contiguous()
        scratch = torch.full((scr_n + canary,), float("nan"), device=dev)
        dw = torch.full((w.numel() + canary,), fill, device=dev)
        db = torch.full((b.numel() + canary,), fill, device=dev)
        dx = torch.full((x.numel() + canary,), fill, device=dev) if need_dx else None
        assert lib.cpc_pred_conv_backward(P(x), P(w), P(y) if relu else None, P(dy), P(scratch), P(dw), P(db), P(dx), B, W, G, ks,
                                          int(shared), s, int(relu), None) == 0
        out.update(scratch=scratch, dw=dw, db=db, dx=dx)
    return out


def canaries_ok(out, canary, fill=7.0):
    for k in ("wr", "y", "scratch", "dw", "db", "dx"):
        if out.get(k) is None:
            continue
        tail = out[k][out["n"][k]:]
        assert tail.numel() == canary, k
        assert bool(torch.isnan(tail).all()) if k == "scratch" else bool((tail == fill).all()), k


def rel_err(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def check_against_oracle(out, x, w, b, dy, shared, relu, fwd_bar, grad_bar, show=None):
    """Compare one run() against the oracle; prints every figure before asserting it."""
    y, dw, db, dx = oracle(x.cpu(), w.cpu(), b.cpu(), shared, relu, dy.cpu())
    n = out["n"]
    errs = {
        "y": (rel_err(out["y"][:n["y"]].cpu().double().view_as(y), y), fwd_bar),
        "dw": (rel_err(out["dw"][:n["dw"]].cpu().double().view_as(dw), dw), grad_bar),
        "db": (rel_err(out["db"][:n["db"]].cpu().double().view_as(db), db), grad_bar),
        "dx": (rel_err(out["dx"][:n["dx"]].cpu().double().view_as(dx), dx), grad_bar),
    }
    print(show or "", {k: f"{e:.3e}" for k, (e, _) in errs.items()})
    for k, (e, bar) in errs.items():
        assert e < bar, (k, e, bar)
    G, ks = w.shape[0], w.shape[3]
    assert torch.equal(out["wr"][:n["wr"]].cpu().view(G, H, ks, H), w.cpu().permute(0, 1, 3, 2))
