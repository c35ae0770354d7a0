"""Shared by the dropout-mask tests of the transformer layer (emulator and GPU): the layer's dropout entry points called through
the C ABI on whatever device the tensors live on, and the oracle (oracle/transformer_oracle.py) fed the masks of the independent
reference (tests/philox_util.py) -- never masks the library reports."""
import ctypes

import torch

import philox_util as PU
from oracle import transformer_oracle as T

ORDER = ["multihead.Wo.weight", "multihead.Wk.weight", "multihead.Wq.weight", "multihead.Wv.weight",
         "multihead.Att.Krelpos", "ln_multihead.weight", "ln_multihead.bias", "ffnetwork.lin1.weight",
         "ffnetwork.lin1.bias", "ffnetwork.lin2.weight", "ffnetwork.lin2.bias", "ln_ffnetwork.weight",
         "ln_ffnetwork.bias"]
MASK64 = (1 << 64) - 1


def P(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def library_masks(lib, BH, S, rows, p, seed, device="cpu", stream=None):
    """cpc_dropout_keep_mask of both sites (either may be skipped with 0 elements) -> (BH, S, S), (rows, 2048) on the CPU."""
    out = []
    for site, shape in ((0, (BH, S, S)), (1, (rows, 2048))):
        if shape[0] == 0:
            out.append(None)
            continue
        m = torch.full(shape, float("nan"), device=device)
        assert lib.cpc_dropout_keep_mask(P(m), m.numel(), site, S, p, seed & MASK64, stream) == 0
        out.append(m)
    if device != "cpu":
        torch.cuda.synchronize()
    return [None if m is None else m.cpu() for m in out]


def layer_call(lib, prm, x, dy, p, seed, stream=None):
    """cpc_transformer_layer_forward_dropout + _backward_dropout on x's device -> out, dx, {name: gradient}, all on the CPU."""
    dev = x.device
    B, S = x.shape[:2]
    plist = [prm[k].contiguous().to(dev) if k in prm else None for k in ORDER]
    sizes = (ctypes.c_long * 8)()
    assert lib.cpc_transformer_layout(B, S, sizes) == 0
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)       # noqa: E731
    saved, fscr, bscr = nan(sizes[0]), nan(sizes[1]), nan(sizes[2])
    out, dx = nan(B, S, 256), nan(B, S, 256)
    grads = [torch.full_like(t, float("nan")) if t is not None else None for t in plist]
    parr = (ctypes.c_void_p * 13)(*[P(t) for t in plist])
    garr = (ctypes.c_void_p * 13)(*[P(t) for t in grads])
    assert lib.cpc_transformer_layer_forward_dropout(P(x), parr, P(saved), P(fscr), P(out), B, S, p, seed & MASK64, stream) == 0
    assert lib.cpc_transformer_layer_backward_dropout(P(x), parr, P(saved), P(dy), P(bscr), P(dx), garr, B, S, p, seed & MASK64,
                                                      stream) == 0
    if dev.type != "cpu":
        torch.cuda.synchronize()
    return out.cpu(), dx.cpu(), {k: g.cpu() for k, g in zip(ORDER, grads) if g is not None}


def group_call(lib, prms, x, dy, p, seed, stream=None):
    """cpc_transformer_group_forward + _backward for the G layers `prms` -> out (B*S, G*256), dx, {name: (G, ...) gradients}."""
    dev = x.device
    B, S = x.shape[:2]
    G = len(prms)
    kinds = [k for k in ORDER if k in prms[0]]
    stacked = {k: torch.stack([q[k] for q in prms]).contiguous().to(dev) for k in kinds}
    sizes = (ctypes.c_long * 8)()
    assert lib.cpc_transformer_layout(B, S, sizes) == 0
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)       # noqa: E731
    saved, fscr, bscr = nan(G * sizes[0]), nan(G * sizes[1]), nan(G * sizes[2])
    out, dx = nan(B * S, G * 256), nan(B, S, 256)
    sgrads = {k: torch.full_like(v, float("nan")) for k, v in stacked.items()}
    parr = (ctypes.c_void_p * 13)(*[P(stacked[k]) if k in stacked else None for k in ORDER])
    garr = (ctypes.c_void_p * 13)(*[P(sgrads[k]) if k in sgrads else None for k in ORDER])
    assert lib.cpc_transformer_group_forward(P(x), parr, P(saved), P(fscr), P(out), B, S, G, p, seed & MASK64, stream) == 0
    assert lib.cpc_transformer_group_backward(P(x), parr, P(saved), P(dy), P(bscr), P(dx), garr, B, S, G, p, seed & MASK64,
                                              stream) == 0
    if dev.type != "cpu":
        torch.cuda.synchronize()
    return out.cpu(), dx.cpu(), {k: g.cpu() for k, g in sgrads.items()}


def oracle_with_reference_masks(prm, x, dy, p, seed, prefix=""):
    """The oracle's layer under the REFERENCE's masks of `seed` -> y, dx, {name: gradient}, smallest |hidden pre-activation| of a
    kept unit (a unit within fp32 rounding of zero may take the other side of the ReLU on a device: see the GPU test)."""
    B, S = x.shape[:2]
    attn_keep = PU.attn_keep_ref(B * 8, S, p, seed & MASK64)
    ffn_keep = PU.ffn_keep_ref(B * S, p, seed & MASK64).view(B, S, 2048)
    leaves = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
    xr = x.clone().requires_grad_(True)
    yr = T.layer_forward(leaves, xr, prefix=prefix, attn_keep=attn_keep, ffn_keep=ffn_keep)
    (yr * dy).sum().backward()
    with torch.no_grad():                                                   # float64: where do the hidden units sit?
        got = {}
        T.layer_forward({k: v.double() for k, v in prm.items()}, x.double(), prefix=prefix, collect=got, attn_keep=attn_keep.double(),
                        ffn_keep=ffn_keep.double())
        pre = got["y"] @ prm[f"{prefix}ffnetwork.lin1.weight"].double().t() + prm[f"{prefix}ffnetwork.lin1.bias"].double()
        nearest = pre.abs()[ffn_keep > 0].min().item()
    return yr.detach(), xr.grad, {k[len(prefix):]: v.grad for k, v in leaves.items()}, nearest


def assert_layer_matches(got, ref, tol, what):
    """|y - y_ref| < tol absolute; dx and every parameter gradient < tol relative (norm-wise).  Prints each figure first.
    A gradient whose reference is EXACTLY zero has no relative error (S = 1: the softmax of a single score is constant, so Wq, Wk
    and Krelpos receive none, while a device that forms dScore = A (dA - sum A dA) from two differently rounded products leaves
    rounding noise there).  Its norm is then measured against the norm of Wv's reference gradient: the same shape and operand
    (x^T .) out of the same attention backward, i.e. the scale a perturbation of dq or dk is measured against as soon as S > 1 --
    a mask that differed between forward and backward would put a term of that very size there."""
    out, dx, grads = got
    yr, dxr, gr, nearest = ref
    dev_y = (out - yr).abs().max().item()
    dev_dx = 0.0 if dx is None else rel_err(dx, dxr)                # (None: a group's dx is the sum over its layers, checked by the caller)
    scale = {k: (v if v.norm().item() > 0 else gr["multihead.Wv.weight"]) for k, v in gr.items()}
    rels = {k: ((g - gr[k]).norm() / scale[k].norm()).item() for k, g in grads.items()}
    worst = max(rels, key=rels.get)
    print(f"{what}: max|dy| {dev_y:.2e}  rel dx {dev_dx:.2e}  worst gradient {worst} {rels[worst]:.2e}  "
          f"(nearest kept hidden pre-activation to zero, float64: {nearest:.2e})")
    assert dev_y < tol, (what, dev_y)
    assert dev_dx < tol, (what, dev_dx)
    bad = {k: r for k, r in rels.items() if not r < tol}
    assert not bad, (what, bad)
