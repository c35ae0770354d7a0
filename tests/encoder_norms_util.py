"""Shared by the tests of the encoder's batchNorm / instanceNorm / ID modes (cpc_encoder_*_n, csrc/enc_wide.hip): the
float64 reference, one NaN-prefilled run through the C ABI on any library (emulator or device), and the comparison.

The reference states the reference's modules in float64 with oneDNN off: F.conv1d, then F.batch_norm / F.instance_norm / nothing,
then the oracle's tie-aware ReLU fed the device's masks (tests/test_emu_encoder_widths.py)."""
import ctypes

import torch
import torch.nn.functional as F

from oracle import cpc_oracle as O

GEOM = ((10, 5, 3), (8, 4, 2), (4, 2, 1), (4, 2, 1), (4, 2, 1))
NORM = {"layerNorm": 0, "batchNorm": 1, "instanceNorm": 2, "ID": 3}
SLOTS = 32                       # cpc_encoder_layout_n
MOMENTUM, EPS = 0.1, 1e-5
# (normMode, training): the four arithmetic variants
VARIANTS = [("batchNorm", True), ("batchNorm", False), ("instanceNorm", True), ("ID", True)]
# (C, B, L): one block of 3 channels; L_4 = 8 with three utterances inside one row block; a ragged channel block; a layer-0 step no
# layer-1 window touches; the padded path at 256 with L_4 = 4; the full eight blocks
CASES = [(3, 2, 1280), (30, 3, 1290), (65, 1, 1370), (130, 2, 978), (256, 1, 650), (512, 1, 650)]
NAMES = [f"{n}{i}.{w}" for i in range(5) for n, w in (("conv", "weight"), ("conv", "bias"), ("batchNorm", "weight"),
                                                      ("batchNorm", "bias"))]
# The offset case: every conv bias + 10 at (30, 3, 1290).  torch fp32 against float64 on the CPU for it, max |delta| over y0..y3 and z
# / worst gradient: batchNorm training 4.6e-5 / 1.33e-5, batchNorm eval 1.36e-5 / 4.3e-7, instanceNorm 4.53e-5 / 1.55e-5, ID 9.9e-6 /
# 4.3e-7 (x = 10 + O(1) has an ulp of 1e-6 before a normalisation whose rstd reaches 25).  Where that figure is above half the
# emulator's bar of 2e-5 the case has a bar of its own, four times the figure; all of them are below half the device's
# 1e-4, which therefore stays.
OFFSET_CASE = (30, 3, 1290, 10.0)
OFFSET_TORCH_FP32 = {("batchNorm", True): (4.6e-5, 1.33e-5), ("batchNorm", False): (1.36e-5, 4.3e-7),
                     ("instanceNorm", True): (4.53e-5, 1.55e-5), ("ID", True): (9.9e-6, 4.3e-7)}


def offset_bars(mode, training, bar):
    """(forward bar, gradient bar) of the offset case under the ordinary bar `bar`"""
    return tuple(4 * f if f > bar / 2 else bar for f in OFFSET_TORCH_FP32[(mode, training)])


def P(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_params(C, mode, seed=0, bias_offset=0.0):
    """The oracle's parameters with the norm weights as the torch modules hold them, (C,); under batchNorm also running statistics
    away from (0, 1).  ID has the conv tensors only."""
    p = O.make_params(seed=seed, hidden_encoder=C)
    out = {}
    for n in NAMES:
        if "batchNorm" in n:
            if mode != "ID":
                out[n] = p["gEncoder." + n].reshape(C).contiguous()
        else:
            out[n] = (p["gEncoder." + n] + (bias_offset if n.endswith("bias") else 0.0)).contiguous()
    running = None
    if mode == "batchNorm":
        g = torch.Generator().manual_seed(seed + 77)
        running = [t for _ in range(5) for t in (0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g))]
    return out, running


def reference64(mode, training, params, running, wave, dz=None, relu_override=None):
    """-> z (B, L_4, C), [y0..y3] channels-last, the float64 leaves (with .grad when dz is given), the running buffers after the
    call, and dx_i = the gradient at each conv's output (B, C, L_i)."""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    run = None if running is None else [r.double().clone() for r in running]
    acts, convs = [], []
    x = wave.double()
    with torch.backends.mkldnn.flags(enabled=False):
        for i, (_, s, p) in enumerate(GEOM):
            x = F.conv1d(x, leaves[f"conv{i}.weight"], leaves[f"conv{i}.bias"], stride=s, padding=p)
            x.retain_grad()
            convs.append(x)
            if mode == "batchNorm":
                x = F.batch_norm(x, run[2 * i], run[2 * i + 1], leaves[f"batchNorm{i}.weight"], leaves[f"batchNorm{i}.bias"],
                                 training, MOMENTUM, EPS)
            elif mode == "instanceNorm":
                x = F.instance_norm(x, None, None, leaves[f"batchNorm{i}.weight"], leaves[f"batchNorm{i}.bias"], True, MOMENTUM, EPS)
            x = torch.relu(x) if relu_override is None else O._ReluTieAware.apply(x, relu_override[i], 1e-5)
            acts.append(x)
        z = x.permute(0, 2, 1)
        if dz is not None:
            (z * dz.double()).sum().backward()
    ys = [a.detach().permute(0, 2, 1).contiguous() for a in acts[:4]]
    return z.detach(), ys, leaves, run, [c.grad for c in convs]


def run_abi(lib, mode, training, C, B, L, params, running, wave, dz=None, dev="cpu", fill=float("nan"), stream=None, backward=True):
    """One cpc_encoder_forward_n (+ _backward_n) on buffers prefilled with `fill` -> dict(z, ys, grads {name: tensor}, running
    (after the call), dz, sizes, saved), all on the CPU except saved."""
    norm, tr = NORM[mode], int(training)
    sizes = (ctypes.c_long * SLOTS)()
    assert lib.cpc_encoder_layout_n(B, L, C, norm, tr, sizes) == 0
    Ls = [sizes[3 + i] for i in range(5)]
    slots = [params.get(n) for n in NAMES]
    dslots = [None if t is None else t.to(dev) for t in slots]
    run = None if running is None else [r.clone().to(dev) for r in running]
    wd = wave.to(dev)
    saved = torch.full((max(1, sizes[0]),), fill, device=dev)
    fscr = torch.full((max(1, sizes[1]),), fill, device=dev)
    z = torch.full((B, Ls[4], C), float("nan"), device=dev)
    parr = (ctypes.c_void_p * 20)(*[P(t) for t in dslots])
    rarr = None if run is None else (ctypes.c_void_p * 10)(*[P(t) for t in run])
    assert lib.cpc_encoder_forward_n(P(wd), parr, rarr, P(saved), P(fscr), P(z), B, L, C, norm, tr, MOMENTUM, EPS, stream) == 0
    ys = []
    for i in range(4):
        y = torch.full((B, Ls[i], C), float("nan"), device=dev)
        assert lib.cpc_encoder_saved_activation_n(P(saved), i, P(y), B, L, C, norm, stream) == 0
        ys.append(y.cpu())
    out = dict(z=z.cpu(), ys=ys, running=None if run is None else [r.cpu() for r in run], sizes=list(sizes), saved=saved, grads=None,
               dz=dz)
    if not backward:
        return out
    if dz is None:
        dz = torch.randn(B, Ls[4], C, generator=torch.Generator().manual_seed(11))
    dzd = dz.to(dev)
    bscr = torch.full((sizes[2],), fill, device=dev)
    grads = [None if t is None else torch.full_like(t, float("nan")) for t in dslots]
    garr = (ctypes.c_void_p * 20)(*[P(t) for t in grads])
    assert lib.cpc_encoder_backward_n(P(wd), parr, P(saved), P(z), P(dzd), P(bscr), garr, B, L, C, norm, tr, stream) == 0
    out["grads"] = {n: g.cpu() for n, g in zip(NAMES, grads) if g is not None}
    out["dz"] = dz
    return out


def compare(mode, training, params, running, wave, res, bar, check_grads=True, grad_bar=None):
    """The parity statement of both suites.  max |delta| < bar on y0..y3 and z; every gradient within bar (norm-wise relative)
    -- except the conv bias gradient where the normalisation removes the mean (batchNorm in training, instanceNorm): analytically
    zero, torch fp32 itself returns rounding noise, so |G[c]| <= 1e-4 sum over rows |dx[row, c]| with dx from float64."""
    grad_bar = bar if grad_bar is None else grad_bar
    O.tie_report()
    z_ref, ys_ref, leaves, run_ref, dxs = reference64(mode, training, params, running, wave, res["dz"] if check_grads else None,
                                                       [(y > 0).permute(0, 2, 1) for y in res["ys"] + [res["z"]]])
    ties = O.tie_report()
    print(f"relu ties: {ties}")
    assert O.tie_ok(ties) and ties["disagree_outside"] == 0, ties
    assert z_ref.shape == res["z"].shape
    for i in range(4):
        err = (res["ys"][i].double() - ys_ref[i]).abs().max().item()
        print(f"y{i}: max |delta| = {err:.3g}")
        assert err < bar, f"layer {i}"
    err = (res["z"].double() - z_ref).abs().max().item()
    print(f"z: max |delta| = {err:.3g}")
    assert err < bar
    if not check_grads:
        return run_ref
    bad = {}
    zero_bias = mode == "instanceNorm" or (mode == "batchNorm" and training)
    assert set(res["grads"]) == set(params)
    for n, g in res["grads"].items():
        ref = leaves[n].grad
        assert g.shape == ref.shape
        if not torch.isfinite(g).all():
            bad[n] = float("inf")
        elif zero_bias and n.startswith("conv") and n.endswith("bias"):
            bound = 1e-4 * dxs[int(n[4])].abs().sum(dim=(0, 2))
            worst = (g.double().abs() / bound).max().item()
            print(f"{n}: max |G| / (1e-4 sum |dx|) = {worst:.3g}")
            if not worst <= 1.0:
                bad[n] = worst
        else:
            e = rel_err(g, ref)
            print(f"{n}: {e:.3g}")
            if not e < grad_bar:
                bad[n] = e
    assert not bad, bad
    return run_ref
