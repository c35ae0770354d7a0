"""A plain torch model of the bf16-storage encoder (cpc_set_mfma_mode(4)) that rounds where the kernels round, and the rules by
which the emulator and GPU tests compare the kernels with it (tests/test_emu_bf16_rounding.py, tests/test_gpu_bf16_rounding.py).

The variant's rounding points (everything between them is fp32 on the device):
  * y0 = bf16(relu(.)) in conv0's forward (enc_conv0.hip);
  * y_i = bf16(relu(xh w + b)) and the saved xhat_i = bf16(xh) in the forward epilogue (conv_dma.hip), xh itself unrounded; z is fp32;
  * the conv weights of layers 1..4, rounded to bf16 by the re-layouts (permute_w_*_bf16_elem), for forward and data gradient alike;
  * dx_i = bf16(v) in the norm backward (norm_bwd_kernel<2, ., true>); its ReLU mask is the sign of bf16(xh) w + b;
  * the data gradient bf16(conv1d_input(dx_i, bf16(W_i))) (conv_dgrad_dma_kernel), which for layer 1 is conv0's dy0.
Every stage below takes a dtype: float64 is the reference, float32 its companion -- the distance between the two runs of a stage
on the same inputs is the tolerance the device gets (see `Report`).  Each stage is fed the DEVICE's stored inputs, so one flipped
bf16 element does not spread down the stack.
Tensors are channels-last (n, steps, 256) like the device's; stages return their outputs BEFORE the bf16 rounding of the store
(the comparison rounds), and round what the kernels round on the way: the weights and the data gradient between two stages."""
import ctypes

import torch
import torch.nn.functional as F
from torch.nn.grad import conv1d_input, conv1d_weight

C = 256
GEOM = [(10, 5, 3), (8, 4, 2), (4, 2, 1), (4, 2, 1), (4, 2, 1)]      # (k, s, p) of the five conv layers
EPS = 1e-5                                                          # ChannelNorm's epsilon
NAMES = [f"gEncoder.{n}{i}.{w}" for i in range(5)
         for n, w in (("conv", "weight"), ("conv", "bias"), ("batchNorm", "weight"), ("batchNorm", "bias"))]


# ---------------------------------------------------------------------------------------------------------------- helpers
def bf16_round(x):
    """Round to the nearest bf16, ties to even, as bf16_rne does: of the FLOAT32 value (a float64 input is first brought to
    float32, which is what the device holds -- rounding the float64 value to bf16 directly could land on the other side of a tie)."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def bf16_ulp(x):
    """Spacing of the bf16 values around x (8 significant bits): 2^(floor(log2|x|) - 7), for zero the smallest normal binade's."""
    _, e = torch.frexp(x.detach().to(torch.float64).abs())          # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e.clamp_min(-125) - 8)


def read_bf16(buf, off, shape):
    """The bf16 tensor of `shape` that starts `off` FLOATS into the float32 buffer `buf` (saved workspace / backward scratch)."""
    n = 1
    for d in shape:
        n *= d
    return buf[off:off + (n + 1) // 2].view(torch.bfloat16)[:n].view(*shape)


def read_f32(buf, off, shape):
    n = 1
    for d in shape:
        n *= d
    return buf[off:off + n].view(*shape)


def uncovered_steps(Lin, i):
    """Input steps of layer i (i >= 1) that no window of the conv touches: their data gradient is exactly zero."""
    k, s, p = GEOM[i]
    Lout = (Lin + 2 * p - k) // s + 1
    return list(range((Lout - 1) * s + k - p, Lin))


def _aff(t, dt):
    return t.reshape(-1).to(dt)


# ----------------------------------------------------------------------------------------------------------------- stages
def layer_forward(i, x_in, W, b, gw, gb, dt, rnd=True):
    """Layer i on x_in: the waveform (n, 1, L) for i = 0 (fp32 weights), a bf16-valued (n, Lin, 256) tensor and bf16(W) for
    i >= 1.  Returns mean, rstd (n, Lout) and xhat, y (n, Lout, 256), all unrounded: xhat = (a - mean) rstd with the unbiased
    variance, y = relu(xhat w + b) on that unrounded xhat."""
    k, s, p = GEOM[i]
    Wq = bf16_round(W) if (rnd and i >= 1) else W
    x = x_in if i == 0 else x_in.permute(0, 2, 1)
    a = F.conv1d(x.to(dt), Wq.to(dt), b.to(dt), stride=s, padding=p)          # (n, C, T)
    m = a.sum(1, keepdim=True) / C
    d = a - m
    rs = torch.rsqrt((d * d).sum(1, keepdim=True) / (C - 1) + EPS)
    xh = d * rs
    pre = xh * _aff(gw, dt)[None, :, None] + _aff(gb, dt)[None, :, None]
    return {"mean": m[:, 0, :], "rstd": rs[:, 0, :], "xhat": xh.permute(0, 2, 1), "y": torch.relu(pre).permute(0, 2, 1),
            "xw": (xh * _aff(gw, dt)[None, :, None]).permute(0, 2, 1), "pre": pre.permute(0, 2, 1)}


def bwd_mask(xhat, gw, gb):
    """The norm backward's ReLU mask: the sign of xhat w + b on the xhat it is given (the stored bf16 one in this mode), exact --
    fmaf rounds once, which keeps the sign; in float64 the product of an 8-bit and a 24-bit significand is exact."""
    return (xhat.double() * gw.reshape(-1).double() + gb.reshape(-1).double()) > 0


def norm_backward(dy, xhat, rstd, gw, gb, dt):
    """ReLU' + ChannelNorm backward of one layer.  dy, xhat (n, T, 256), rstd (n, T).  Returns v (the unrounded dx; the kernel
    stores bf16(v)), d norm.weight, d norm.bias (column sums over the masked dy) and d conv.bias (the sum of the unrounded v)."""
    mask = bwd_mask(xhat, gw, gb)
    dy, xhat, rs, w = dy.to(dt), xhat.to(dt), rstd.to(dt)[..., None], _aff(gw, dt)
    dyh = torch.where(mask, dy, torch.zeros_like(dy))
    dxh = dyh * w
    s1 = dxh.sum(-1, keepdim=True) / C
    s2 = (dxh * xhat).sum(-1, keepdim=True) / (C - 1)
    v = rs * (dxh - s1 - xhat * s2)
    return {"v": v, "dnw": (dyh * xhat).sum((0, 1)), "dnb": dyh.sum((0, 1)), "dcb": v.sum((0, 1)), "mask": mask}


def dgrad(i, dx, W, Lin, dt, rnd=True):
    """Data gradient of layer i (i >= 1) from dx (n, Lout, 256) w.r.t. its (n, Lin, 256) input, unrounded (the kernel stores
    bf16 of it); steps that no window covers come out exactly zero."""
    k, s, p = GEOM[i]
    Wq = (bf16_round(W) if rnd else W).to(dt)
    g = conv1d_input((dx.shape[0], C, Lin), Wq, dx.to(dt).permute(0, 2, 1).contiguous(), stride=s, padding=p)
    return g.permute(0, 2, 1)


def wgrad(i, dx, x_in, dt):
    """Weight gradient of layer i (i >= 1) from dx (n, Lout, 256) and the layer's input (n, Lin, 256); fp32 on the device."""
    k, s, p = GEOM[i]
    return conv1d_weight(x_in.to(dt).permute(0, 2, 1).contiguous(), (C, C, k), dx.to(dt).permute(0, 2, 1).contiguous(),
                         stride=s, padding=p)


def layer0_backward(wave, W, b, gw, gb, mean0, rstd0, dy0, dt):
    """Layer 0's four gradients from dy0 (bf16-valued): xhat0 is recomputed from the waveform and the saved mean0 / rstd0, its
    mask from that xhat0."""
    k, s, p = GEOM[0]
    a = F.conv1d(wave.to(dt), W.to(dt), b.to(dt), stride=s, padding=p).permute(0, 2, 1)
    xh = (a - mean0.to(dt)[..., None]) * rstd0.to(dt)[..., None]
    nb = norm_backward(dy0, xh, rstd0, gw, gb, dt)
    dw = conv1d_weight(wave.to(dt), tuple(W.shape), nb["v"].permute(0, 2, 1).contiguous(), stride=s, padding=p)
    return {"dw": dw, "dcb": nb["dcb"], "dnw": nb["dnw"], "dnb": nb["dnb"]}


def chain(plist, wave, dz, dt, rnd):
    """The whole encoder, forward and backward, on the model's OWN tensors: every stage above in the order the device runs them.
    rnd = False switches every rounding off -- then this is the plain encoder, which is how the model is validated against the
    oracle (tests/test_bf16_model_cpu.py) before anything is compared with it."""
    q = (lambda t: bf16_round(t)) if rnd else (lambda t: t)
    acts, xh, rs = [], [None] * 5, [None] * 5
    x = wave
    for i in range(5):
        f = layer_forward(i, x, *plist[4 * i:4 * i + 4], dt, rnd)
        if i == 0:
            mean0 = f["mean"]
        rs[i], xh[i] = f["rstd"], q(f["xhat"])
        x = f["y"] if i == 4 else q(f["y"])
        acts.append(x)
    g = [None] * 20
    dy = dz
    for i in range(4, 0, -1):
        nb = norm_backward(dy, xh[i], rs[i], plist[4 * i + 2], plist[4 * i + 3], dt)
        g[4 * i + 1], g[4 * i + 2], g[4 * i + 3] = nb["dcb"], nb["dnw"], nb["dnb"]
        dx = q(nb["v"])
        g[4 * i] = wgrad(i, dx, acts[i - 1], dt)
        dy = q(dgrad(i, dx, plist[4 * i], acts[i - 1].shape[1], dt, rnd))
    l0 = layer0_backward(wave, *plist[0:4], mean0, rs[0], dy, dt)
    g[0], g[1], g[2], g[3] = l0["dw"], l0["dcb"], l0["dnw"], l0["dnb"]
    return acts, g


# ----------------------------------------------------------------------------------------------------------- comparison rules
MARGIN = 8                    # t = MARGIN * e_ref: a different summation order and whatever the MFMA does inside a 16-deep product
FLIP_CAP = 1e-3               # share of elements of a bf16 tensor with dev != bf16(m64)
REF_FLIP_CAP = 5e-4           # ... and of bf16(m32) != bf16(m64) on the same inputs: what the reference pair itself must stay under
F32_FLOOR = 4 * 2.0 ** -23    # fp32 tensors: + this times max|m64|


class Report:
    """Collects the comparisons of one case; prints a line per tensor; `assert_ok` fails with every violated rule.

    m64 / m32: the float64 model's and its float32 companion's output of the stage, on the same (device-stored) inputs,
    before the store's rounding.  e_ref = max|m32 - m64| over the tensor, t = 8 e_ref.
      bf16-stored tensor: every element |dev - m64| <= bf16_ulp(m64) / 2 + t; share(dev != bf16(m64)) <= 1e-3;
                          share(bf16(m32) != bf16(m64)) < 5e-4; elements of `zero` (structural zeros) exactly zero.
      fp32 tensor:        every element |dev - m64| <= t + 4 2^-23 max|m64|."""

    def __init__(self, tag=""):
        self.tag, self.failures, self.rows = tag, [], []

    def _fail(self, msg):
        self.failures.append(msg)

    def bf16(self, name, dev, m64, m32, zero=None):
        dev, m64, m32 = dev.double(), m64.double(), m32.double()
        assert dev.shape == m64.shape == m32.shape, (name, dev.shape, m64.shape, m32.shape)
        e_ref = (m32 - m64).abs().max().item()
        t = MARGIN * e_ref
        bound = 0.5 * bf16_ulp(m64) + t
        ratio = ((dev - m64).abs() / bound).max().item() if torch.isfinite(dev).all() else float("inf")
        # (how much of t the worst element uses beyond its half ulp: what a GPU that needed a wider margin would show)
        used = (((dev - m64).abs() - 0.5 * bf16_ulp(m64)).max().item() / t) if t > 0 else float("nan")
        flips = (dev != bf16_round(m64)).double().mean().item()
        ref_flips = (bf16_round(m32) != bf16_round(m64)).double().mean().item()
        nz = 0 if zero is None else int((dev[zero.expand_as(dev)] != 0).sum())
        self.rows.append({"name": name, "kind": "bf16", "t": t, "ratio": ratio, "used": used, "flips": flips, "ref_flips": ref_flips})
        print(f"{self.tag} {name:12s} bf16 t {t:.3e}  worst |dev-m64|/bound {ratio:.3f} (beyond ulp/2: {used:.3f} t)  "
              f"flips dev {flips:.2e} ref {ref_flips:.2e}"
              + (f"  nonzero in structural zeros {nz}" if zero is not None else ""))
        if not ratio <= 1.0:
            self._fail(f"{name}: |dev - m64| is {ratio:.3f} x (ulp/2 + t), t = {t:.3e}")
        if not flips <= FLIP_CAP:
            self._fail(f"{name}: {flips:.2e} of the elements differ from bf16(m64)")
        if not ref_flips < REF_FLIP_CAP:
            self._fail(f"{name}: the reference pair itself flips {ref_flips:.2e} of the elements (choose another seed)")
        if nz:
            self._fail(f"{name}: {nz} non-zero elements where no window reaches")

    def f32(self, name, dev, m64, m32):
        dev, m64, m32 = dev.double().reshape(-1), m64.double().reshape(-1), m32.double().reshape(-1)
        assert dev.shape == m64.shape == m32.shape, (name, dev.shape, m64.shape, m32.shape)
        e_ref = (m32 - m64).abs().max().item()
        t = MARGIN * e_ref
        bound = t + F32_FLOOR * m64.abs().max().item()
        ratio = ((dev - m64).abs().max().item() / bound) if torch.isfinite(dev).all() else float("inf")
        self.rows.append({"name": name, "kind": "f32", "t": t, "ratio": ratio})
        print(f"{self.tag} {name:12s} fp32 t {t:.3e}  worst |dev-m64|/bound {ratio:.3f}  (max|m64| {m64.abs().max().item():.3e})")
        if not ratio <= 1.0:
            self._fail(f"{name}: |dev - m64| is {ratio:.3f} x (t + 4 2^-23 max|m64|), t = {t:.3e}")

    @property
    def ok(self):
        return not self.failures

    def assert_ok(self):
        assert not self.failures, "\n".join(self.failures)


# ------------------------------------------------------------------------------------- running the kernels, checking a run
def make_dz(B, L4, items, seed):
    """dz (B, L4, 256), non-zero on the batch items of `items` only (all of them if None)."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randn(B, L4, C, generator=g)
    if items is not None:
        keep = torch.zeros(B, dtype=torch.bool)
        keep[list(items)] = True
        dz[~keep] = 0
    return dz


def run_device(lib, plist, wave, dz_of, device="cpu", stream=None, items=None, keep_dy=True):
    """Forward and backward of the bf16-storage encoder through the C ABI (`lib`: the emulator's or the product library, already in
    mode 4).  dz_of(Ls) gives dz.  Returns CPU tensors of batch items `items` (all if None) of everything the device stores --
    bf16 tensors with their exact values in float32 -- plus the twenty gradients, and `others_zero`: whether dx1..4 and dy0..3 are
    exactly zero on every other item, `z_finite`: whether all of z is finite."""
    B, L = wave.shape[0], wave.shape[2]
    sizes = (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout(B, L, sizes) == 0
    boffs = (ctypes.c_long * 5)()
    assert lib.cpc_encoder_backward_offsets(B, L, boffs) == 0
    Ls = [sizes[3 + i] for i in range(5)]
    P = lambda t: t.data_ptr()
    par = [t.contiguous().to(device) for t in plist]
    wd = wave.contiguous().to(device)
    saved = torch.full((sizes[0],), float("nan"), device=device)
    fscr = torch.full((max(1, sizes[1]),), float("nan"), device=device)
    z = torch.full((B, Ls[4], C), float("nan"), device=device)
    parr = (ctypes.c_void_p * 20)(*[P(t) for t in par])
    assert lib.cpc_encoder_forward(P(wd), parr, P(saved), P(fscr), P(z), B, L, stream) == 0
    dz = dz_of(Ls)
    dzd = dz.contiguous().to(device)
    bscr = torch.full((sizes[2],), float("nan"), device=device)
    grads = [torch.full_like(t, float("nan")) for t in par]
    garr = (ctypes.c_void_p * 20)(*[P(t) for t in grads])
    # dy1..dy3, the data gradients of layers 2..4 (one temporary on the device, overwritten layer by layer): copied out on the way
    keep = torch.full((B * (Ls[1] + Ls[2] + Ls[3]) * C // 2,), float("nan"), device=device) if keep_dy else None
    assert lib.cpc_encoder_keep_data_gradients(P(keep) if keep_dy else None) == 0
    try:
        assert lib.cpc_encoder_backward(P(wd), parr, P(saved), P(z), P(dzd), P(bscr), garr, B, L, stream) == 0
        if device != "cpu":
            torch.cuda.synchronize()
    finally:
        lib.cpc_encoder_keep_data_gradients(None)
    sel = list(range(B)) if items is None else list(items)
    rest = [b for b in range(B) if b not in sel]
    take = lambda t: t[sel].float().cpu()
    run = {"B": B, "L": L, "Ls": Ls, "items": sel, "plist": [t.contiguous() for t in plist], "wave": wave[sel], "dz": dz[sel],
           "z": take(z), "z_finite": bool(torch.isfinite(z).all()),
           "y": [take(read_bf16(saved, sizes[8 + i], (B, Ls[i], C))) for i in range(4)],
           "xhat": [None] + [take(read_bf16(saved, sizes[11 + i], (B, Ls[i], C))) for i in range(1, 5)],
           "rstd": [take(read_f32(saved, sizes[16 + i], (B, Ls[i]))) for i in range(5)],
           "mean0": take(read_f32(saved, sizes[21], (B, Ls[0]))),
           "grads": [g.cpu() for g in grads]}
    dx = [None] + [read_bf16(bscr, boffs[i - 1], (B, Ls[i], C)) for i in range(1, 5)]
    dy0 = read_bf16(bscr, boffs[4], (B, Ls[0], C))
    dy = [dy0]
    if keep_dy:
        off = 0
        for i in range(1, 4):
            dy.append(read_bf16(keep, off // 2, (B, Ls[i], C)))
            off += B * Ls[i] * C
    run["others_zero"] = all(bool((t[rest] == 0).all()) for t in dx[1:] + dy) if rest else True
    run["dx"] = [None] + [take(t) for t in dx[1:]]
    run["dy"] = [take(t) for t in dy]                       # dy[0] = dy0; dy[1..3] only with keep_dy
    return run


def _pair(fn):
    """fn in float64 and in float32.  On ONE thread: torch's reductions split their sums by the number of threads, and the
    float32 run -- with it e_ref and the handful of elements the pair rounds differently -- must not depend on the machine."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.backends.mkldnn.flags(enabled=False):    # (torch's oneDNN conv backward is wrong at some odd lengths)
            return fn(torch.float64), fn(torch.float32)
    finally:
        torch.set_num_threads(threads)


def check_forward(run, rep):
    """Every stored tensor of the forward against the model of ITS layer, fed the device's stored input of that layer."""
    pl = run["plist"]
    for i in range(5):
        x_in = run["wave"] if i == 0 else run["y"][i - 1]
        m64, m32 = _pair(lambda dt: layer_forward(i, x_in, *pl[4 * i:4 * i + 4], dt))
        if i == 0:
            rep.f32("mean0", run["mean0"], m64["mean"], m32["mean"])
        rep.f32(f"rstd{i}", run["rstd"][i], m64["rstd"], m32["rstd"])
        if i >= 1:
            rep.bf16(f"xhat{i}", run["xhat"][i], m64["xhat"], m32["xhat"])
        if i < 4:
            rep.bf16(f"y{i}", run["y"][i], m64["y"], m32["y"])
        else:
            rep.f32("z", run["z"], m64["y"], m32["y"])
    if not run["z_finite"]:
        rep._fail("z is not finite on every batch item")


def check_mask(run, rep):
    """The backward's ReLU mask (sign of bf16(xh) w + b) may differ from the forward's (y > 0, rectified on the unrounded xh) only
    where the bf16 rounding of xh, relative 2^-9, can carry the pre-activation across zero: |xh w + b| <= 2^-8 |xh w|, with xh
    from the float64 model on the device's input."""
    pl = run["plist"]
    for i in range(1, 5):
        with torch.backends.mkldnn.flags(enabled=False):
            m = layer_forward(i, run["y"][i - 1], *pl[4 * i:4 * i + 4], torch.float64)
        y_dev = run["y"][i] if i < 4 else run["z"]
        dis = (y_dev > 0) != bwd_mask(run["xhat"][i], pl[4 * i + 2], pl[4 * i + 3])
        outside = dis & ~(m["pre"].abs() <= 2.0 ** -8 * m["xw"].abs())
        print(f"{rep.tag} mask{i}: forward and backward masks differ on {dis.double().mean().item():.2e} of the elements, "
              f"{int(outside.sum())} of them outside the band")
        if outside.any():
            rep._fail(f"layer {i}: {int(outside.sum())} mask disagreements outside |xh w + b| <= 2^-8 |xh w|")


def check_backward(run, rep, grads=None, tag=""):
    """dx1..4, dy0..3 and the twenty gradients, each against ONE model stage fed the device's own stored tensors:
    layer 4's norm backward from dz; dW_i from the device's dx_i and y_{i-1}; dy_{i-1} (the data gradient) from the device's dx_i;
    dx_{i-1} and layer i-1's three small gradients from the device's dy_{i-1} through the norm backward; layer 0's gradients from
    the device's dy0.
    (dy1..3 share one temporary on the device and do not survive a backward; run_device has them copied out on the way,
    cpc_encoder_keep_data_gradients.  Modelling dgrad + norm backward as ONE stage from dx_i does not work: the float32 and the
    float64 run round a few elements of the intermediate to different bf16 values, each of which moves its whole row of dx_{i-1}
    -- the reference pair then disagrees on 3.5e-3 of dx2's elements at (2, 1280), against a cap of 5e-4, and its e_ref is a
    bf16 ulp of the intermediate instead of fp32 noise.)
    `grads`: another set of gradients to check the weight gradients of (a re-run with another weight-gradient plan); then only
    those are compared."""
    pl, Ls, g = run["plist"], run["Ls"], (grads if grads is not None else run["grads"])
    only_w = grads is not None
    if not run["others_zero"]:
        rep._fail("dx1..4 / dy0 are not exactly zero on the batch items whose dz is zero")

    def small(i, m64, m32):
        rep.f32(f"dconv{i}.b", g[4 * i + 1], m64["dcb"], m32["dcb"])
        rep.f32(f"dnorm{i}.w", g[4 * i + 2], m64["dnw"], m32["dnw"])
        rep.f32(f"dnorm{i}.b", g[4 * i + 3], m64["dnb"], m32["dnb"])

    if not only_w:
        m64, m32 = _pair(lambda dt: norm_backward(run["dz"], run["xhat"][4], run["rstd"][4], pl[18], pl[19], dt))
        rep.bf16("dx4", run["dx"][4], m64["v"], m32["v"])
        small(4, m64, m32)
    for i in range(4, 0, -1):
        m64, m32 = _pair(lambda dt: wgrad(i, run["dx"][i], run["y"][i - 1], dt))
        rep.f32(f"dconv{i}.w{tag}", g[4 * i], m64, m32)
        if only_w:
            continue
        m64, m32 = _pair(lambda dt: dgrad(i, run["dx"][i], pl[4 * i], Ls[i - 1], dt))
        zero = torch.zeros(1, Ls[i - 1], 1, dtype=torch.bool)
        zero[:, uncovered_steps(Ls[i - 1], i)] = True
        rep.bf16(f"dy{i - 1}", run["dy"][i - 1], m64, m32, zero=zero)
        if i >= 2:
            m64, m32 = _pair(lambda dt: norm_backward(run["dy"][i - 1], run["xhat"][i - 1], run["rstd"][i - 1], pl[4 * i - 2],
                                                      pl[4 * i - 1], dt))
            rep.bf16(f"dx{i - 1}", run["dx"][i - 1], m64["v"], m32["v"])
            small(i - 1, m64, m32)
    if not only_w:
        m64, m32 = _pair(lambda dt: layer0_backward(run["wave"], *pl[0:4], run["mean0"], run["rstd"][0], run["dy"][0], dt))
        rep.f32("dconv0.w", g[0], m64["dw"], m32["dw"])
        small(0, m64, m32)
