"""Shared by the feature-width tests of the PER phone classifier's kernels and of the phone posteriors (csrc/phone_head.hip,
csrc/seqnorm.hip, csrc/posterior.hip: the cpc_*_d entry points): seeded cases, the float64 CPU oracles (F.conv1d,
F.log_softmax, F.ctc_loss, F.linear, torch.softmax; seqnorm_util.oracle is the module's own loop under autograd) and the checks
themselves, written once against the C ABI.  tests/test_emu_head_widths.py runs them on the host emulator's build of the
sources (CPU tensors), tests/test_gpu_head_widths.py on the product library (CUDA tensors).

Every output buffer carries CANARY spare elements behind its last one that must stay untouched; scratch is NaN-filled.  The
oracle is never the HIP path itself."""
import ctypes
import json
import math
import os

import torch
import torch.nn.functional as F

import zerospeech_util as ZU
from phone_head_util import REDUCTION, oracle_ctc, oracle_full, oracle_head, ragged_targets
from seqnorm_util import LENGTH_RANGE, oracle as seqnorm_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 64
FILL = 7.0
H = 256
# one column; odd; % 4 == 0 and narrow; either side of 256; % 4 == 0 but % 16 != 0; the maximum
WIDTHS = (1, 13, 40, 255, 257, 260, 512)

# (B, S, C): one window; an uncovered tail; overlapping windows; several windows; a second class tile
HEAD_SHAPES = [(1, 8, 2), (2, 11, 7), (3, 12, 7), (2, 37, 41), (1, 77, 65)]
HEAD_CASES = [(D, 2, 11, 7) for D in WIDTHS] + [(D, 2, 37, 41) for D in WIDTHS] + \
    [(D, *s) for D in (13, 260) for s in HEAD_SHAPES if s not in ((2, 11, 7), (2, 37, 41))]

# (B, S) -> lengths: below, at and across the kernel's 32-frame step; n = S and n = 2 in every batch that has room for both
SEQNORM_SHAPES = {(1, 2): [2], (2, 31): [31, 2], (3, 33): [33, 20, 2], (2, 70): [70, 37]}

# (R, C); the last two are past the logits a tile keeps in LDS (384 classes): a second walk over the classes
POSTERIOR_SHAPES = [(1, 2), (33, 42), (70, 65), (33, 251), (130, 42), (5, 385), (40, 400)]


def P(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def buf(n, dev, fill=FILL, offset=0, dtype=torch.float32, canary=CANARY):
    """n + canary elements of ``fill``; for float32 the first one lies ``offset`` floats past a 16-byte boundary."""
    raw = torch.full((n + canary + 8,), fill, device=dev, dtype=dtype)
    skip = (-(raw.data_ptr() // raw.element_size())) % (16 // raw.element_size()) + offset
    return raw[skip:skip + n + canary]


def placed(t, dev, offset=0):
    """A dense copy of t on ``dev`` whose first element lies ``offset`` floats past a 16-byte boundary."""
    out = buf(t.numel(), dev, 0.0, offset, t.dtype, canary=0).view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * offset
    return out


def taken(b, n, nan=False):
    """The first n elements of an output buffer on the CPU, after its canaries were found untouched."""
    tail = b[n:].cpu()
    assert tail.numel() == CANARY
    assert bool(torch.isnan(tail).all()) if nan else bool((tail == FILL).all())
    return b[:n].cpu()


# ---------------------------------------------------------------------------------------------------------------- the head
def head_case(D, B, S, C):
    g = torch.Generator().manual_seed(1000003 + 10007 * D + 101 * S + 7 * B + C)
    x = torch.randn(B, S, D, generator=g)
    W = torch.randn(C, D, 8, generator=g) / math.sqrt(8 * D)
    b = 0.1 * torch.randn(C, generator=g)
    T = (S - 8) // 4 + 1
    dl = torch.randn(B, T, C, generator=g)
    return x, W, b, dl


def head_layout(lib, B, S, C, Lmax, D, entry="d"):
    sizes = (ctypes.c_long * 5)()
    if entry == "d":
        assert lib.cpc_phone_head_layout_d(B, S, C, Lmax, D, sizes) == 0
    else:
        assert D == H and lib.cpc_phone_head_layout(B, S, C, Lmax, sizes) == 0
    return tuple(sizes)


def run_head(lib, dev, x, W, b, dl=None, need_dx=True, entry="d"):
    """cpc_phone_head_forward_d (+ _backward_d with dl), or the 256 entry points -> dict of CPU tensors, canaries checked."""
    B, S, D = x.shape
    C = W.shape[0]
    T, wr_n, scr_n, lg_n, _ = head_layout(lib, B, S, C, 0, D, entry)
    x, W, b = x.contiguous().to(dev), W.contiguous().to(dev), b.to(dev)
    wr, logits = buf(wr_n, dev), buf(lg_n, dev)
    scratch = buf(scr_n, dev, float("nan"))
    tail = (D, None) if entry == "d" else (None,)
    fn = lib.cpc_phone_head_forward_d if entry == "d" else lib.cpc_phone_head_forward
    assert fn(P(x), P(W), P(b), P(wr), P(scratch), P(logits), B, S, C, *tail) == 0
    out = dict(T=T, wr=taken(wr, wr_n).view(C, 8, D), logits=taken(logits, lg_n).view(B, T, C))
    assert lg_n == B * T * C and wr_n == C * 8 * D
    if dl is not None:
        dl = dl.contiguous().to(dev)
        dW, db = buf(C * D * 8, dev), buf(C, dev)
        dX = buf(B * S * D, dev) if need_dx else None
        fn = lib.cpc_phone_head_backward_d if entry == "d" else lib.cpc_phone_head_backward
        assert fn(P(x), P(wr), P(dl), P(scratch), P(dW), P(db), P(dX), B, S, C, *tail) == 0
        out.update(dW=taken(dW, C * D * 8).view(C, D, 8), db=taken(db, C), dX=taken(dX, B * S * D).view(B, S, D) if need_dx else None)
    taken(scratch, scr_n, nan=True)
    taken(wr, wr_n)
    return out


def check_head(lib, dev, D, B, S, C):
    """Logits, dW, db and dX within 1e-5 (norm-relative) of F.conv1d in float64 and its autograd; exact zeros where no window
    reaches; the relaid weight; dX = NULL, a second call, and an utterance alone give the same bits."""
    x, W, b, dl = head_case(D, B, S, C)
    T = (S - 8) // 4 + 1
    out = run_head(lib, dev, x, W, b, dl)
    assert out["T"] == T
    logits, dW, db, dX = oracle_head(x, W, b, dl)
    errs = dict(logits=rel_err(out["logits"].double(), logits), dW=rel_err(out["dW"].double(), dW), db=rel_err(out["db"].double(), db),
                dX=rel_err(out["dX"].double(), dX))
    print(f"head D={D} B={B} S={S} C={C}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-5, (k, v)
    covered = 4 * (T - 1) + 8
    assert bool((out["dX"][:, covered:] == 0).all()) and bool((dX[:, covered:] == 0).all())
    assert bool((out["dX"][:, :covered] != 0).any())
    assert torch.equal(out["wr"], W.permute(0, 2, 1))
    again = run_head(lib, dev, x, W, b, dl)
    none = run_head(lib, dev, x, W, b, dl, need_dx=False)
    assert none["dX"] is None
    for k in ("logits", "dW", "db", "dX"):
        assert torch.equal(again[k], out[k]), k
    assert torch.equal(none["dW"], out["dW"]) and torch.equal(none["db"], out["db"])
    if B > 1:
        alone = run_head(lib, dev, x[:1], W, b, dl[:1])
        assert torch.equal(alone["logits"], out["logits"][:1]) and torch.equal(alone["dX"], out["dX"][:1])


def check_head_at_256(lib, dev, B, S, C):
    """The _d entry points at D = 256 give the bits of the 256 entry points on every output, and the same sizes."""
    x, W, b, dl = head_case(H, B, S, C)
    assert head_layout(lib, B, S, C, 5, H, "d") == head_layout(lib, B, S, C, 5, H, "256")
    wide, fixed = run_head(lib, dev, x, W, b, dl, entry="d"), run_head(lib, dev, x, W, b, dl, entry="256")
    for k in ("wr", "logits", "dW", "db", "dX"):
        assert torch.equal(wide[k], fixed[k]), k
    assert rel_err(wide["logits"].double(), oracle_head(x, W, b)) < 1e-5


def run_head_ctc(lib, dev, x, W, b, in_len, targets, tgt_len, blank, reduction):
    """Head, log-softmax and CTC forward and backward through the C ABI -> (loss, dW, db, dX) on the CPU."""
    B, S, D = x.shape
    C, Lmax, red = W.shape[0], targets.shape[1], REDUCTION[reduction]
    T, wr_n, scr_n, lg_n, saved_n = head_layout(lib, B, S, C, Lmax, D)
    x, W, b = x.contiguous().to(dev), W.contiguous().to(dev), b.to(dev)
    in_len, targets, tgt_len = in_len.to(dev), targets.contiguous().to(dev), tgt_len.to(dev)
    wr, logits, scratch = buf(wr_n, dev), buf(lg_n, dev), buf(scr_n, dev, float("nan"))
    assert lib.cpc_phone_head_forward_d(P(x), P(W), P(b), P(wr), P(scratch), P(logits), B, S, C, D, None) == 0
    saved = buf(saved_n, dev, float("nan"))
    n_loss = B if red == 0 else 1
    loss, dloss = buf(n_loss, dev), torch.ones(n_loss, device=dev)
    assert lib.cpc_ctc_seq_forward(P(logits), P(in_len), P(targets), targets.stride(0), P(tgt_len), P(saved), P(loss), B, T, C,
                                   Lmax, blank, red, None) == 0
    dl = buf(lg_n, dev)
    assert lib.cpc_ctc_seq_backward(P(logits), P(saved), P(dloss), P(dl), B, T, C, Lmax, blank, red, None) == 0
    dW, db, dX = buf(C * D * 8, dev), buf(C, dev), buf(B * S * D, dev)
    assert lib.cpc_phone_head_backward_d(P(x), P(wr), P(dl), P(scratch), P(dW), P(db), P(dX), B, S, C, D, None) == 0
    taken(scratch, scr_n, nan=True)
    return taken(loss, n_loss), taken(dW, C * D * 8).view(C, D, 8), taken(db, C), taken(dX, B * S * D).view(B, S, D)


def ragged_ctc_case(D=40, B=4, S=130, C=65):
    """(4, 130, 65): 31 windows, a second class tile, input lengths [T, T - 1, T // 2, 0] as tests/test_gpu_phone_head.py has
    them at 256 features."""
    x, W, b, _ = head_case(D, B, S, C)
    T = (S - 8) // 4 + 1
    targets, tgt_len = ragged_targets(B, 9, C - 1, seed=S + 1)
    in_len = torch.tensor([T, T - 1, T // 2, 0])
    return x, W, b, in_len, targets, tgt_len, C - 1


def check_ctc_results(got, x, W, b, in_len, targets, tgt_len, blank, reduction):
    """(loss, dW, db, dX) against float64 end to end: the loss 1e-5 relative, the gradients 1e-4 norm-relative."""
    rl, _, rdW, rdb, rdx = oracle_full(x, W, b, in_len, targets, tgt_len, blank, reduction)
    loss, dW, db, dX = got
    errs = dict(dW=rel_err(dW.double(), rdW), db=rel_err(db.double(), rdb), dX=rel_err(dX.double(), rdx))
    print("head + ctc: loss", loss.tolist(), "ref", rl.view(-1).tolist(), " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert bool(((loss.double().view(-1) - rl.view(-1)).abs() <= 1e-5 * rl.view(-1).abs()).all()), (loss, rl)
    for k, v in errs.items():
        assert v < 1e-4, (k, v)
    assert bool((dX[3] == 0).all()) and bool((rdx[3] == 0).all())          # in_len 0: no gradient reaches its frames


# -------------------------------------------------------------------------------------------------------------- seqNorm
def seqnorm_case(D, B, S):
    """x ~ N(0, 1), dy, and a scale in {0, 2} (Dropout2d at p = 0.5) with both.  No channel offset here: with n = 2 and a single
    channel (D = 1) one pair of frames is the whole case, and an offset of k spreads makes float32's rounding of x itself k times
    larger relative to x - m, whatever the code does.  What an offset asks of the variance is tested at 256 features
    (tests/test_emu_seqnorm.py: the offset cases), and check_seqnorm_columns shows that a column has those bits at every D."""
    g = torch.Generator().manual_seed(2000003 + 10007 * D + 101 * S + B)
    x = torch.randn(B, S, D, generator=g)
    dy = torch.randn(B, S, D, generator=g)
    scale = torch.empty(B, D).bernoulli_(0.5, generator=g).mul_(2)
    scale[:, 0] = 2.0
    if D > 1:
        scale[:, 1] = 0.0
    return x, dy, scale


def run_seqnorm(lib, dev, x, lengths, scale, normalise=True, dy=None, scalar=False, entry="d"):
    """cpc_seqnorm_forward_d (+ _backward_d with dy), or the 256 entry points -> dict of CPU tensors y, stats, dx; canaries
    checked.  scalar: x, y, dy and dx lie one float past a 16-byte boundary."""
    B, S, D = x.shape
    off = 1 if scalar else 0
    xd = placed(x, dev, off)
    ld = None if lengths is None else lengths.to(dev)
    sd = None if scale is None else scale.contiguous().to(dev)
    y, stats = buf(B * S * D, dev, offset=off), buf(B * 2 * D, dev)
    tail = (D,) if entry == "d" else ()
    assert entry == "d" or D == H
    fwd = lib.cpc_seqnorm_forward_d if entry == "d" else lib.cpc_seqnorm_forward
    assert fwd(P(xd), P(ld), P(sd), P(y), P(stats) if normalise else None, B, S, *tail, int(normalise), None) == 0
    out = dict(y=taken(y, B * S * D).view(B, S, D))
    if normalise:
        out["stats"] = taken(stats, B * 2 * D).view(B, 2, D)
    else:
        assert bool((stats.cpu() == FILL).all())
    if dy is not None:
        dyd = placed(dy, dev, off)
        dx = buf(B * S * D, dev, offset=off)
        bwd = lib.cpc_seqnorm_backward_d if entry == "d" else lib.cpc_seqnorm_backward
        assert bwd(P(xd) if normalise else None, P(dyd), P(ld), P(sd), P(stats) if normalise else None, P(dx), B, S, *tail,
                   int(normalise), None) == 0
        out["dx"] = taken(dx, B * S * D).view(B, S, D)
    assert torch.equal(xd.cpu(), x)                                        # the input is never written
    return out


def check_seqnorm(lib, dev, D, B, S, with_scale, normalise, scalar):
    """y within 1e-5 and dx within 1e-4 (norm-relative) of the float64 oracle; the statistics; the same bits on a second call and
    for an utterance alone.

    The gradient's denominator: where every utterance of the batch has n = 2 = S (the (1, 2) shape) the true gradient of the
    valid frames is O(eps = 1e-8) -- y is +-1/sqrt(2) whatever x is -- and float32 forms it as the difference of two terms of
    the size of r g.  A norm-relative error against that near-zero result measures rounding noise only (seqnorm_util.py says the
    same of its backward cases), so there the error is taken relative to the term before the cancellation, r g scale, which is
    what the float32 roundings are relative to.  Every other shape has an utterance with n >= 20 and uses the plain measure."""
    x, dy, scale = seqnorm_case(D, B, S)
    lengths = torch.tensor(SEQNORM_SHAPES[(B, S)], dtype=torch.long)
    scale = scale if with_scale else None
    got = run_seqnorm(lib, dev, x, lengths, scale, normalise, dy, scalar)
    ref = seqnorm_oracle(x, lengths, scale, normalise, dy)
    ey = rel_err(got["y"].double(), ref["y"])
    denom = ref["dx"]
    if normalise and min(SEQNORM_SHAPES[(B, S)]) == S == 2:
        denom = ref["r"][:, None, :] * dy.double() * (1.0 if scale is None else scale.double()[:, None, :])
    edx = ((got["dx"].double() - ref["dx"]).norm() / (denom.norm() + 1e-30)).item()
    print(f"seqnorm D={D} B={B} S={S} scale={with_scale} normalise={normalise} scalar={scalar}: y {ey:.2e} dx {edx:.2e}")
    assert ey < 1e-5 and edx < 1e-4
    if normalise:
        assert rel_err(got["stats"][:, 0].double(), ref["m"]) < 1e-5 and rel_err(got["stats"][:, 1].double(), ref["r"]) < 1e-5
    again = run_seqnorm(lib, dev, x, lengths, scale, normalise, dy, scalar)
    assert torch.equal(again["y"], got["y"]) and torch.equal(again["dx"], got["dx"])
    other = run_seqnorm(lib, dev, x, lengths, scale, normalise, dy, not scalar)     # either load path: the same bits
    assert torch.equal(other["y"], got["y"]) and torch.equal(other["dx"], got["dx"])
    if B > 1:
        alone = run_seqnorm(lib, dev, x[:1], lengths[:1], None if scale is None else scale[:1], normalise, dy[:1], scalar)
        assert torch.equal(alone["y"], got["y"][:1]) and torch.equal(alone["dx"], got["dx"][:1])


def check_seqnorm_columns(lib, dev, D, B, S, scalar):
    """Column c of a D-wide call has the bits of the same column in a 256-wide call (cpc_seqnorm_forward / _backward) on the same
    data, zero-extended: the columns from 0 on and, above 256 features, the columns of the last -- partial -- slab."""
    x, dy, scale = seqnorm_case(D, B, S)
    lengths = torch.tensor(SEQNORM_SHAPES[(B, S)], dtype=torch.long)
    got = run_seqnorm(lib, dev, x, lengths, scale, True, dy, scalar)
    last = (D - 1) // 64 * 64
    for lo in sorted({0, last if D > H else 0}):
        n = min(D - lo, H)

        def ext(t):
            out = torch.zeros(*t.shape[:-1], H)
            out[..., :n] = t[..., lo:lo + n]
            return out

        ref = run_seqnorm(lib, dev, ext(x), lengths, ext(scale), True, ext(dy), False, entry="256")
        for k in ("y", "dx", "stats"):
            assert torch.equal(got[k][..., lo:lo + n], ref[k][..., :n]), (k, lo)


def check_seqnorm_at_256(lib, dev, B, S, scalar):
    x, dy, scale = seqnorm_case(H, B, S)
    lengths = torch.tensor(SEQNORM_SHAPES[(B, S)], dtype=torch.long)
    for normalise in (True, False):
        wide = run_seqnorm(lib, dev, x, lengths, scale, normalise, dy, scalar, entry="d")
        fixed = run_seqnorm(lib, dev, x, lengths, scale, normalise, dy, scalar, entry="256")
        for k in wide:
            assert torch.equal(wide[k], fixed[k]), (k, normalise)


def check_seqnorm_lengths(lib, dev, D):
    """n = 1: NaN for that utterance only.  A length past S: flagged once, clamped."""
    B, S = 2, 31
    x, dy, scale = seqnorm_case(D, B, S)
    lib.cpc_device_error_flags(1)                                          # (whatever an earlier test left behind)
    good = run_seqnorm(lib, dev, x, torch.tensor([31, 2]), scale, True, dy)
    assert lib.cpc_device_error_flags(1) == 0
    one = run_seqnorm(lib, dev, x, torch.tensor([31, 1]), scale, True, dy)
    assert bool(torch.isnan(one["y"][1]).all()) and bool(torch.isnan(one["dx"][1]).all())
    assert torch.equal(one["y"][0], good["y"][0]) and torch.equal(one["dx"][0], good["dx"][0])
    assert lib.cpc_device_error_flags(1) == 0                              # n < 2 is no error
    past = run_seqnorm(lib, dev, x, torch.tensor([32, 2]), scale, True, None)
    assert lib.cpc_device_error_flags(1) == LENGTH_RANGE and lib.cpc_device_error_flags(1) == 0
    assert torch.equal(past["y"], good["y"])


# ------------------------------------------------------------------------------------------------------------ posteriors
_posterior = {}


def f32_dev():
    with open(os.path.join(ROOT, "tests", "golden", "zerospeech_meta.json")) as f:
        return json.load(f)["f32_dev"]


def posterior_case(D, R, C):
    """Seeded inputs and their float64 logits, computed once per case and left unchanged."""
    if (D, R, C) not in _posterior:
        g = torch.Generator().manual_seed(3000009 + 100000 * D + 3000 * R + C)
        x = torch.randn(R, D, generator=g)
        W = (2 * torch.rand(C, D, generator=g) - 1) / math.sqrt(D)
        b = (2 * torch.rand(C, generator=g) - 1) / 16
        _posterior[(D, R, C)] = (x, W, b, F.linear(x.double(), W.double(), b.double()))
    return _posterior[(D, R, C)]


def run_posterior(lib, dev, x, W, b, mode, layout="dense", entry="d", with_argmax=True):
    """cpc_posterior_forward_d (or the 256 entry point) -> (out (R, C), argmax (R)) on the CPU, canaries checked.  layout: dense;
    'stride': rows D + 4 floats apart with NaNs in between, read in place; 'offset1': the rows start one float past a 16-byte boundary."""
    R, D = x.shape
    C = W.shape[0]
    if layout == "stride":
        owner = torch.full((R, D + 4), float("nan"))
        owner[:, :D] = x
        owner = owner.to(dev)
        xv, ldx = owner[:, :D], D + 4
    else:
        xv, ldx = placed(x, dev, 1 if layout == "offset1" else 0), D
    W, b = W.contiguous().to(dev), b.to(dev)
    out = buf(R * C, dev, 7, dtype=torch.float32 if mode == 0 else torch.int64)
    am = buf(R, dev, 7, dtype=torch.int32)
    tail = (D,) if entry == "d" else ()
    assert entry == "d" or D == H
    fn = lib.cpc_posterior_forward_d if entry == "d" else lib.cpc_posterior_forward
    assert fn(xv.data_ptr(), ldx, P(W), P(b), R, C, *tail, mode, P(out), P(am) if with_argmax else None, None) == 0
    if not with_argmax:
        assert bool((am.cpu() == 7).all())
        return taken(out, R * C).view(R, C), None
    return taken(out, R * C).view(R, C), taken(am, R)


def check_posterior(lib, dev, D, R, C):
    """Softmax within 4 x f32_dev of float64 (tests/golden/zerospeech_meta.json: what torch's own float32 run deviates, the bar of
    tests/test_gpu_posterior.py), row sums within 1e-6, one-hot and argmax exact -- after the float64 logits were found to have
    no row whose top-2 margin is under 1e-4 of its scale, which is a condition on the case, not a tolerance."""
    x, W, b, logits = posterior_case(D, R, C)
    assert ZU.close_rows(logits) == 0
    post, am0 = run_posterior(lib, dev, x, W, b, 0)
    ref = torch.softmax(logits, dim=1)
    err = (post.double() - ref).abs().max().item()
    row_sum = (post.double().sum(dim=1) - 1).abs().max().item()
    print(f"posterior D={D} R={R} C={C}: max abs err {err:.3e} (bound {4 * f32_dev():.3e}), max |row sum - 1| {row_sum:.3e}")
    assert not torch.isnan(post).any()
    assert err <= 4 * f32_dev()
    assert row_sum <= 1e-6
    hot, am1 = run_posterior(lib, dev, x, W, b, 1)
    arg = logits.argmax(dim=1)
    assert hot.dtype == torch.int64 and torch.equal(hot, F.one_hot(arg, C))
    assert torch.equal(am0.long(), arg) and torch.equal(am1, am0)
    again, _ = run_posterior(lib, dev, x, W, b, 0, with_argmax=False)
    assert torch.equal(again, post)
    for layout in ("stride", "offset1"):                   # read in place behind a wider row; scalar loads
        moved, am2 = run_posterior(lib, dev, x, W, b, 0, layout=layout)
        assert torch.equal(moved, post) and torch.equal(am2, am0), layout
    if R > 33:                                             # split at a row that is no multiple of the 32-row tile
        head, _ = run_posterior(lib, dev, x[:33], W, b, 0)
        rest, _ = run_posterior(lib, dev, x[33:], W, b, 0)
        assert torch.equal(torch.cat([head, rest]), post)


def check_posterior_zero_columns(lib, dev, R, C):
    """D = 13 gives the bits of D = 16 with three zero columns appended to x and W."""
    x, W, b, _ = posterior_case(13, R, C)
    x16, W16 = torch.zeros(R, 16), torch.zeros(C, 16)
    x16[:, :13], W16[:, :13] = x, W
    for mode in (0, 1):
        a, am_a = run_posterior(lib, dev, x, W, b, mode)
        c, am_c = run_posterior(lib, dev, x16, W16, b, mode)
        assert torch.equal(a, c) and torch.equal(am_a, am_c)


def check_posterior_at_256(lib, dev, R, C):
    x, W, b, _ = posterior_case(H, R, C)
    for mode in (0, 1):
        for layout in ("dense", "offset1"):
            a, am_a = run_posterior(lib, dev, x, W, b, mode, layout, entry="d")
            c, am_c = run_posterior(lib, dev, x, W, b, mode, layout, entry="256")
            assert torch.equal(a, c) and torch.equal(am_a, am_c), (mode, layout)
