"""The fused probe step and the supervised criteria at any feature width (cpc_probe_*_d, cpc_classifier_*_d, cpc_ctc_forward_d)
through the C ABI against torch in float64 on the CPU: cases and checks shared by tests/test_emu_probe_widths.py (host emulator)
and tests/test_gpu_probe_widths.py (MI355X).  ``lib`` is the bound library, ``device`` where its buffers live.

Bounds (those of test_emu_probe.py / test_emu_supervised.py): loss within 1e-5 relative; dW, db and dX within 1e-5 relative norm
(1e-4 behind the CTC loss, as there); accuracy equal to the float64 one -- the seeds below leave no row with a top-2 margin under
1e-5 of its scale, which every check asserts."""
import ctypes
import math

import torch
import torch.nn.functional as F

LABEL_RANGE = 16     # CPC_DEVERR_LABEL_RANGE
LR, BETA1, BETA2, EPS = 2e-4, 0.9, 0.999, 2e-8
CANARY = 64

# (D, R, C): odd and scalar-loaded; vector-loaded with three tiles and two class steps; one column past the 256 block in the
# 32-class step; D % 4 == 0 above 256 on the speaker probe's shape; the maximum with three class steps; the smallest call; the
# last width of the 64-class step
CASES = [(13, 33, 41), (40, 70, 65), (257, 33, 41), (260, 8, 251), (512, 33, 130), (1, 1, 2), (255, 33, 41)]
# the speaker layout read in place (row pitch 3 D: scalar loads at 13, 16-byte loads at 40) and x one float past a 16-byte boundary
LAYOUTS = {"speaker13": (13, 8, 12, 3 * 13, 2 * 13), "speaker40": (40, 8, 12, 120, 80), "offset40": (40, 33, 41, 40, 1)}


def P(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bias_corrections(step):
    return 1.0 - BETA1 ** step, math.sqrt(1.0 - BETA2 ** step)


class Case:
    """R rows of D features at pitch ``ldx`` starting ``off`` floats into a dense buffer, a (C, D) classifier and labels."""

    def __init__(self, D, R, C, seed, ldx=None, off=0):
        g = torch.Generator().manual_seed(seed)
        self.D, self.R, self.C, self.ldx, self.off = D, R, C, (D if ldx is None else ldx), off
        self.base = torch.randn(off + (R - 1) * self.ldx + D, generator=g)
        self.W = 0.1 * torch.randn(C, D, generator=g)
        self.b = 0.1 * torch.randn(C, generator=g)
        self.y = torch.randint(0, C, (R,), generator=g)
        self.moments = (1e-3 * torch.randn(C, D, generator=g), 1e-6 * torch.rand(C, D, generator=g),
                        1e-3 * torch.randn(C, generator=g), 1e-6 * torch.rand(C, generator=g))

    @property
    def x(self):
        return self.base.as_strided((self.R, self.D), (self.ldx, 1), self.off)

    def on(self, device):
        """(the base buffer on the device -- keep it alive --, the address of x's first row)"""
        base = self.base.to(device)
        assert base.data_ptr() % 16 == 0
        return base, base.data_ptr() + 4 * self.off


def padded(t, device, fill=7.0):
    out = torch.full((t.numel() + CANARY,), fill, dtype=t.dtype)
    out[:t.numel()] = t.reshape(-1)
    return out.to(device)


def probe_layout(lib, R, C, D=None):
    sizes = (ctypes.c_long * 3)()
    assert (lib.cpc_probe_layout(R, C, sizes) if D is None else lib.cpc_probe_layout_d(R, C, D, sizes)) == 0
    return tuple(sizes)


def train(lib, case, device="cpu", step=3, accum=None, export=True, old_entry=False, W=None, b=None, moments=None):
    """cpc_probe_train_step_d (``old_entry``: cpc_probe_train_step, D = 256) on a workspace full of NaN, every buffer with
    CANARY spare elements behind it.  -> the buffers, on the CPU."""
    R, C, D = case.R, case.C, case.D
    W, b, moments = (case.W if W is None else W), (case.b if b is None else b), (case.moments if moments is None else moments)
    ws_n = probe_layout(lib, R, C, None if old_entry else D)[0]
    base, x_ptr = case.on(device)
    y = case.y.to(device)
    buf = {"W": padded(W, device), "b": padded(b, device), "mW": padded(moments[0], device), "vW": padded(moments[1], device),
           "mb": padded(moments[2], device), "vb": padded(moments[3], device),
           "ws": torch.full((ws_n + CANARY,), float("nan"), device=device), "loss": torch.full((1 + CANARY,), 7.0, device=device),
           "acc": torch.full((1 + CANARY,), 7.0, dtype=torch.float64, device=device),
           "accum": (torch.tensor([0.0, 0.0] + [7.0] * CANARY, dtype=torch.float64) if accum is None else accum).to(device),
           "dW": torch.full((C * D + CANARY,), 7.0, device=device) if export else None,
           "db": torch.full((C + CANARY,), 7.0, device=device) if export else None}
    bc1, bc2s = bias_corrections(step)
    tail = (P(buf["W"]), P(buf["b"]), P(buf["mW"]), P(buf["vW"]), P(buf["mb"]), P(buf["vb"]), LR, BETA1, BETA2, EPS, bc1, bc2s,
            P(buf["ws"]), P(buf["loss"]), P(buf["acc"]), P(buf["accum"]), P(buf["dW"]), P(buf["db"]), None)
    if old_entry:
        assert D == 256 and lib.cpc_probe_train_step(x_ptr, case.ldx, P(y), R, C, *tail) == 0
    else:
        assert lib.cpc_probe_train_step_d(x_ptr, case.ldx, P(y), R, C, D, *tail) == 0
    out = {k: (None if v is None else v.cpu()) for k, v in buf.items()}
    out["ws_n"] = ws_n
    return out


def evaluate(lib, case, device="cpu", accum=None, old_entry=False, W=None, b=None):
    R, C, D = case.R, case.C, case.D
    W, b = (case.W if W is None else W), (case.b if b is None else b)
    ws_n = probe_layout(lib, R, C, None if old_entry else D)[0]
    base, x_ptr = case.on(device)
    y, Wd, bd = case.y.to(device), W.contiguous().to(device), b.to(device)
    buf = {"ws": torch.full((ws_n + CANARY,), float("nan"), device=device), "loss": torch.full((1 + CANARY,), 7.0, device=device),
           "acc": torch.full((1 + CANARY,), 7.0, dtype=torch.float64, device=device),
           "accum": (torch.tensor([0.0, 0.0] + [7.0] * CANARY, dtype=torch.float64) if accum is None else accum).to(device)}
    tail = (P(Wd), P(bd), P(buf["ws"]), P(buf["loss"]), P(buf["acc"]), P(buf["accum"]), None)
    if old_entry:
        assert D == 256 and lib.cpc_probe_eval(x_ptr, case.ldx, P(y), R, C, *tail) == 0
    else:
        assert lib.cpc_probe_eval_d(x_ptr, case.ldx, P(y), R, C, D, *tail) == 0
    out = {k: v.cpu() for k, v in buf.items()}
    out["ws_n"] = ws_n
    return out


def oracle(x, W, b, y):
    xr, Wr, br = (t.double().clone().requires_grad_(True) for t in (x, W, b))
    logits = F.linear(xr, Wr, br)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return loss.detach(), logits.detach(), Wr.grad, br.grad, xr.grad


def close_rows(logits):
    """Rows whose top-2 margin is under 1e-5 of the row's scale: the float32 argmax may differ there."""
    top2 = logits.topk(2, dim=1).values
    scale = logits.abs().max(dim=1).values.clamp_min(1e-30)
    return int(((top2[:, 0] - top2[:, 1]) < 1e-5 * scale).sum())


def check_against_float64(out, case, what=""):
    C, D = case.C, case.D
    loss, logits, dW, db, _ = oracle(case.x, case.W, case.b, case.y)
    acc = (logits.argmax(dim=1) == case.y).double().mean().item()
    errs = dict(loss=abs(out["loss"][0].item() - loss.item()) / abs(loss.item()), acc=abs(out["acc"][0].item() - acc))
    if out.get("dW") is not None:
        errs["dW"] = rel_err(out["dW"][:C * D].double().view(C, D), dW)
        errs["db"] = rel_err(out["db"][:C].double(), db)
    print(f"probe {what} D={D} R={case.R} C={C} ldx={case.ldx} off={case.off}: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert close_rows(logits) == 0                        # (the seeds were chosen so: the accuracy compares exactly)
    assert errs["loss"] <= 1e-5
    assert out["acc"][0].item() == acc
    assert errs.get("dW", 0.0) < 1e-5 and errs.get("db", 0.0) < 1e-5


def adam_reference(lib, case, dW, db, step, device):
    """cpc_adam_step on copies of the same state, from the gradients the probe step exported."""
    ps = [case.W.clone().reshape(-1).to(device), case.b.clone().to(device)]
    gs = [dW.clone().to(device), db.clone().to(device)]
    ms = [case.moments[0].clone().reshape(-1).to(device), case.moments[2].clone().to(device)]
    vs = [case.moments[1].clone().reshape(-1).to(device), case.moments[3].clone().to(device)]
    arr = ctypes.c_void_p * 2
    ns = (ctypes.c_long * 2)(ps[0].numel(), ps[1].numel())
    bc1, bc2s = bias_corrections(step)
    assert lib.cpc_adam_step(arr(*[P(t) for t in ps]), arr(*[P(t) for t in gs]), arr(*[P(t) for t in ms]),
                             arr(*[P(t) for t in vs]), ns, 2, LR, BETA1, BETA2, EPS, bc1, bc2s, None) == 0
    return [t.cpu() for t in ps], [t.cpu() for t in ms], [t.cpu() for t in vs]


def check_canaries(buf, C, D):
    for k, n in (("W", C * D), ("b", C), ("mW", C * D), ("vW", C * D), ("mb", C), ("vb", C), ("loss", 1), ("acc", 1), ("accum", 2),
                 ("dW", C * D), ("db", C)):
        if buf.get(k) is not None:
            assert buf[k].numel() == n + CANARY and bool((buf[k][n:] == 7.0).all()), k
    assert buf["ws"].numel() == buf["ws_n"] + CANARY and bool(torch.isnan(buf["ws"][buf["ws_n"]:]).all())


BITS = ("loss", "acc", "accum", "W", "b", "mW", "vW", "mb", "vb", "dW", "db")


def check_probe_case(lib, case, device="cpu"):
    """Train step, eval and accum against float64; the exported gradients; the update as cpc_adam_step makes it from them, bit
    for bit; canaries; identical calls give identical bits; no device error."""
    C, D = case.C, case.D
    lib.cpc_device_error_flags(1)
    out = train(lib, case, device, step=3)
    check_against_float64(out, case, "train")
    ps, ms, vs = adam_reference(lib, case, out["dW"][:C * D], out["db"][:C], 3, device)
    assert torch.equal(out["W"][:C * D], ps[0]) and torch.equal(out["b"][:C], ps[1])
    assert torch.equal(out["mW"][:C * D], ms[0]) and torch.equal(out["mb"][:C], ms[1])
    assert torch.equal(out["vW"][:C * D], vs[0]) and torch.equal(out["vb"][:C], vs[1])
    assert not torch.equal(out["W"][:C * D], case.W.reshape(-1))
    check_canaries(out, C, D)
    assert out["accum"][0].item() == float(out["loss"][0]) and out["accum"][1].item() == out["acc"][0].item()
    again = train(lib, case, device, step=3)
    for k in BITS:
        assert torch.equal(out[k], again[k]), k
    bare = train(lib, case, device, step=3, export=False)               # without the optional gradient outputs: the same update
    for k in ("loss", "acc", "W", "b", "mW", "vW", "mb", "vb"):
        assert torch.equal(bare[k], out[k]), k
    accum = out["accum"].clone()
    ev = evaluate(lib, case, device, accum=accum)
    check_against_float64(ev, case, "eval")
    assert torch.equal(ev["loss"][:1], out["loss"][:1]) and torch.equal(ev["acc"][:1], out["acc"][:1])
    assert ev["accum"][0].item() == float(out["loss"][0]) + float(ev["loss"][0])
    assert ev["accum"][1].item() == out["acc"][0].item() + ev["acc"][0].item()
    check_canaries(ev, C, D)
    assert torch.equal(evaluate(lib, case, device, accum=accum)["loss"], ev["loss"])
    assert lib.cpc_device_error_flags(1) == 0


def check_d256_gives_the_bits_of_the_256_entry_points(lib, device="cpu"):
    """The probe at (R, C) with one and with three class steps, the classifier forward and backward: the _d calls at D = 256 and
    the existing calls on the same inputs -- loss, acc, W, b, moments, dW, db and dX."""
    for R, C, seed in ((70, 41, 61), (70, 130, 62)):
        case = Case(256, R, C, seed)
        assert probe_layout(lib, R, C, 256) == probe_layout(lib, R, C)
        new, old = train(lib, case, device), train(lib, case, device, old_entry=True)
        for k in BITS:
            assert torch.equal(new[k], old[k]), (C, k)
        e_new, e_old = evaluate(lib, case, device), evaluate(lib, case, device, old_entry=True)
        assert torch.equal(e_new["loss"], e_old["loss"]) and torch.equal(e_new["acc"], e_old["acc"])
        c_new, c_old = classifier(lib, case, device), classifier(lib, case, device, old_entry=True)
        for k in ("loss", "acc", "dW", "db", "dX"):
            assert torch.equal(c_new[k], c_old[k]), (C, k)


# ---------------------------------------------------------------------------------------- classifier and CTC criterion
def supervised_layout(lib, B, S, C, D, ctc, old_entry=False):
    sizes = (ctypes.c_long * 3)()
    rc = lib.cpc_supervised_layout(B, S, C, ctc, sizes) if old_entry else lib.cpc_supervised_layout_d(B, S, C, D, ctc, sizes)
    assert rc == 0
    return tuple(sizes)


def classifier(lib, case, device="cpu", dlogits=None, old_entry=False):
    """cpc_classifier_forward_d + _backward_d (dloss = 1) with dX; with ``dlogits`` the backward alone on the caller's dlogits."""
    R, C, D = case.R, case.C, case.D
    saved_n, scr_n, _ = supervised_layout(lib, R, 1, C, D, 0, old_entry)
    base, x_ptr = case.on(device)
    W, b, y = case.W.to(device), case.b.to(device), case.y.to(device)
    saved = torch.full((saved_n + CANARY,), float("nan"), device=device)
    scratch = torch.full((scr_n + CANARY,), float("nan"), device=device)
    loss = torch.full((1 + CANARY,), 7.0, device=device)
    acc = torch.full((1 + CANARY,), 7.0, dtype=torch.float64, device=device)
    dloss = torch.ones(1, device=device)
    dl = None if dlogits is None else dlogits.contiguous().to(device)
    extra = () if old_entry else (D,)
    if dl is None:
        fwd = lib.cpc_classifier_forward if old_entry else lib.cpc_classifier_forward_d
        assert fwd(x_ptr, case.ldx, P(W), P(b), P(y), P(saved), P(loss), P(acc), R, C, *extra, None) == 0
    dW = torch.full((C * D + CANARY,), 7.0, device=device)
    db = torch.full((C + CANARY,), 7.0, device=device)
    dX = torch.full((R * D + CANARY,), 7.0, device=device)
    bwd = lib.cpc_classifier_backward if old_entry else lib.cpc_classifier_backward_d
    assert bwd(x_ptr, case.ldx, P(W), P(y), P(saved), P(dloss), P(dl), P(scratch), P(dW), P(db), P(dX), R, C, *extra, None) == 0
    out = dict(loss=loss, acc=acc, dW=dW, db=db, dX=dX, saved=saved, scratch=scratch)
    out = {k: v.cpu() for k, v in out.items()}
    for k, n in (("loss", 1), ("acc", 1), ("dW", C * D), ("db", C), ("dX", R * D)):
        if dl is None or k not in ("loss", "acc"):
            assert bool((out[k][n:] == 7.0).all()), k
    assert bool(torch.isnan(out["saved"][saved_n:]).all()) and bool(torch.isnan(out["scratch"][scr_n:]).all())
    return out


def check_classifier_case(lib, D, device="cpu", R=70, C=65):
    """Forward, dW, db and dX against float64; then the backward alone on caller-supplied dlogits against the same products."""
    lib.cpc_device_error_flags(1)
    case = Case(D, R, C, seed=100 + D)
    out = classifier(lib, case, device)
    loss, logits, dW, db, dx = oracle(case.x, case.W, case.b, case.y)
    errs = dict(loss=abs(out["loss"][0].item() - loss.item()) / abs(loss.item()), dW=rel_err(out["dW"][:C * D].double().view(C, D), dW),
                db=rel_err(out["db"][:C].double(), db), dX=rel_err(out["dX"][:R * D].double().view(R, D), dx))
    print(f"classifier D={D} on {device}: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert close_rows(logits) == 0
    assert errs["loss"] <= 1e-5 and errs["dW"] < 1e-5 and errs["db"] < 1e-5 and errs["dX"] < 1e-5
    assert out["acc"][0].item() == (logits.argmax(dim=1) == case.y).double().mean().item()
    dl = torch.randn(R, C, generator=torch.Generator().manual_seed(D)) / R
    given = classifier(lib, case, device, dlogits=dl)
    d64 = dl.double()
    assert rel_err(given["dW"][:C * D].double().view(C, D), d64.t() @ case.x.double()) < 1e-5
    assert rel_err(given["db"][:C].double(), d64.sum(0)) < 1e-5
    assert rel_err(given["dX"][:R * D].double().view(R, D), d64 @ case.W.double()) < 1e-5
    assert lib.cpc_device_error_flags(1) == 0


def ctc_oracle(x, W, b, labels):
    xr, Wr, br = (t.double().clone().requires_grad_(True) for t in (x, W, b))
    Bq, S, _ = x.shape
    logits = F.linear(xr, Wr, br)
    logits.retain_grad()
    lp = F.log_softmax(logits, dim=2).permute(1, 0, 2)
    keep = torch.ones_like(labels, dtype=torch.bool)
    keep[:, 1:] = labels[:, 1:] != labels[:, :-1]
    loss = F.ctc_loss(lp, labels[keep], torch.full((Bq,), S, dtype=torch.long), keep.sum(1), blank=W.shape[0] - 1,
                      reduction="mean", zero_infinity=True)
    loss.backward()
    return loss.detach(), logits.grad.reshape(Bq * S, -1), Wr.grad, br.grad, xr.grad


def check_ctc_case(lib, D, device="cpu", Bq=4, S=16, n_phones=41):
    """cpc_ctc_forward_d, cpc_ctc_backward (one call for every width) and cpc_classifier_backward_d on its dlogits against
    torch's float64 CTC: loss 1e-5, gradients 1e-4 (test_emu_supervised.py's bounds for this path)."""
    lib.cpc_device_error_flags(1)
    C = n_phones + 1
    g = torch.Generator().manual_seed(200 + D)
    case = Case(D, Bq * S, C, seed=300 + D)
    labels = torch.randint(0, n_phones, (Bq, S // 2), generator=g).repeat_interleave(2, dim=1)      # runs of two frames
    saved_n, _, dl_n = supervised_layout(lib, Bq, S, C, D, 1)
    assert dl_n == Bq * S * C
    base, x_ptr = case.on(device)
    W, b, lab = case.W.to(device), case.b.to(device), labels.to(device)
    saved = torch.full((saved_n + CANARY,), float("nan"), device=device)
    loss = torch.full((1 + CANARY,), 7.0, device=device)
    assert lib.cpc_ctc_forward_d(x_ptr, P(W), P(b), P(lab), P(saved), P(loss), Bq, S, C, D, None) == 0
    dl = torch.full((dl_n + CANARY,), 7.0, device=device)
    dloss = torch.ones(1, device=device)
    assert lib.cpc_ctc_backward(P(saved), P(dloss), P(dl), Bq, S, C, None) == 0
    loss, dl, saved = loss.cpu(), dl.cpu(), saved.cpu()
    out = classifier(lib, case, device, dlogits=dl[:dl_n].view(Bq * S, C))
    rl, rdl, rdW, rdb, rdx = ctc_oracle(case.x.view(Bq, S, D), case.W, case.b, labels)
    errs = dict(loss=abs(loss[0].item() - rl.item()) / abs(rl.item()), dlogits=rel_err(dl[:dl_n].double().view_as(rdl), rdl),
                dW=rel_err(out["dW"][:C * D].double().view_as(rdW), rdW), db=rel_err(out["db"][:C].double(), rdb),
                dX=rel_err(out["dX"][:Bq * S * D].double().view_as(rdx), rdx))
    print(f"CTC D={D} on {device}: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert errs["loss"] <= 1e-5
    assert errs["dlogits"] < 1e-4 and errs["dW"] < 1e-4 and errs["db"] < 1e-4 and errs["dX"] < 1e-4
    assert bool((loss[1:] == 7.0).all()) and bool((dl[dl_n:] == 7.0).all()) and bool(torch.isnan(saved[saved_n:]).all())
    assert lib.cpc_device_error_flags(1) == 0
