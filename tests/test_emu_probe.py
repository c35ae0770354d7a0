"""The fused probe step (csrc/probe.hip: cpc_probe_train_step / cpc_probe_eval) on the host SIMT emulator against torch in
float64 on the CPU.  Bounds are those of test_emu_supervised.py: loss within 1e-5 relative, gradients within 1e-5 relative norm,
accuracy exact except on rows whose top-2 margin is under 1e-5 of the row's scale."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from emu_util import P, emu, rel_err

H = 256
LABEL_RANGE = 16     # CPC_DEVERR_LABEL_RANGE
LR, BETA1, BETA2, EPS = 2e-4, 0.9, 0.999, 2e-8
CANARY = 64


def _layout(lib, R, C):
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_probe_layout(R, C, sizes) == 0
    return tuple(sizes)


def _bias_corrections(step):
    return 1.0 - BETA1 ** step, math.sqrt(1.0 - BETA2 ** step)


def _case(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, H, generator=g)
    W = 0.1 * torch.randn(C, H, generator=g)
    b = 0.1 * torch.randn(C, generator=g)
    y = torch.randint(0, C, (R,), generator=g)
    return x, W, b, y


def _moments(C, seed):
    """Moments as after some earlier steps: the update is checked from a state that is not all zeros."""
    g = torch.Generator().manual_seed(seed)
    return (1e-3 * torch.randn(C, H, generator=g), 1e-6 * torch.rand(C, H, generator=g),
            1e-3 * torch.randn(C, generator=g), 1e-6 * torch.rand(C, generator=g))


def _padded(t, fill=7.0):
    out = torch.full((t.numel() + CANARY,), fill, dtype=t.dtype)
    out[:t.numel()] = t.reshape(-1)
    return out


def _train(lib, x, ldx, W, b, y, moments, step=3, accum=None, export=True):
    R, C = y.numel(), W.shape[0]
    ws_n = _layout(lib, R, C)[0]
    buf = {"W": _padded(W), "b": _padded(b), "mW": _padded(moments[0]), "vW": _padded(moments[1]), "mb": _padded(moments[2]),
           "vb": _padded(moments[3]), "ws": torch.full((ws_n + CANARY,), float("nan")), "loss": torch.full((1 + CANARY,), 7.0),
           "acc": torch.full((1 + CANARY,), 7.0, dtype=torch.float64),
           "accum": torch.full((2 + CANARY,), 7.0, dtype=torch.float64) if accum is None else accum,
           "dW": torch.full((C * H + CANARY,), 7.0) if export else None, "db": torch.full((C + CANARY,), 7.0) if export else None}
    if accum is None:
        buf["accum"][:2] = 0
    bc1, bc2s = _bias_corrections(step)
    rc = lib.cpc_probe_train_step(x.data_ptr(), ldx, P(y), R, C, P(buf["W"]), P(buf["b"]), P(buf["mW"]), P(buf["vW"]), P(buf["mb"]),
                                  P(buf["vb"]), LR, BETA1, BETA2, EPS, bc1, bc2s, P(buf["ws"]), P(buf["loss"]), P(buf["acc"]),
                                  P(buf["accum"]), P(buf["dW"]), P(buf["db"]), None)
    assert rc == 0
    buf["ws_n"] = ws_n
    return buf


def _eval(lib, x, ldx, W, b, y, accum=None):
    R, C = y.numel(), W.shape[0]
    ws_n = _layout(lib, R, C)[0]
    buf = {"ws": torch.full((ws_n + CANARY,), float("nan")), "loss": torch.full((1 + CANARY,), 7.0),
           "acc": torch.full((1 + CANARY,), 7.0, dtype=torch.float64),
           "accum": torch.full((2 + CANARY,), 7.0, dtype=torch.float64) if accum is None else accum}
    if accum is None:
        buf["accum"][:2] = 0
    assert lib.cpc_probe_eval(x.data_ptr(), ldx, P(y), R, C, P(W), P(b), P(buf["ws"]), P(buf["loss"]), P(buf["acc"]),
                              P(buf["accum"]), None) == 0
    buf["ws_n"] = ws_n
    return buf


def _oracle(x, W, b, y):
    Wr, br = W.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    logits = F.linear(x.double(), Wr, br)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return loss.detach(), logits.detach(), Wr.grad, br.grad


def _check_acc(acc, logits, y):
    """test_emu_supervised.py's rule: exactly the float64 accuracy, except that rows whose top-2 margin is under 1e-5 of the
    row's scale may differ."""
    top2 = logits.topk(2, dim=1).values
    scale = logits.abs().max(dim=1).values.clamp_min(1e-30)
    close = (top2[:, 0] - top2[:, 1]) < 1e-5 * scale
    hit = (logits.argmax(dim=1) == y)
    lo = (hit & ~close).sum().item() / y.numel()
    hi = (hit | close).sum().item() / y.numel()
    assert lo - 1e-15 <= acc <= hi + 1e-15, (acc, lo, hi, int(close.sum()))
    if not close.any():
        assert acc == hit.double().mean().item()


def _adam_reference(lib, W, b, moments, dW, db, step):
    """cpc_adam_step on copies of the same state, from the gradients the probe step exported."""
    ps = [W.clone().reshape(-1), b.clone()]
    gs = [dW.clone(), db.clone()]
    ms = [moments[0].clone().reshape(-1), moments[2].clone()]
    vs = [moments[1].clone().reshape(-1), moments[3].clone()]
    arr = ctypes.c_void_p * 2
    ns = (ctypes.c_long * 2)(ps[0].numel(), ps[1].numel())
    bc1, bc2s = _bias_corrections(step)
    assert lib.cpc_adam_step(arr(*[P(t) for t in ps]), arr(*[P(t) for t in gs]), arr(*[P(t) for t in ms]),
                             arr(*[P(t) for t in vs]), ns, 2, LR, BETA1, BETA2, EPS, bc1, bc2s, None) == 0
    return ps, ms, vs


def _check_canaries(buf, C):
    for k, n in (("W", C * H), ("b", C), ("mW", C * H), ("vW", C * H), ("mb", C), ("vb", C), ("loss", 1), ("acc", 1), ("accum", 2),
                 ("dW", C * H), ("db", C)):
        if buf.get(k) is not None:
            assert bool((buf[k][n:] == 7.0).all()), k
    assert torch.isnan(buf["ws"][buf["ws_n"]:]).all()


@pytest.mark.parametrize("R,C", [(512, 41), (300, 300), (77, 2), (1, 5), (16, 2049)])
def test_probe_train_and_eval_match_torch_float64_emulated(R, C):
    lib = emu()
    lib.cpc_device_error_flags(1)
    x, W, b, y = _case(R, C, seed=R + C)
    moments = _moments(C, seed=R)
    loss, logits, dW, db = _oracle(x, W, b, y)
    out = _train(lib, x, H, W, b, y, moments, step=3)
    assert abs(out["loss"][0].item() - loss.item()) <= 1e-5 * abs(loss.item())
    _check_acc(out["acc"][0].item(), logits, y)
    assert rel_err(out["dW"][:C * H].double().view(C, H), dW) < 1e-5
    assert rel_err(out["db"][:C].double(), db) < 1e-5
    # the update is cpc_adam_step's, bit for bit, from the exported gradients
    ps, ms, vs = _adam_reference(lib, W, b, moments, out["dW"][:C * H], out["db"][:C], step=3)
    assert torch.equal(out["W"][:C * H], ps[0]) and torch.equal(out["b"][:C], ps[1])
    assert torch.equal(out["mW"][:C * H], ms[0]) and torch.equal(out["mb"][:C], ms[1])
    assert torch.equal(out["vW"][:C * H], vs[0]) and torch.equal(out["vb"][:C], vs[1])
    assert not torch.equal(out["W"][:C * H], W.reshape(-1))
    _check_canaries(out, C)
    # without the optional gradient outputs: the same update
    bare = _train(lib, x, H, W, b, y, moments, step=3, export=False)
    assert torch.equal(bare["W"], out["W"]) and torch.equal(bare["b"], out["b"])
    ev = _eval(lib, x, H, W, b, y)
    assert torch.equal(ev["loss"][:1], out["loss"][:1]) and torch.equal(ev["acc"][:1], out["acc"][:1])
    _check_canaries(ev, C)
    assert lib.cpc_device_error_flags(1) == 0


def test_probe_reads_the_last_frame_through_its_row_stride_emulated():
    """SpeakerCriterion: cFeature[:, -1, :] read in place (ldx = S * 256)."""
    lib = emu()
    Bq, S, C = 8, 16, 12
    g = torch.Generator().manual_seed(5)
    c = torch.randn(Bq, S, H, generator=g)
    W, b = 0.1 * torch.randn(C, H, generator=g), 0.1 * torch.randn(C, generator=g)
    y = torch.randint(0, C, (Bq,), generator=g)
    last = c[:, -1, :]
    assert last.stride(0) == S * H
    moments = _moments(C, seed=6)
    out = _train(lib, last, S * H, W, b, y, moments)
    loss, logits, dW, db = _oracle(last.contiguous(), W, b, y)
    assert abs(out["loss"][0].item() - loss.item()) <= 1e-5 * abs(loss.item())
    _check_acc(out["acc"][0].item(), logits, y)
    assert rel_err(out["dW"][:C * H].double().view(C, H), dW) < 1e-5 and rel_err(out["db"][:C].double(), db) < 1e-5
    dense = _train(lib, last.contiguous(), H, W, b, y, moments)
    for k in ("loss", "acc", "dW", "db", "W", "b"):
        assert torch.equal(out[k], dense[k]), k
    ev = _eval(lib, last, S * H, W, b, y)
    assert torch.equal(ev["loss"][:1], out["loss"][:1])


def test_accum_is_the_float64_sum_of_the_outputs_emulated():
    lib = emu()
    x, W, b, y = _case(96, 41, seed=17)
    moments = [m.clone() for m in _moments(41, seed=18)]
    accum = torch.full((2 + CANARY,), 7.0, dtype=torch.float64)
    accum[:2] = 0
    losses, accs = [], []
    Wc, bc = W, b
    for step in (1, 2, 3):
        out = _train(lib, x, H, Wc, bc, y, moments, step=step, accum=accum)
        losses.append(out["loss"][0].item())
        accs.append(out["acc"][0].item())
        Wc, bc = out["W"][:41 * H].view(41, H).clone(), out["b"][:41].clone()
        moments = [out["mW"][:41 * H].view(41, H).clone(), out["vW"][:41 * H].view(41, H).clone(), out["mb"][:41].clone(),
                   out["vb"][:41].clone()]
    assert losses[2] < losses[0]                                      # it trains
    assert accum[0].item() == (losses[0] + losses[1]) + losses[2]
    assert accum[1].item() == (accs[0] + accs[1]) + accs[2]
    ev = _eval(lib, x, H, Wc, bc, y, accum=accum)
    assert accum[0].item() == ((losses[0] + losses[1]) + losses[2]) + ev["loss"][0].item()
    assert bool((accum[2:] == 7.0).all())


def test_argmax_ties_break_on_the_first_index_emulated():
    lib = emu()
    R, C = 8, 70
    x, W, b = torch.zeros(R, H), torch.zeros(C, H), torch.zeros(C)
    b[5] = b[66] = 1.0                                   # a tie between class 5 and class 66 (another 64-class step)
    y = torch.tensor([5, 66, 5, 66, 0, 5, 66, 5])
    assert _eval(lib, x, H, W, b, y)["acc"][0].item() == 4 / 8       # torch.max picks 5


def test_identical_calls_give_identical_bits_emulated():
    lib = emu()
    x, W, b, y = _case(700, 300, seed=21)                 # several row slabs, several class steps
    moments = _moments(300, seed=22)
    a1, a2 = _train(lib, x, H, W, b, y, moments), _train(lib, x, H, W, b, y, moments)
    for k in ("loss", "acc", "dW", "db", "W", "b", "mW", "vW", "mb", "vb", "accum"):
        assert torch.equal(a1[k], a2[k]), k
    e1, e2 = _eval(lib, x, H, W, b, y), _eval(lib, x, H, W, b, y)
    assert torch.equal(e1["loss"], e2["loss"]) and torch.equal(e1["acc"], e2["acc"])


@pytest.mark.parametrize("R,C", [(200, 4100), (8300, 5)])
def test_slabs_of_several_tiles_emulated(R, C):
    """More 32-row tiles than slabs -- many classes (the partials' cap leaves few slabs; a workgroup per slab and class step) or
    more than 256 tiles (C <= 64: both walks in one workgroup, the rows' log-sum-exp kept in the workspace in between)."""
    lib = emu()
    Z, rows = _layout(lib, R, C)[1:]
    assert Z < (R + 31) // 32 and rows > 32
    x, W, b, y = _case(R, C, seed=31)
    moments = _moments(C, seed=32)
    out = _train(lib, x, H, W, b, y, moments)
    loss, logits, dW, db = _oracle(x, W, b, y)
    assert abs(out["loss"][0].item() - loss.item()) <= 1e-5 * abs(loss.item())
    _check_acc(out["acc"][0].item(), logits, y)
    assert rel_err(out["dW"][:C * H].double().view(C, H), dW) < 1e-5 and rel_err(out["db"][:C].double(), db) < 1e-5
    _check_canaries(out, C)
    ev = _eval(lib, x, H, W, b, y)
    assert torch.equal(ev["loss"][:1], out["loss"][:1]) and torch.equal(ev["acc"][:1], out["acc"][:1])
    _check_canaries(ev, C)


@pytest.mark.parametrize("C", [41, 70])
def test_label_out_of_range_flags_and_gives_nan_emulated(C):
    lib = emu()
    lib.cpc_device_error_flags(1)
    x, W, b, y = _case(40, C, seed=9)
    y[7] = C
    out = _train(lib, x, H, W, b, y, _moments(C, seed=10))
    assert torch.isnan(out["loss"][0]) and torch.isnan(out["accum"][0])
    assert lib.cpc_device_error_flags(1) == LABEL_RANGE
    _check_canaries(out, C)
    y[7] = -1
    assert torch.isnan(_eval(lib, x, H, W, b, y)["loss"][0])
    assert lib.cpc_device_error_flags(1) == LABEL_RANGE
    assert lib.cpc_device_error_flags(1) == 0


def test_shapes_and_arguments_are_checked_before_any_launch_emulated():
    lib = emu()
    sizes = (ctypes.c_long * 3)()
    for bad in [(0, 41), (4, 1), (4, 8193), (1 << 20, 4096)]:
        assert lib.cpc_probe_layout(*bad, sizes) == 1, bad
    assert lib.cpc_probe_layout(4, 41, None) == 2
    assert lib.cpc_probe_layout(1, 2, sizes) == 0 and lib.cpc_probe_layout(262143, 8192, sizes) == 0
    x, W, b, y = _case(4, 41, seed=1)
    m = [t.clone() for t in _moments(41, seed=2)]
    Wc, bc = W.clone(), b.clone()
    ws, loss = torch.full((4096,), 7.0), torch.full((1,), 7.0)
    acc = torch.zeros(1, dtype=torch.float64)
    bc1, bc2s = _bias_corrections(1)

    def train(x_=P(x), ldx=H, y_=P(y), R=4, C=41, W_=P(Wc), ws_=P(ws), bc1_=bc1):
        return lib.cpc_probe_train_step(x_, ldx, y_, R, C, W_, P(bc), P(m[0]), P(m[1]), P(m[2]), P(m[3]), LR, BETA1, BETA2, EPS, bc1_,
                                        bc2s, ws_, P(loss), P(acc), None, None, None, None)

    assert train(C=1) == 1 and train(C=8193) == 1 and train(R=0) == 1
    assert train(x_=None) == 2 and train(ldx=255) == 2 and train(y_=None) == 2 and train(W_=None) == 2 and train(ws_=None) == 2
    assert train(bc1_=0.0) == 2
    assert lib.cpc_probe_eval(P(x), 255, P(y), 4, 41, P(W), P(b), P(ws), P(loss), P(acc), None, None) == 2
    assert lib.cpc_probe_eval(P(x), H, P(y), 4, 41, P(W), P(b), P(ws), None, P(acc), None, None) == 2
    assert lib.cpc_probe_eval(P(x), H, P(y), 4, 8193, P(W), P(b), P(ws), P(loss), P(acc), None, None) == 1
    assert bool((ws == 7.0).all()) and bool((loss == 7.0).all()) and torch.equal(Wc, W) and torch.equal(bc, b)
