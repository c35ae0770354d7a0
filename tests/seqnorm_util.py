"""Shared by the seqNorm tests: seeded cases, the float64 CPU oracle (CTCphone_criterion's own non-in-place loop times a
given scale, autograd for dx) and the calls through the C ABI (the emulator library on the CPU)."""
import json
import os

import numpy as np
import torch

from cpc_audio_amd import common_voices_eval as CV
from oracle.make_golden_predictors import seeded_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LSTM_KEYS = ("conv1.weight_ih_l0", "conv1.weight_hh_l0", "conv1.bias_ih_l0", "conv1.bias_hh_l0")
H = 256
LENGTH_RANGE = 128           # CPC_DEVERR_LENGTH_RANGE
EPS = 1e-8

# name -> (B, S, lengths, channel offset).  The kernel's time tile is 32 frames: 45 has a ragged second tile, 130 crosses four
# tiles and ends in a ragged fifth.  The offset cases are the ones a one-pass variance (E[x^2] - m^2) fails.
FORWARD_CASES = {
    "one-2": (1, 2, [2], 0.0),
    "ragged-45": (3, 45, [45, 38, 2], 0.0),
    "tiles-130": (2, 130, [130, 67], 0.0),
    "offset-45": (3, 45, [45, 38, 3], 30.0),
    "offset-130": (2, 130, [130, 67], 30.0),
}
# every length >= 3: at n = 2 the normalised values are +-1/sqrt(2) whatever x is, the true gradient of the valid frames is 0
# and a relative error measures rounding noise only
BACKWARD_CASES = {
    "three-3": (1, 3, [3], 0.0),
    "ragged-45": (3, 45, [45, 38, 3], 0.0),
    "tiles-130": (2, 130, [130, 67], 0.0),
    "offset-45": (3, 45, [45, 38, 3], 30.0),
    "offset-130": (2, 130, [130, 67], 30.0),
}


def P(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def case(B, S, lengths, offset, seed):
    """x (B, S, 256) with unit spread around a per-channel offset, lengths (B) int64, dy, and a scale in {0, 2} with both."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, H, generator=g) + offset * (1.0 + 0.1 * torch.randn(H, generator=g))
    dy = torch.randn(B, S, H, generator=g)
    scale = torch.empty(B, H).bernoulli_(0.5, generator=g).mul_(2)
    scale[:, 0], scale[:, 1] = 0.0, 2.0
    return x, torch.tensor(lengths, dtype=torch.long), dy, scale


def oracle(x, lengths, scale=None, normalise=True, dy=None):
    """float64: y, and with dy (y, dx).  With normalise also m and r per (b, c): -> dict."""
    xr = x.double().clone().requires_grad_(True)
    B, S, _ = x.shape
    out = {}
    cur = xr
    if normalise:
        rows, ms, rs = [], [], []
        for b in range(B):
            size = S if lengths is None else int(lengths[b])
            m = xr[b, :size].mean(dim=0, keepdim=True)
            v = xr[b, :size].var(dim=0, keepdim=True)
            rows.append((xr[b] - m) / torch.sqrt(v + EPS))
            ms.append(m.detach()[0])
            rs.append((1.0 / torch.sqrt(v + EPS)).detach()[0])
        cur = torch.stack(rows)
        out.update(m=torch.stack(ms), r=torch.stack(rs))
    if scale is not None:
        cur = cur * scale.double()[:, None, :]
    out["y"] = cur.detach()
    if dy is not None:
        (cur * dy.double()).sum().backward()
        out["dx"] = xr.grad
    return out


def misaligned(t):
    """A copy of t whose data pointer is 4 bytes past a 16-byte boundary (the kernels' scalar path)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype)
    skip = (1 - buf.data_ptr() // 4) % 4           # first element at 16 k + 4 bytes
    view = buf[skip:skip + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _out(n, canary, fill, scalar):
    buf = torch.full((n + canary + 8,), fill)
    skip = -(buf.data_ptr() // 4) % 4 + (1 if scalar else 0)
    return buf[skip:skip + n + canary]


def run_forward(lib, x, lengths, scale, normalise=True, want_stats=True, canary=0, fill=7.0, scalar=False):
    """cpc_seqnorm_forward on host tensors -> (y, stats or None), flat, each with `canary` spare floats.  scalar: x and y
    sit 4 bytes past a 16-byte boundary."""
    B, S, _ = x.shape
    x = misaligned(x) if scalar else x.contiguous()
    y = _out(B * S * H, canary, fill, scalar)
    stats = _out(B * 2 * H, canary, fill, False) if want_stats else None
    assert lib.cpc_seqnorm_forward(P(x), P(lengths), P(scale), P(y), P(stats), B, S, int(normalise), None) == 0
    return y, stats


def run_backward(lib, x, dy, lengths, scale, stats, normalise=True, canary=0, fill=7.0, scalar=False):
    """cpc_seqnorm_backward on host tensors -> dx, flat with `canary` spare floats."""
    B, S, _ = dy.shape
    x = None if x is None else (misaligned(x) if scalar else x.contiguous())
    dy = misaligned(dy) if scalar else dy.contiguous()
    dx = _out(B * S * H, canary, fill, scalar)
    assert lib.cpc_seqnorm_backward(P(x), P(dy), P(lengths), P(scale), P(stats), P(dx), B, S, int(normalise), None) == 0
    return dx


# ---- the reference fixture (tools/make_golden_phone_front.py)
def golden():
    with open(os.path.join(GOLDEN, "phone_front_meta.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN, "phone_front.npz"))), meta


def golden_criterion(meta, lstm, **kw):
    crit = CV.CTCphone_criterion(meta["dimEncoder"], meta["nPhones"], lstm, seqNorm=meta["seqNorm"], reduction=meta["reduction"],
                                 **kw)
    assert list(crit.state_dict().keys()) == meta["keys"]
    crit.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in crit.state_dict().items()}, meta["seed"]))
    return crit.eval()


def check_against_golden(crit, arrays, meta, lstm, device, pred_tol, grad_tol):
    """forward + backward of `crit` on the fixture's input against the reference's prediction, loss and gradients (norm-relative)."""
    tag = "lstm" if lstm else "plain"
    rel = lambda a, b: float((a.double().cpu() - b.double()).norm() / b.double().norm())     # noqa: E731
    x = torch.from_numpy(arrays["x"]).to(device)
    x0 = x.clone()
    sizes = torch.tensor(meta["feature_size"], device=device)
    label = torch.from_numpy(arrays["label"]).to(device)
    label_size = torch.tensor(meta["label_size"], device=device)
    with torch.no_grad():
        pred = crit.getPrediction(x, sizes)
    assert rel(pred, torch.from_numpy(arrays[f"pred_{tag}"])) < pred_tol
    loss = crit(x, sizes, label, label_size)
    assert abs(float(loss.detach()) - meta["loss"][tag]) <= 1e-5 * abs(meta["loss"][tag])
    loss.sum().backward()
    head = crit.PhoneCriterionClassifier
    assert rel(head.weight.grad, torch.from_numpy(arrays[f"dweight_{tag}"])) < grad_tol
    assert rel(head.bias.grad, torch.from_numpy(arrays[f"dbias_{tag}"])) < grad_tol
    if lstm:
        for k in LSTM_KEYS:
            grad = dict(crit.named_parameters())[k].grad
            sub = grad[::16, ::16] if grad.dim() == 2 else grad[::16]
            assert rel(sub, torch.from_numpy(arrays["d" + k])) < grad_tol, k
            assert abs(float(grad.double().norm()) - meta["lstm_grad_norm"][k]) < grad_tol * meta["lstm_grad_norm"][k], k
            assert abs(float(grad.double().sum()) - meta["lstm_grad_sum"][k]) < grad_tol * meta["lstm_grad_norm"][k], k
    assert torch.equal(x, x0)                                  # the module does not write into its input (the reference does)
