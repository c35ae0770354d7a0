"""The width-parametric InfoNCE scores (csrc/nce_wide.hip) on the host SIMT emulator, through the C ABI, against torch autograd
(float64) on the reference formula: cpc/criterion/criterion.py:115-116 (mean over the C features of pred * candidate) and
:245-257, on predictions given as a tensor -- as test_emu_nce.py::test_nce_scores_of_foreign_predictions_emulated does at 256.

Bars (tests/test_emu_nce.py): losses and logits within 1e-5 * max(1, |ref|), accuracies within 1e-6, gradients rel_err < 1e-5."""
import ctypes

import pytest
import torch

from cpc_audio_amd import _lib as _L
from cpc_audio_amd.ops import candidate_destinations

from emu_util import P, emu, rel_err
from oracle import cpc_oracle as O

ERR_SHAPE, ERR_ARG = 1, 2       # include/cpc_hip.h: CPC_ERR_SHAPE, CPC_ERR_ARG


def _reference(pred, z, rows, gl, k0=0):
    """pred (B, W, K, C), z (B, S, C), rows (B, W, N) rows of z.view(B*S, C) -> float64 losses (K), acc (K),
    logits (B, W, K, 1+N), d pred, d z for the upstream gradients gl; head k's positive is z[b, t + k0 + k + 1]."""
    B, W, K, C = pred.shape
    S = z.shape[1]
    p = pred.double().requires_grad_(True)
    zr = z.double().requires_grad_(True)
    neg = zr.reshape(B * S, C)[rows.reshape(-1).long()].view(B, W, -1, C)
    losses, accs, logits = [], [], []
    for k in range(K):
        pos = zr[:, k0 + k + 1:k0 + k + 1 + W]
        cand = torch.cat([pos.unsqueeze(2), neg], dim=2)                       # (B, W, 1+N, C)
        sc = (p[:, :, k].unsqueeze(2) * cand).mean(dim=3)                      # (B, W, 1+N)
        flat = sc.reshape(B * W, -1)
        losses.append(torch.nn.functional.cross_entropy(flat, torch.zeros(B * W, dtype=torch.long)))
        accs.append((flat[:, 0] >= flat[:, 1:].max(dim=1).values).double().mean())      # a tie resolves to class 0 (:253)
        logits.append(sc)
    losses = torch.stack(losses)
    (losses * gl.double()).sum().backward()
    return losses.detach(), torch.stack(accs).detach(), torch.stack(logits, dim=2).detach(), p.grad, zr.grad


def _pad(t, Cp):
    return torch.nn.functional.pad(t, (0, Cp - t.shape[-1])).contiguous()


def _prepare(lib, B, S, K, N, seed, Ktot=None):
    W = S - (Ktot or K)
    Np = lib.cpc_nce_padded_negatives(N)
    bi, si = O.draw_negative_indices(B, S, W, N, generator=torch.Generator().manual_seed(seed))
    ext = torch.full((B, W, Np), -1, dtype=torch.int32)
    perm = torch.full((B * W * (Np + K),), -1, dtype=torch.int32)
    row_ptr = torch.full((B * S + 1,), -1, dtype=torch.int32)
    work = torch.zeros(B * W * (Np + K) + 2 * B * S + 2, dtype=torch.int32)
    assert lib.cpc_nce_prepare(P(bi), P(si), P(ext), P(perm), P(row_ptr), P(work), B, S, K, N, None) == 0
    return ext, perm, row_ptr


def _run(lib, pred, z, ext, perm, row_ptr, gl, N):
    """pred (B, W, K, C), z (B, S, C) unpadded -> losses, acc, logits (B, W, K, 1+Np), dpred (B, W, K, Cp), dz (B, S, Cp);
    every buffer the library writes starts as NaN."""
    B, W, K, C = pred.shape
    S = z.shape[1]
    Cp = lib.cpc_nce_wide_padded_width(C)
    Np = ext.shape[2]
    pp, zp = _pad(pred, Cp), _pad(z, Cp)
    sizes = (ctypes.c_long * 5)()
    assert lib.cpc_nce_wide_layout(B, S, K, N, C, sizes) == 0
    saved = torch.full((sizes[0],), float("nan")); fscr = torch.full((sizes[1],), float("nan"))
    bscr = torch.full((sizes[2],), float("nan"))
    losses = torch.full((K,), float("nan")); acc = torch.full((K,), float("nan"))
    assert lib.cpc_nce_wide_forward(P(pp), P(zp), P(ext), P(saved), P(fscr), P(losses), P(acc), B, S, K, N, C, None) == 0
    logits = saved[sizes[3]: sizes[3] + B * W * K * (Np + 1)].view(B, W, K, Np + 1).clone()
    dpred = torch.full((B, W, K, Cp), float("nan")); dz = torch.full((B, S, Cp), float("nan"))
    assert lib.cpc_nce_wide_backward(P(pp), P(zp), P(ext), P(perm), P(row_ptr), P(saved), P(gl), P(bscr), P(dpred), P(dz),
                                     B, S, K, N, C, None) == 0
    return losses, acc, logits, dpred, dz


def _check(got, ref, C, N):
    losses, acc, logits, dpred, dz = got
    rl, ra, rlg, rdp, rdz = ref
    assert (losses - rl).abs().max().item() < 1e-5 * max(1.0, rl.abs().max().item()), (losses, rl)
    assert (acc - ra).abs().max().item() < 1e-6, (acc, ra)
    assert (logits[..., :N + 1] - rlg).abs().max().item() < 1e-5 * max(1.0, rlg.abs().max().item())
    assert (logits[..., N + 1:] <= -3.0e38).all()                           # the padding candidates, masked by position
    assert rel_err(dpred[..., :C].double(), rdp) < 1e-5
    assert rel_err(dz[..., :C].double(), rdz) < 1e-5
    # the padding columns: exactly zero (no NaN left of the fill either)
    assert torch.equal(dpred[..., C:], torch.zeros_like(dpred[..., C:]))
    assert torch.equal(dz[..., C:], torch.zeros_like(dz[..., C:]))


def _inputs(B, S, K, C, scale, seed=3):
    torch.manual_seed(seed)
    W = S - K
    return scale * torch.randn(B, W, K, C), torch.relu(torch.randn(B, S, C)), torch.randn(K)


@pytest.mark.parametrize("B,S,K,N,C,scale", [
    (2, 20, 12, 16, 64, 2.0),        # one block
    (2, 21, 7, 32, 40, 2.0),         # padded
    (3, 19, 5, 24, 13, 2.0),         # padded, C not a multiple of 4, N not a multiple of 16
    (2, 20, 12, 16, 192, 2.0),       # three blocks
    (2, 20, 5, 16, 320, 2.0),        # above 256: two passes of the backward kernels, 80 threads per gathered row
    (1, 20, 16, 16, 512, 2.0),       # eight blocks and a full head tile
    (2, 21, 7, 32, 64, 400.0),       # logits tens apart: the running reference of the online softmax moves
])
def test_wide_scores_forward_backward_emulated(B, S, K, N, C, scale):
    lib = emu()
    pred, z, gl = _inputs(B, S, K, C, scale)
    ext, perm, row_ptr = _prepare(lib, B, S, K, N, seed=11)
    ref = _reference(pred, z, ext[:, :, :N], gl)
    if scale > 100:
        lg = ref[2]
        assert (lg.max(dim=3).values - lg[..., 0]).max().item() > 40.0          # ... it does move (the kernel's threshold)
    _check(_run(lib, pred, z, ext, perm, row_ptr, gl, N), ref, C, N)


def test_wide_scores_eighteen_heads_in_groups_emulated():
    """cpc_nce_head_group: heads 0..15 and 16..17 of an 18-step criterion, W = S - 18 windows, positives z[t + k0 + k + 1]; the
    groups' losses side by side and their dz summed are the 18-head reference's."""
    lib = emu()
    B, S, K, N, C = 2, 25, 18, 24, 40
    pred, z, gl = _inputs(B, S, K, C, 3.0)
    W = S - K
    try:
        dz_sum, ref = torch.zeros(B, S, C, dtype=torch.float64), None
        assert lib.cpc_nce_wide_layout(B, S, K, N, C, (ctypes.c_long * 5)()) != 0       # no group set: K > 16 is not one call
        for k0 in range(0, K, 16):
            kg = min(16, K - k0)
            assert lib.cpc_nce_head_group(k0, K) == 0
            ext, perm, row_ptr = _prepare(lib, B, S, kg, N, seed=5, Ktot=K)
            if ref is None:
                ref = _reference(pred, z, ext[:, :, :N], gl)
            g = gl[k0:k0 + kg].contiguous()
            losses, acc, logits, dpred, dz = _run(lib, pred[:, :, k0:k0 + kg].contiguous(), z, ext, perm, row_ptr, g, N)
            assert lib.cpc_nce_head_group(0, 0) == 0
            rl, ra, rlg, rdp, rdz = ref
            assert (losses - rl[k0:k0 + kg]).abs().max().item() < 1e-5 * max(1.0, rl.abs().max().item())
            assert (acc - ra[k0:k0 + kg]).abs().max().item() < 1e-6
            assert (logits[..., :N + 1] - rlg[:, :, k0:k0 + kg]).abs().max().item() < 1e-5 * max(1.0, rlg.abs().max().item())
            assert rel_err(dpred[..., :C].double(), rdp[:, :, k0:k0 + kg]) < 1e-5
            assert torch.equal(dz[..., C:], torch.zeros_like(dz[..., C:]))
            dz_sum += dz[..., :C].double()
        assert rel_err(dz_sum, ref[4]) < 1e-5
    finally:
        lib.cpc_nce_head_group(0, 0)


def test_a_negative_that_is_the_positive_row_ties_to_class_zero_emulated():
    """criterion.py:253: predictions.max(1)[1] == 0 -- a negative that IS the positive row scores exactly the positive's score
    and the first maximum wins.  The positives go through the same MFMA chain as the negatives, so the tie is bit-exact: the
    crafted window counts as correct and the loss is the reference's."""
    lib = emu()
    B, S, K, N, C = 2, 20, 5, 16, 40
    pred, z, gl = _inputs(B, S, K, C, 2.0)
    W = S - K
    ext, _, _ = _prepare(lib, B, S, K, N, seed=7)
    b, t, k = 1, 6, 3
    pos_row = b * S + t + k + 1
    ext[b, t, 2] = pos_row
    pred[b, t, k] = 40.0 * z[b, t + k + 1]            # ... and it is that head's best candidate by far
    perm, row_ptr = candidate_destinations(ext, B, S, K)
    ref = _reference(pred, z, ext[:, :, :N], gl)
    lg = ref[2][b, t, k]
    assert lg[0] == lg[1 + 2] and (lg[0] > torch.cat([lg[1:3], lg[4:]])).all()         # an exact tie at the top
    got = _run(lib, pred, z, ext, perm, row_ptr, gl, N)
    assert got[2][b, t, k, 0] == got[2][b, t, k, 1 + 2]                                # bit-identical scores
    # without the tie rule the window would count as wrong: 1 / (B W) of head k's accuracy, far above the bar
    _check(got, ref, C, N)


def test_wide_scores_at_256_agree_with_the_plain_scores_path_emulated():
    """Four blocks: the same algorithm as cpc_nce_scores_* under cpc_set_nce_fused(0)."""
    lib = emu()
    B, S, K, N, C = 2, 20, 12, 16, 256
    pred, z, gl = _inputs(B, S, K, C, 2.0)
    W = S - K
    ext, perm, row_ptr = _prepare(lib, B, S, K, N, seed=11)
    got = _run(lib, pred, z, ext, perm, row_ptr, gl, N)
    _check(got, _reference(pred, z, ext[:, :, :N], gl), C, N)
    assert lib.cpc_set_nce_fused(0) == 0
    try:
        sizes = (ctypes.c_long * 6)()
        assert lib.cpc_nce_layout(B, S, K, N, sizes) == 0
        saved = torch.full((sizes[0],), float("nan")); fscr = torch.full((sizes[1],), float("nan"))
        bscr = torch.full((sizes[2],), float("nan"))
        losses = torch.full((K,), float("nan")); acc = torch.full((K,), float("nan"))
        pd = pred.reshape(B, W, K * C).contiguous()
        assert lib.cpc_nce_scores_forward(P(pd), P(z), P(ext), P(saved), P(fscr), P(losses), P(acc), B, S, K, N, None) == 0
        dpred = torch.full((B, W, K * C), float("nan")); dz = torch.full((B, S, C), float("nan"))
        assert lib.cpc_nce_scores_backward(P(pd), P(z), P(ext), P(perm), P(row_ptr), P(saved), P(gl), P(bscr), P(dpred),
                                           P(dz), B, S, K, N, None) == 0
        logits = saved[sizes[4]: sizes[4] + B * W * K * (N + 1)].view(B, W, K, N + 1)
    finally:
        lib.cpc_set_nce_fused(_L.DEFAULT_NCE_FUSED)
    assert (got[0] - losses).abs().max().item() < 1e-5 * max(1.0, losses.abs().max().item())
    assert (got[1] - acc).abs().max().item() < 1e-6
    assert (got[2] - logits).abs().max().item() < 1e-5 * max(1.0, logits.abs().max().item())
    assert rel_err(got[3].reshape(B, W, K * C), dpred) < 1e-5 and rel_err(got[4], dz) < 1e-5


def test_wide_scores_refuse_bad_shapes_and_null_pointers_emulated():
    lib = emu()
    B, S, K, N, C = 2, 20, 5, 16, 40
    sizes = (ctypes.c_long * 5)()
    x = torch.zeros(64)
    for bad in ((B, S, K, N, 0), (B, S, K, N, 513), (B, S, 17, N, C), (B, S, K, 0, C), (B, 5, K, N, C), (0, S, K, N, C)):
        assert lib.cpc_nce_wide_layout(*bad, sizes) == ERR_SHAPE, bad
        assert lib.cpc_nce_wide_forward(P(x), P(x), P(x), P(x), P(x), P(x), P(x), *bad, None) == ERR_SHAPE, bad
        assert lib.cpc_nce_wide_backward(*([P(x)] * 10), *bad, None) == ERR_SHAPE, bad
    assert lib.cpc_nce_wide_forward(None, P(x), P(x), P(x), P(x), P(x), P(x), B, S, K, N, C, None) == ERR_ARG
    assert lib.cpc_nce_wide_backward(*([P(x)] * 9), None, B, S, K, N, C, None) == ERR_ARG
