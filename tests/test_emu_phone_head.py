"""The PER phone classifier's kernels (csrc/phone_head.hip) on the host SIMT emulator against torch in float64 on the CPU:
the windowed head Conv1d(256, C, 8, stride 4) forward and backward, and log_softmax + nn.CTCLoss(zero_infinity=True) with
per-sequence input lengths and padded targets.  Every output buffer carries spare canary floats that must stay untouched.

Tolerances are those of the project's other supervised kernels (tests/test_emu_supervised.py): the head alone 1e-5, losses
1e-5 relative, CTC gradients 1e-4."""
import pytest
import torch

from emu_util import emu, rel_err
from phone_head_util import (H, LABEL_RANGE, LENGTH_RANGE, P, frames_for, head_case, layout, oracle_ctc, oracle_head,
                             ragged_targets, run_ctc, run_head)

CANARY = 64


def _canaries_ok(out, keys, fill=7.0):
    for k in keys:
        if out.get(k) is None:
            continue
        tail = out[k][out["n"][k]:]
        assert tail.numel() == CANARY, k
        assert bool(torch.isnan(tail).all()) if k == "scratch" else bool((tail == fill).all()), k


@pytest.mark.parametrize("B,S,C", [(1, 8, 2), (2, 11, 7), (3, 12, 7), (2, 37, 41), (1, 77, 65)])
def test_head_matches_conv1d_float64_emulated(B, S, C):
    """(1, 8, 2) one window; (2, 11, 7) an uncovered tail; (3, 12, 7) two overlapping windows; (1, 77, 65) a second class tile."""
    lib = emu()
    x, W, b = head_case(B, S, C, seed=B + S + C)
    T = (S - 8) // 4 + 1
    dl = torch.randn(B, T, C, generator=torch.Generator().manual_seed(S))
    out = run_head(lib, x, W, b, dlogits=dl, canary=CANARY)
    assert out["T"] == T
    logits, dW, db, dX = oracle_head(x, W, b, dl)
    assert rel_err(out["logits"][:B * T * C].double().view(B, T, C), logits) < 1e-5
    assert rel_err(out["dW"][:C * H * 8].double().view(C, H, 8), dW) < 1e-5
    assert rel_err(out["db"][:C].double(), db) < 1e-5
    got_dx = out["dX"][:B * S * H].view(B, S, H)
    assert rel_err(got_dx.double(), dX) < 1e-5
    covered = 4 * (T - 1) + 8
    assert bool((got_dx[:, covered:] == 0).all()) and bool((dX[:, covered:] == 0).all())
    wr = out["wr"][:C * H * 8].view(C, 8, H)
    assert torch.equal(wr, W.permute(0, 2, 1))
    _canaries_ok(out, ("wr", "scratch", "logits", "dW", "db", "dX"))


def test_head_uncovered_tail_and_null_dx_emulated():
    lib = emu()
    x, W, b = head_case(2, 11, 7, seed=5)
    dl = torch.randn(2, 1, 7, generator=torch.Generator().manual_seed(6))
    full = run_head(lib, x, W, b, dlogits=dl, canary=CANARY)
    assert bool((full["dX"][:2 * 11 * H].view(2, 11, H)[:, 8:] == 0).all())           # frames 8..10: no window
    assert bool((full["dX"][:2 * 11 * H].view(2, 11, H)[:, :8] != 0).any())
    none = run_head(lib, x, W, b, dlogits=dl, need_dx=False, canary=CANARY)            # frozen features: dX = NULL
    assert none["dX"] is None
    assert torch.equal(none["dW"], full["dW"]) and torch.equal(none["db"], full["db"])
    _canaries_ok(none, ("wr", "scratch", "logits", "dW", "db"))


def test_head_is_batch_independent_and_deterministic_emulated():
    lib = emu()
    x, W, b = head_case(3, 37, 41, seed=8)
    dl = torch.randn(3, 8, 41, generator=torch.Generator().manual_seed(9))
    a1, a2 = run_head(lib, x, W, b, dlogits=dl), run_head(lib, x, W, b, dlogits=dl)
    for k in ("logits", "dW", "db", "dX"):
        assert torch.equal(a1[k], a2[k]), k
    alone = run_head(lib, x[:1].contiguous(), W, b, dlogits=dl[:1].contiguous())
    assert torch.equal(alone["logits"], a1["logits"][:8 * 41])
    assert torch.equal(alone["dX"], a1["dX"][:37 * H])


def _logits(B, T, C, seed):
    return 2.0 * torch.randn(B, T, C, generator=torch.Generator().manual_seed(seed))


def _check_ctc(lib, logits, in_len, targets, tgt_len, blank, reduction, dloss=None):
    B, T, C = logits.shape
    loss, dl, saved = run_ctc(lib, logits, in_len, targets, tgt_len, blank, reduction, dloss=dloss, canary=CANARY)
    rl, rdl = oracle_ctc(logits, in_len, targets, tgt_len, blank, reduction, dloss=dloss)
    n_loss = B if reduction == "none" else 1
    got = loss[:n_loss].double()
    assert bool(((got - rl.view(-1)).abs() <= 1e-5 * rl.view(-1).abs()).all()), (got, rl)
    got_dl = dl[:B * T * C].view(B, T, C)
    if rdl.norm() > 0:
        assert rel_err(got_dl.double(), rdl) < 1e-4
    for bq in range(B):                                    # exactly 0 behind the input length and for infeasible sequences
        assert bool((got_dl[bq, int(in_len[bq]):] == 0).all()), bq
        if bool((rdl[bq] == 0).all()):
            assert bool((got_dl[bq] == 0).all()), bq
    assert bool((loss[n_loss:] == 7.0).all()) and bool((dl[B * T * C:] == 7.0).all())
    _, _, _, _, saved_n = layout(lib, B, frames_for(T), C, targets.shape[1])
    assert saved.numel() == saved_n + CANARY and bool(torch.isnan(saved[saved_n:]).all())
    assert lib.cpc_device_error_flags(1) == 0
    return got, got_dl


def _four():
    """Input lengths [8, 5, 2, 0]; targets [1,1,2], six times 3 (does not fit into 5 frames), [] and [2] (no frame at all)."""
    targets = torch.tensor([[1, 1, 2, 0, 0, 0], [3, 3, 3, 3, 3, 3], [0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0]])
    return torch.tensor([8, 5, 2, 0]), targets, torch.tensor([3, 6, 0, 1])


@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_ctc_with_lengths_matches_torch_float64_emulated(reduction):
    lib = emu()
    in_len, targets, tgt_len = _four()
    logits = _logits(4, 8, 7, seed=31)
    loss, dl = _check_ctc(lib, logits, in_len, targets, tgt_len, 6, reduction)
    assert bool((dl[1] == 0).all()) and bool((dl[3] == 0).all())       # infinite losses: zero_infinity
    assert bool((dl[0] != 0).all()) and bool((dl[2, :2] != 0).all())
    if reduction == "none":
        assert loss[1] == 0 and loss[3] == 0 and loss[0] > 0 and loss[2] > 0


def test_ctc_repeats_at_the_minimal_feasible_length_emulated():
    """[1, 1, 2] needs a blank between its repeats: 4 frames are the least, 3 are infeasible (loss 0, gradient 0)."""
    lib = emu()
    targets = torch.tensor([[1, 1, 2], [1, 1, 2]])
    logits = _logits(2, 8, 7, seed=32)
    loss, dl = _check_ctc(lib, logits, torch.tensor([4, 3]), targets, torch.tensor([3, 3]), 6, "none")
    assert loss[0] > 0 and loss[1] == 0 and bool((dl[1] == 0).all())


@pytest.mark.parametrize("B,T,C,Lmax,reduction", [(3, 8, 7, 4, "mean"),      # every target as long as the padding
                                                   (3, 8, 2, 3, "sum"),       # one phone: every target is a run of repeats
                                                   (2, 8, 65, 5, "mean"),     # a second 64-class tile
                                                   (3, 1, 7, 1, "sum")])      # a single window
def test_ctc_edge_shapes_emulated(B, T, C, Lmax, reduction):
    lib = emu()
    full = (C, Lmax) == (7, 4)
    targets, tgt_len = ragged_targets(B, Lmax, C - 1, seed=C + T, lengths=[Lmax] * B if full else None)
    in_len = torch.tensor([T, max(T - 1, 1), T][:B])
    _check_ctc(lib, _logits(B, T, C, seed=33 + C), in_len, targets, tgt_len, C - 1, reduction)


def test_ctc_scales_with_dloss_and_reads_the_target_stride_emulated():
    lib = emu()
    in_len, targets, tgt_len = _four()
    logits = _logits(4, 8, 7, seed=34)
    _check_ctc(lib, logits, in_len, targets, tgt_len, 6, "mean", dloss=torch.tensor([-2.5]))
    _check_ctc(lib, logits, in_len, targets, tgt_len, 6, "none", dloss=torch.tensor([0.5, 3.0, -1.25, 2.0]))
    wide = torch.full((4, 11), 99)                         # a view into a wider tensor: row stride 11
    wide[:, :6] = targets
    loss_v, dl_v, _ = run_ctc(lib, logits, in_len, wide[:, :6], tgt_len, 6, "sum")
    loss_c, dl_c, _ = run_ctc(lib, logits, in_len, targets, tgt_len, 6, "sum")
    assert wide[:, :6].stride(0) == 11 and torch.equal(loss_v, loss_c) and torch.equal(dl_v, dl_c)


def test_ctc_is_batch_independent_and_deterministic_emulated():
    lib = emu()
    in_len, targets, tgt_len = _four()
    logits = _logits(4, 8, 7, seed=35)
    l1, d1, _ = run_ctc(lib, logits, in_len, targets, tgt_len, 6, "none")
    l2, d2, _ = run_ctc(lib, logits, in_len, targets, tgt_len, 6, "none")
    assert torch.equal(l1, l2) and torch.equal(d1, d2)
    la, da, _ = run_ctc(lib, logits[:1].contiguous(), in_len[:1], targets[:1], tgt_len[:1], 6, "none")
    assert torch.equal(la[0], l1[0]) and torch.equal(da, d1[:8 * 7])


def test_bad_labels_and_lengths_flag_and_give_nan_for_that_sequence_only_emulated():
    lib = emu()
    lib.cpc_device_error_flags(1)
    in_len, targets, tgt_len = _four()
    logits = _logits(4, 8, 7, seed=36)
    good, _, _ = run_ctc(lib, logits, in_len, targets, tgt_len, 6, "none")
    for bad_label in (6, 7, -1):                           # the blank, beyond the classes, negative
        t = targets.clone()
        t[0, 1] = bad_label
        loss, dl, _ = run_ctc(lib, logits, in_len, t, tgt_len, 6, "none", canary=CANARY)
        assert lib.cpc_device_error_flags(1) == LABEL_RANGE, bad_label
        assert torch.isnan(loss[0]) and torch.equal(loss[1:4], good[1:4])
        assert bool((loss[4:] == 7.0).all()) and bool((dl[4 * 8 * 7:] == 7.0).all())
    t = targets.clone()
    t[0, 5] = 99                                           # behind the target's length: never read
    loss, _, _ = run_ctc(lib, logits, in_len, t, tgt_len, 6, "none")
    assert torch.equal(loss, good) and lib.cpc_device_error_flags(1) == 0
    for lens in ((torch.tensor([9, 5, 2, 0]), tgt_len), (torch.tensor([-1, 5, 2, 0]), tgt_len),
                 (in_len, torch.tensor([7, 6, 0, 1])), (in_len, torch.tensor([-1, 6, 0, 1]))):
        loss, dl, _ = run_ctc(lib, logits, lens[0], targets, lens[1], 6, "none", canary=CANARY)
        assert lib.cpc_device_error_flags(1) == LENGTH_RANGE
        assert torch.isnan(loss[0]) and torch.equal(loss[1:4], good[1:4])
        assert bool((dl[4 * 8 * 7:] == 7.0).all())
    loss, _, _ = run_ctc(lib, logits, torch.tensor([9, 5, 2, 0]), targets, tgt_len, 6, "sum")
    assert torch.isnan(loss[0])


def test_arguments_are_checked_before_any_launch_emulated():
    lib = emu()
    x = torch.full((8 * H,), 7.0)
    W, b = torch.zeros(7, H, 8), torch.zeros(7)
    buf = torch.full((64,), 7.0)
    lens = torch.zeros(1, dtype=torch.long)
    assert lib.cpc_phone_head_forward(P(x), P(W), P(b), P(buf), P(buf), P(buf), 1, 7, 7, None) == 1      # S < 8
    assert lib.cpc_phone_head_forward(P(x), P(W), P(b), None, P(buf), P(buf), 1, 8, 7, None) == 2
    assert lib.cpc_phone_head_backward(P(x), P(buf), P(buf), P(buf), P(buf), P(buf), None, 1, 8, 1, None) == 1
    assert lib.cpc_phone_head_backward(P(x), P(buf), None, P(buf), P(buf), P(buf), None, 1, 8, 7, None) == 2
    assert lib.cpc_ctc_seq_forward(P(buf), P(lens), P(lens), 1, P(lens), P(buf), P(buf), 1, 1, 7, 513, 6, 2, None) == 1
    assert lib.cpc_ctc_seq_forward(P(buf), P(lens), P(lens), 1, P(lens), P(buf), P(buf), 1, 1, 7, 1, 7, 2, None) == 2   # blank
    assert lib.cpc_ctc_seq_forward(P(buf), P(lens), P(lens), 1, P(lens), P(buf), P(buf), 1, 1, 7, 1, 6, 3, None) == 2   # reduction
    assert lib.cpc_ctc_seq_forward(P(buf), P(lens), None, 1, P(lens), P(buf), P(buf), 1, 1, 7, 1, 6, 2, None) == 2
    assert lib.cpc_ctc_seq_forward(P(buf), P(lens), P(lens), 0, P(lens), P(buf), P(buf), 1, 1, 7, 1, 6, 2, None) == 2   # stride
    assert lib.cpc_ctc_seq_backward(P(buf), P(buf), P(buf), P(buf), 1, 2049, 7, 1, 6, 2, None) == 1
    assert lib.cpc_ctc_seq_backward(P(buf), P(buf), None, P(buf), 1, 1, 7, 1, 6, 2, None) == 2
    assert bool((buf == 7.0).all())
