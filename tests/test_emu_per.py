"""PER kernels (csrc/ctc_decode.hip) on the host SIMT emulator: the batched beam search bit for bit against the reference's
beam_search lists in tests/golden/per.npz (float32 and float64; all-zero ties, exact non-zero ties, subnormals, a prefix that
leaves the beam and comes back), the reference unit tests' known answers, mixed lengths in one batch, canaries behind every
output, the range flag, and the Needleman-Wunsch score against the reference's values."""
import ctypes
import math

import numpy as np
import pytest
import torch

import per_util as U
from emu_util import P, emu
from cpc_audio_amd import seq_alignment as SA

DECODE_RANGE = 64     # CPC_DEVERR_DECODE_RANGE
CANARY = 8

CASES = U.beam_cases()


def _decode(lib, tabs, lengths, n_keep, blank, n_out, T_max=None):
    """cpc_ctc_beam_search on (B, T_max, P) host tensors with canaries behind every output -> per sequence [(score, labels)]."""
    Pn = tabs[0].shape[1]
    T_max = T_max or max(t.shape[0] for t in tabs)
    dtype = torch.float32 if tabs[0].dtype == np.float32 else torch.float64
    probs = torch.zeros(len(tabs), T_max, Pn, dtype=dtype)
    for b, t in enumerate(tabs):
        probs[b, :t.shape[0]] = torch.from_numpy(t)
    B = len(tabs)
    lens = torch.tensor(lengths, dtype=torch.int32)
    sizes = (ctypes.c_long * 7)()
    assert lib.cpc_ctc_decode_layout(B, T_max, Pn, n_keep, sizes) == 0
    scratch = torch.empty(int(sizes[0]), dtype=torch.uint8)
    labels = torch.full((B * n_out * T_max + CANARY,), 7777, dtype=torch.int32)
    label_len = torch.full((B * n_out + CANARY,), 7777, dtype=torch.int32)
    scores = torch.full((B * n_out + CANARY,), 7777.0, dtype=dtype)
    n_beams = torch.full((B + CANARY,), 7777, dtype=torch.int32)
    rc = lib.cpc_ctc_beam_search(P(probs), 0 if dtype == torch.float32 else 1, *probs.stride(), P(lens), B, T_max, Pn, blank,
                                 n_keep, n_out, P(scratch), scratch.numel(), P(labels), P(label_len), P(scores), P(n_beams),
                                 None)
    assert rc == 0
    for t, n in ((labels, B * n_out * T_max), (label_len, B * n_out), (scores, B * n_out), (n_beams, B)):
        assert (t[n:] == 7777).all(), "an output was written past its end"
    labels = labels[:B * n_out * T_max].view(B, n_out, T_max)
    label_len, scores = label_len[:B * n_out].view(B, n_out), scores[:B * n_out].view(B, n_out)
    out = []
    for b in range(B):
        nb = min(int(n_beams[b]), n_out)
        for k in range(nb):
            row = labels[b, k]
            assert (row[int(label_len[b, k]):] == SA.PAD).all()
        out.append([(scores[b, k].numpy(), labels[b, k, :int(label_len[b, k])].tolist()) for k in range(nb)])
    return out, n_beams[:B], scores


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{c['kind']}-T{c['T']}-P{c['P']}-K{c['n_keep']}-{c['dtype']}"
                                                       for c, _ in CASES])
def test_beam_search_bit_identical_to_reference(k):
    case, tab = CASES[k]
    got, _, _ = _decode(emu(), [tab], [tab.shape[0]], case["n_keep"], case["blank"], case["n_keep"])
    U.check_list(got[0], case)


def test_fixture_covers_the_hard_cases():
    kinds = {c["kind"] for c, _ in CASES}
    assert {"peaked", "flat", "ties", "reentry", "unit"} <= kinds
    assert any(c["all_zero"] and c["dtype"] == "f32" for c, _ in CASES)
    assert {c["n_keep"] for c, _ in CASES} >= {1, 2, 20, 100} and {c["P"] for c, _ in CASES} >= {3, 12, 41, 128}


def test_reference_known_answers():
    lib = emu()
    big = np.array([[0.1, 0.2, 0., 0., 0., 0., 0., 0.01, 0., 0.1, 0.99, 0.1],
                    [0.1, 0.2, 0.6, 0.1, 0.9, 0., 0., 0.01, 0., 0.9, 1., 0.]])
    got, _, _ = _decode(lib, [big], [2], 10, 11, 1)
    assert float(got[0][0][0]) == 1.09 and got[0][0][1] == [10]
    small = np.array([[0.1, 0.2, 0.], [0.4, 0.2, 0.6], [0.01, 0.3, 0.]])
    got, _, _ = _decode(lib, [small], [3], 10, 2, 10)
    want = [(0.036, [1, 1]), (0.0004, [0]), (0.012, [1]), (0.024, [1, 0, 1]), (0.0002, [0, 1, 0]), (0.0, [1, 1, 1]),
            (0.0, [1, 1, 0]), (0.0006, [0, 0]), (0.036, [0, 1]), (0.0024, [1, 0])]
    want.sort(reverse=True)
    assert [lab for _, lab in got[0]] == [lab for _, lab in want]
    assert all(abs(float(s) - w) < 1e-8 for (s, _), (w, _) in zip(got[0], want))
    per = _nw(lib, [[0, 1, 1, 2, 0, 2, 2]], [[1, 1, 2, 2, 0, 0]], -1, -1, 0, 1)
    assert per[0] == 4. / 7.


def test_mixed_lengths_in_one_batch():
    """Sequences of different lengths (and the same table cut short) share one launch; each gives its own reference list."""
    lib = emu()
    same_p = [(c, t) for c, t in CASES if c["P"] == 12 and c["dtype"] == "f32" and c["n_keep"] <= 20]
    assert len(same_p) >= 2
    case0, tab0 = same_p[0]
    K, blank = case0["n_keep"], case0["blank"]
    tabs = [t for _, t in same_p] + [tab0[:3]]
    got, n_beams, _ = _decode(lib, tabs, [t.shape[0] for t in tabs], K, blank, K, T_max=max(t.shape[0] for t in tabs) + 5)
    alone = [_decode(lib, [t], [t.shape[0]], K, blank, K)[0][0] for t in tabs]
    for g, a in zip(got, alone):
        assert len(g) == len(a)
        for (s1, l1), (s2, l2) in zip(g, a):
            assert l1 == l2 and U.same_bits(s1, s2, np.float32)
    U.check_list(got[0], case0)


def test_range_flag_marks_the_sequence_and_spares_the_others():
    lib = emu()
    lib.cpc_device_error_flags(1)
    case, tab = next((c, t) for c, t in CASES if c["kind"] == "ties" and c["dtype"] == "f32")
    T = tab.shape[0]
    got, n_beams, scores = _decode(lib, [tab, tab, tab], [T, 0, T + 1], case["n_keep"], case["blank"], 2, T_max=T)
    assert lib.cpc_device_error_flags(1) == DECODE_RANGE
    U.check_list(got[0], {**case, "scores": case["scores"][:2], "labels": case["labels"][:2]})
    assert n_beams.tolist() == [len(case["scores"]), 0, 0]
    assert torch.isnan(scores[1:]).all()
    _, _, scores = _decode(lib, [tab], [T], case["n_keep"], case["P"], 1)        # blank outside [0, P)
    assert torch.isnan(scores).all() and lib.cpc_device_error_flags(1) == DECODE_RANGE
    assert lib.cpc_device_error_flags(1) == 0


def test_limits_are_checked_on_the_host():
    lib = emu()
    sizes = (ctypes.c_long * 7)()
    assert lib.cpc_ctc_decode_layout(1, 10, 129, 20, sizes) == 1          # CPC_ERR_SHAPE
    assert lib.cpc_ctc_decode_layout(1, 10, 41, 129, sizes) == 1
    assert lib.cpc_ctc_decode_layout(1, 10, 41, 0, sizes) == 1
    assert lib.cpc_ctc_decode_layout(2, 100, 41, 128, sizes) == 0 and sizes[4] == 128 and sizes[5] == 128
    assert sizes[2] <= 160 * 1024 and sizes[3] <= sizes[2]
    t = torch.rand(1, 5, 4)
    with pytest.raises(ValueError):
        SA.launch_beam_search(lib, t, torch.tensor([5], dtype=torch.int32), 129, 0, 1)
    with pytest.raises(ValueError):
        SA.launch_beam_search(lib, torch.rand(1, 5, 200), torch.tensor([5], dtype=torch.int32), 4, 0, 1)
    with pytest.raises(ValueError):
        SA.launch_beam_search(lib, t, torch.tensor([5], dtype=torch.int32), 4, 0, 5)     # n_out > n_keep


def _nw(lib, refs, hyps, d, m, r, normalize, canary=True):
    B = len(refs)
    L1, L2 = max([len(a) for a in refs] + [1]), max([len(b) for b in hyps] + [1])
    ref = torch.full((B, L1), -5, dtype=torch.int32)
    hyp = torch.full((B, L2), -6, dtype=torch.int32)
    for k, (a, b) in enumerate(zip(refs, hyps)):
        ref[k, :len(a)] = torch.tensor(a, dtype=torch.int32)
        hyp[k, :len(b)] = torch.tensor(b, dtype=torch.int32)
    rl = torch.tensor([len(a) for a in refs], dtype=torch.int32)
    hl = torch.tensor([len(b) for b in hyps], dtype=torch.int32)
    out = torch.full((B + CANARY,), 7.0, dtype=torch.float64)
    assert lib.cpc_nw_align_score(P(ref), L1, P(rl), L1, P(hyp), L2, P(hl), L2, B, float(d), float(m), float(r), normalize,
                                  P(out), None) == 0
    assert (out[B:] == 7.0).all()
    return out[:B].tolist()


def test_needleman_wunsch_matches_reference():
    lib = emu()
    meta, _ = U.load_golden()
    for e in meta["nw"]:
        got = _nw(lib, [e["ref"]], [e["hyp"]], e["d"], e["m"], e["r"], int(e["normalize"]))[0]
        if e["out"] is None:
            assert math.isnan(got)          # the reference divides by zero
        else:
            assert got == e["out"], (e, got)
    assert meta["per_unit"] == 4. / 7.


def test_needleman_wunsch_long_rows_and_batch():
    """Rows of several 64-row blocks and hypotheses near the 4096 limit, batched, against a float64 restatement."""
    lib = emu()
    rng = np.random.default_rng(3)

    def nw64(a, b, d, m, r):
        t = np.zeros((len(a) + 1, len(b) + 1))
        t[:, 0] = np.arange(len(a) + 1) * d
        t[0, :] = np.arange(len(b) + 1) * d
        for i in range(len(a)):
            for j in range(len(b)):
                t[i + 1, j + 1] = max(t[i, j] + (r if a[i] == b[j] else m), max(t[i + 1, j] + d, t[i, j + 1] + d))
        return -t[-1, -1] / len(a)
    refs = [rng.integers(0, 4, n).tolist() for n in (130, 64, 1, 65)]
    hyps = [rng.integers(0, 4, n).tolist() for n in (90, 200, 4096, 0)]
    got = _nw(lib, refs, hyps, -1, -1, 0, 1)
    for g, a, b in zip(got, refs, hyps):
        assert g == nw64(a, b, -1, -1, 0)


def test_needleman_wunsch_range_flag():
    lib = emu()
    lib.cpc_device_error_flags(1)
    ref = torch.zeros(2, 4, dtype=torch.int32)
    hyp = torch.zeros(2, 4, dtype=torch.int32)
    rl, hl = torch.tensor([4, 5], dtype=torch.int32), torch.tensor([4, 4], dtype=torch.int32)
    out = torch.zeros(2, dtype=torch.float64)
    assert lib.cpc_nw_align_score(P(ref), 4, P(rl), 4, P(hyp), 4, P(hl), 4, 2, -1.0, -1.0, 0.0, 1, P(out), None) == 0
    assert out[0].item() == 0.0 and math.isnan(out[1].item())
    assert lib.cpc_device_error_flags(1) == DECODE_RANGE
    assert lib.cpc_nw_align_score(P(ref), 4, P(rl), 4, P(hyp), 4, P(hl), 4097, 2, -1.0, -1.0, 0.0, 1, P(out), None) == 1
