"""ABX kernels (csrc/abx.hip) on the host SIMT emulator: the DTW-only entry bit for bit against the reference's _dtw outputs in
tests/golden/abx.npz (ties included), the reference's known answers, random pairs on both sides of the 64-row fast path
against a float64 restatement, canaries behind every output, and the index flag."""
import ctypes
import math

import numpy as np
import pytest
import torch

import abx_util as U
from emu_util import P, emu
from cpc_audio_amd import abx

ABX_INDEX = 32     # CPC_DEVERR_ABX_INDEX
CANARY = 8


def _dtw64(d):
    """dtw.pyx:_dtw (normalized) in float64."""
    n, m = d.shape
    c = np.empty((n, m))
    c[0, 0] = d[0, 0]
    for i in range(1, n):
        c[i, 0] = d[i, 0] + c[i - 1, 0]
    for j in range(1, m):
        c[0, j] = d[0, j] + c[0, j - 1]
    for i in range(1, n):
        for j in range(1, m):
            c[i, j] = d[i, j] + min(c[i - 1, j], c[i - 1, j - 1], c[i, j - 1])
    i, j, L = n - 1, m - 1, 1
    while i > 0 and j > 0:
        up, left, dg = c[i - 1, j], c[i, j - 1], c[i - 1, j - 1]
        if dg <= left and dg <= up:
            i, j = i - 1, j - 1
        elif left <= up:
            j -= 1
        else:
            i -= 1
        L += 1
    L += j if i == 0 else 0
    L += i if j == 0 else 0
    return c[n - 1, m - 1] / L


def _dist64(x, y, metric):
    x, y = x.double(), y.double()
    if metric == 0:
        return (torch.clamp(x @ y.T, -1, 1).acos() / math.pi).numpy()
    return torch.cdist(x, y).numpy()


def _dtw_only(lib, d, n, m, ignore_diag=0, symmetric=0):
    """cpc_abx_dtw on one (1, 1, S1, S2) matrix with a canary behind the output."""
    S1, S2 = d.shape
    dist = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).reshape(1, 1, S1, S2).contiguous()
    s1, s2 = torch.tensor([n], dtype=torch.int32), torch.tensor([m], dtype=torch.int32)
    out = torch.full((1 + CANARY,), 7.0)
    assert lib.cpc_abx_dtw(P(dist), P(s1), P(s2), 1, 1, S1, S2, ignore_diag, symmetric, P(out), None) == 0
    assert (out[1:] == 7.0).all()
    return out[0]


def test_dtw_only_bit_identical_to_reference():
    lib = emu()
    _, arrays = U.load_golden()
    for d, (n, m), want in zip(arrays["dtw:mats"], arrays["dtw:sizes"], arrays["dtw:out"]):
        got = _dtw_only(lib, d, int(n), int(m))
        assert np.float32(got.item()) == want, (n, m, got.item(), want)


def test_dtw_only_crafted_ties():
    lib = emu()
    for n, m in ((1, 1), (1, 7), (7, 1), (5, 5), (3, 9), (70, 3), (66, 66)):
        for d in (np.full((n, m), 0.5), np.zeros((n, m)), (np.add.outer(np.arange(n), np.arange(m)) % 2).astype(float)):
            want = np.float32(_dtw64(d.astype(np.float32).astype(np.float64)))
            assert _dtw_only(lib, d, n, m).item() == pytest.approx(float(want), rel=1e-6, abs=1e-7), (n, m)


def _segments(*seqs):
    feat = torch.cat(seqs, dim=0).contiguous()
    lens = torch.tensor([s.size(0) for s in seqs], dtype=torch.int32)
    offs = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int32), lens[:-1]]), 0).to(torch.int32)
    return feat, offs, lens


def _pair_dtw(lib, seqs, pairs, metric):
    feat, offs, lens = _segments(*seqs)
    ids = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).contiguous()
    out = torch.full((len(pairs) + CANARY,), 7.0)
    assert lib.cpc_abx_pair_dtw(P(feat), P(offs), P(lens), len(seqs), feat.size(0), feat.size(1), int(lens.max()), metric,
                                P(ids), len(pairs), P(out), None) == 0
    assert (out[len(pairs):] == 7.0).all()
    return out[:len(pairs)]


def test_reference_known_answers_euclidean():
    lib = emu()
    X = torch.tensor([[[0, 1], [0, 0], [1, 1], [42, 42]], [[0, 2], [0, 1], [1, 1], [-1, 0]],
                      [[0, 0], [0, 1], [0, 0], [21, 211]]], dtype=torch.float)
    sizes = [3, 4, 2]
    Y = torch.tensor([[0, 1], [1, 2], [0, 0]], dtype=torch.float)
    got = _pair_dtw(lib, [X[k, :sizes[k]] for k in range(3)] + [Y], [(0, 3), (1, 3), (2, 3)], 1)
    want = [math.sqrt(2) / 2, 3 / 4, (2 + math.sqrt(2)) / 3]
    assert torch.allclose(got.double(), torch.tensor(want, dtype=torch.float64), atol=1e-6)


def test_reference_known_answers_cosine_singularity():
    lib = emu()
    x = abx.normalize_with_singularity(torch.tensor([[[1., 0., 0., 0.], [0., 0., 0., 0.]],
                                                     [[0., 0., -1., 0.], [0.5, -0.5, 0.5, -0.5]]]))
    y = abx.normalize_with_singularity(torch.tensor([[[-0.5, -0.5, -0.5, 0.5], [0., 0., 0., 0.], [0., 1., 0., 0.]]]))
    frames = [x[0, 0:1], x[0, 1:2], x[1, 0:1], x[1, 1:2]] + [y[0, k:k + 1] for k in range(3)]
    pairs = [(i, 4 + j) for i in range(4) for j in range(3)]
    got = _pair_dtw(lib, frames, pairs, 0).view(4, 3)
    want = torch.tensor([[2 / 3, 1, 1 / 2], [1, 0, 1], [1 / 3, 1, 1 / 2], [2 / 3, 1, 2 / 3]])
    assert (got - want).abs().max() < 1e-4


def _group_scores(lib, seqs, A, B, X, symmetric, metric, groups_first=None, max_len=None):
    feat, offs, lens = _segments(*seqs)
    members, groups, base, work, total = [], [], [], [], 0
    for g, (a, b, x) in enumerate(zip(A, B, X)):
        groups.append((len(members), len(a), len(b), len(x)))
        members += [*a, *b, *x]
        base.append(total)
        total += len(x) * (len(a) + len(b))
        work += [(g, i) for i in range(len(x))]
    sizes = (ctypes.c_long * 4)()
    ml = int(lens.max()) if max_len is None else max_len
    assert lib.cpc_abx_layout(feat.size(1), ml, len(groups), total, sizes) == 0 and sizes[0] == total
    dist = torch.full((total + CANARY,), 7.0)
    scores = torch.full((len(groups) + CANARY,), 7.0)
    t = lambda v, dt=torch.int32: torch.tensor(v, dtype=dt).contiguous()       # noqa: E731
    assert lib.cpc_abx_group_scores(P(feat), P(offs), P(lens), len(seqs), feat.size(0), feat.size(1), ml, metric,
                                    P(t(members)), P(t(groups)), P(t(base, torch.int64)), len(groups), P(t(work)), len(work),
                                    int(symmetric), P(dist), P(scores), None) == 0
    assert (dist[total:] == 7.0).all() and (scores[len(groups):] == 7.0).all()
    return scores[:len(groups)], dist[:total], base


def test_reference_known_answer_symmetric_theta():
    lib = emu()
    A = torch.tensor([[[0, 1], [0, 0], [1, 1], [42, 42]], [[0, 2], [0, 1], [1, 1], [-1, 0]],
                      [[0, 0], [0, 1], [0, 0], [21, 211]]], dtype=torch.float)
    sizes = [3, 4, 2]
    B = torch.tensor([[0, 1], [1, 2], [0, 0]], dtype=torch.float)
    seqs = [A[k, :sizes[k]] for k in range(3)] + [B]
    scores, dist, _ = _group_scores(lib, seqs, [[0, 1, 2]], [[3]], [[0, 1, 2]], True, 1)
    assert scores[0].item() == 0.5                       # theta = 0.5
    dxa = dist[:9].view(3, 3)
    assert torch.equal(dxa, dxa.T) and (dxa.diagonal() == 0).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_random_pairs_against_float64(metric):
    lib = emu()
    g = torch.Generator().manual_seed(21 + metric)
    lens = [1, 2, 5, 17, 40, 64, 65, 70, 131]
    D = 7
    seqs = [torch.randn(n, D, generator=g) for n in lens]
    if metric == 0:
        seqs = [abx.normalize_with_singularity(s[None])[0] for s in seqs]
    pairs = [(0, 4), (4, 0), (2, 3), (5, 3), (6, 2), (7, 6), (8, 1), (3, 8), (8, 4), (5, 5)]
    got = _pair_dtw(lib, seqs, pairs, metric)
    for (i, j), v in zip(pairs, got.tolist()):
        want = _dtw64(_dist64(seqs[i], seqs[j], metric))
        assert v == pytest.approx(want, rel=2e-6, abs=2e-6), (lens[i], lens[j])
    # the same pair gives the same bits wherever it sits: alone, in another list, or as a group's distance
    again = _pair_dtw(lib, seqs, [(7, 6)], metric)
    assert again[0].item() == got[5].item()
    _, dist, _ = _group_scores(lib, seqs, [[6, 2]], [[3]], [[7]], False, metric)
    assert dist[0].item() == got[5].item()


def test_group_scores_match_theta_of_the_distances():
    lib = emu()
    g = torch.Generator().manual_seed(3)
    seqs = [abx.normalize_with_singularity(torch.randn(1, int(n), 9, generator=g))[0]
            for n in torch.randint(1, 12, (12,), generator=g)]
    seqs[5] = seqs[4].clone()                           # an exact duplicate: ties count 0.5
    A, B, X = [[0, 1, 4, 5], [6, 7]], [[2, 3], [8, 9, 10]], [[0, 1, 4, 5], [11, 0]]
    for symmetric in (True, False):
        XX = A if symmetric else X
        scores, dist, base = _group_scores(lib, seqs, A, B, XX, symmetric, 0)
        for k in range(2):
            nx, na, nb = len(XX[k]), len(A[k]), len(B[k])
            dxa = dist[base[k]:base[k] + nx * na].view(nx, na)
            dxb = dist[base[k] + nx * na:base[k] + nx * (na + nb)].view(nx, nb)
            theta = abx.theta_from_distances(dxa, dxb, symmetric)
            assert scores[k].item() == np.float32(1 - theta)


def test_index_flag_and_nan():
    lib = emu()
    lib.cpc_device_error_flags(1)
    seqs = [torch.randn(3, 5), torch.randn(4, 5), torch.randn(2, 5)]
    scores, _, _ = _group_scores(lib, seqs, [[0, 1], [0, 1]], [[2], [7]], [[2], [2]], False, 1)
    assert math.isfinite(scores[0].item()) and math.isnan(scores[1].item())
    assert lib.cpc_device_error_flags(1) & ABX_INDEX
    assert lib.cpc_device_error_flags(1) == 0


def test_argument_validation():
    lib = emu()
    sizes = (ctypes.c_long * 4)()
    assert lib.cpc_abx_layout(1025, 10, 1, 1, sizes) == 1
    assert lib.cpc_abx_layout(257, 1025, 1, 1, sizes) == 1
    assert lib.cpc_abx_layout(257, 0, 1, 1, sizes) == 1
    assert lib.cpc_abx_layout(257, 10, 1, 1, None) == 2
    x = torch.zeros(4)
    s = torch.ones(2, dtype=torch.int32)
    assert lib.cpc_abx_dtw(P(x), P(s), P(s), 2, 1, 1, 1, 0, 1, P(x), None) == 1        # symmetric needs N1 == N2
    assert lib.cpc_abx_pair_dtw(P(x), P(s), P(s), 1, 4, 1, 1, 2, P(s), 1, P(x), None) == 2   # metric
