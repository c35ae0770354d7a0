"""ABX on the MI355X (csrc/abx.hip through cpc_audio_amd.abx) against the reference's outputs in tests/golden/abx.npz: per-group
scores, final within / across scores, the pair API against float64, repeatability, placement independence, long segments and
the command line.  Valid plans only."""
import json
import math
import random

import numpy as np
import pytest
import torch

import abx_util as U
from cpc_audio_amd import abx, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture_set(tmp_path_factory):
    meta, arrays = U.load_golden()
    tmp = str(tmp_path_factory.mktemp("abx"))
    feats = U.file_features(meta["item_text"])
    item, seq = U.write_fixture_files(tmp, meta["item_text"], feats)
    ds = abx.ABXFeatureLoader(item, seq, lambda p: torch.load(p, map_location="cpu"), meta["step_feature"], True)
    return meta, arrays, ds, item, seq, tmp


NAMES = ["within:sampled", "within:full", "across:sampled", "across:full"]


def _plan(ds, name, case):
    random.seed(case["seed"])
    if name.startswith("within"):
        return abx.plan_within(ds, case["max_size_group"])
    return abx.plan_across(ds, case["max_size_group"], 5)


@pytest.mark.parametrize("name", NAMES)
def test_group_scores_match_the_reference(fixture_set, name):
    meta, arrays, ds, _, _, _ = fixture_set
    case = meta["cases"][name]
    plan = _plan(ds, name, case)
    got = abx.score_plan(ds, plan, 0).numpy()
    ops.check_device_errors()
    want, margin = arrays[f"{name}:score"], arrays[f"{name}:margin"]
    off = np.abs(got.astype(np.float64) - want) > 1e-6
    assert not (off & (margin >= 1e-5)).any(), np.nonzero(off & (margin >= 1e-5))
    assert off.sum() < 0.01 * len(want), int(off.sum())
    assert abs(abx.reduce_scores(plan, got) - case["score"]) < 1e-4


def test_abx_final_scores_and_repeatability(fixture_set):
    meta, _, _, item, seq, _ = fixture_set
    load = lambda p: torch.load(p, map_location="cpu")        # noqa: E731
    for mode in ("within", "across"):
        case = meta["cases"][f"{mode}:sampled"]
        random.seed(case["seed"])
        s1 = abx.ABX(load, item, seq, "cosine", meta["step_feature"], [mode], max_size_group=case["max_size_group"])
        assert abs(s1[mode] - case["score"]) < 1e-4
        s2 = abx.ABX(load, item, seq, "cosine", meta["step_feature"], [mode], max_size_group=case["max_size_group"],
                     seed=5)
        s3 = abx.ABX(load, item, seq, "cosine", meta["step_feature"], [mode], max_size_group=case["max_size_group"],
                     seed=5)
        assert s2 == s3                                          # same bits on a repeated call


def _dtw64(d):
    n, m = d.shape
    c = np.empty((n, m))
    c[0, 0] = d[0, 0]
    c[1:, 0] = d[0, 0] + np.cumsum(d[1:, 0])
    c[0, 1:] = d[0, 0] + np.cumsum(d[0, 1:])
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
    return c[-1, -1] / (L + (j if i == 0 else 0) + (i if j == 0 else 0))


@pytest.mark.parametrize("D", [2, 33, 257, 513])
def test_distance_group_dtw_against_float64(D):
    g = torch.Generator().manual_seed(D)
    N1, N2, S = 3, 4, 20
    a1, a2 = torch.randn(N1, S, D, generator=g), torch.randn(N2, S, D, generator=g)
    s1, s2 = torch.randint(1, S + 1, (N1,), generator=g), torch.randint(1, S + 1, (N2,), generator=g)
    n1, n2 = abx.normalize_with_singularity(a1), abx.normalize_with_singularity(a2)
    for fn, x, y in ((abx.get_cosine_distance_batch, n1, n2), (abx.get_euclidian_distance_batch, a1, a2)):
        got = abx.get_distance_group_dtw(x, y, s1, s2, distance_function=fn)
        d64 = fn(x.double(), y.double()).numpy()
        for i in range(N1):
            for j in range(N2):
                want = _dtw64(d64[i, j, :s1[i], :s2[j]])
                assert abs(got[i, j].item() - want) < 5e-5 * max(1.0, abs(want)), (i, j)
        # a custom distance function: torch distances, DTW on the device
        custom = abx.get_distance_group_dtw(x, y, s1, s2, distance_function=lambda p, q: fn(p, q) + 0.0)
        assert (custom - got).abs().max() < 1e-5


def test_same_pair_same_bits_anywhere():
    g = torch.Generator().manual_seed(7)
    a = abx.normalize_with_singularity(torch.randn(5, 30, 257, generator=g))
    s = torch.tensor([30, 12, 1, 25, 7])
    full = abx.get_distance_group_dtw(a, a, s, s)
    sym = abx.get_distance_group_dtw(a, a, s, s, ignore_diag=True, symmetric=True)
    sub = abx.get_distance_group_dtw(a[1:4], a[3:5], s[1:4], s[3:5])
    assert torch.equal(sub, full[1:4, 3:5])
    iu = torch.triu_indices(5, 5, 1)
    assert torch.equal(sym[iu[0], iu[1]], full[iu[0], iu[1]])
    assert torch.equal(full, abx.get_distance_group_dtw(a, a, s, s))


def test_segment_longer_than_128_frames():
    g = torch.Generator().manual_seed(8)
    a = torch.randn(2, 150, 33, generator=g)
    b = torch.randn(2, 140, 33, generator=g)
    sa, sb = torch.tensor([150, 131]), torch.tensor([140, 3])
    got = abx.get_distance_group_dtw(a, b, sa, sb, distance_function=abx.get_euclidian_distance_batch)
    d64 = abx.get_euclidian_distance_batch(a.double(), b.double()).numpy()
    for i in range(2):
        for j in range(2):
            want = _dtw64(d64[i, j, :sa[i], :sb[j]])
            assert abs(got[i, j].item() - want) < 5e-5 * max(1.0, want)


def test_theta_group_dtw_reference_answer():
    A = torch.tensor([[[0, 1], [0, 0], [1, 1], [42, 42]], [[0, 2], [0, 1], [1, 1], [-1, 0]],
                      [[0, 0], [0, 1], [0, 0], [21, 211]]], dtype=torch.float)
    sa = torch.tensor([3, 4, 2])
    B = torch.tensor([[[0, 1], [1, 2], [0, 0]]], dtype=torch.float)
    sb = torch.tensor([3])
    assert abx.get_theta_group_dtw(A, B, A, sa, sb, sa, abx.get_euclidian_distance_batch, True) == 0.5


def test_command_line_from_pre_computed(fixture_set, tmp_path):
    meta, _, _, item, seq, tmp = fixture_set
    out = tmp_path / "out"
    scores = abx.main(["from_pre_computed", tmp, item, "--feature_size", str(1 / meta["step_feature"]), "--out", str(out),
                       "--max_size_group", "3", "--seed", "4"])
    with open(out / "ABX_scores.json") as f:
        saved = json.load(f)
    assert saved == scores and set(saved) == {"within", "across"}
    assert json.load(open(out / "ABX_args.json"))["load"] == "from_pre_computed"
    from pathlib import Path
    from cpc_audio_amd.dataset import findAllSeqs
    found, _ = findAllSeqs(tmp, extension=".pt")
    seq_cli = [(Path(x).stem, str(Path(tmp) / x)) for _, x in found]
    direct = abx.ABX(lambda p: torch.load(p, map_location="cpu"), item, seq_cli, "cosine", meta["step_feature"],
                     ["within", "across"], max_size_group=3, seed=4)
    for k in ("within", "across"):
        assert math.isclose(direct[k], scores[k], abs_tol=1e-6)
