"""ABX host side (cpc_audio_amd/abx.py) without a GPU: item loading, grouping, ABXFeatureLoader and the within iterator on the
reference's own test data (the known answers of its cpc/eval/ABX/unit_tests.py), the planner's draws and the score reduction
against the reference's outputs in tests/golden/abx.npz, and the missing CPU path."""
import os
import random

import numpy as np
import pytest
import torch

import abx_util as U
from cpc_audio_amd import abx


def _npy_feature(path):
    return torch.tensor(np.load(path)).view(1, -1, 1)


def test_get_features_group_known_answers():
    idx, groups = abx.get_features_group([[0], [1], [2], [3], [4], [2], [2], [2]], [0])
    assert idx == [0, 1, 2, 5, 6, 7, 3, 4]
    assert groups == [(0, 1), (1, 2), (2, 6), (6, 7), (7, 8)]
    data = [[0, 1], [1, 2], [2, 3], [3, 3], [4, 0], [2, 2], [4, 2], [2, 2], [0, 3]]
    idx, groups = abx.get_features_group(data, [1, 0])
    assert idx == [4, 0, 1, 5, 7, 6, 8, 2, 3]
    assert groups == [[(0, 1)], [(1, 2)], [(2, 3), (3, 5), (5, 6)], [(6, 7), (7, 8), (8, 9)]]
    data = [[0, 0, 0, 1], [41, 1, 0, 2], [-23, 0, 3, 1], [220, 1, -2, 3], [40, 2, 1, 0], [200, 0, 0, 1]]
    idx, groups = abx.get_features_group(data, [1, 3, 2])
    assert idx == [0, 5, 2, 1, 3, 4]
    assert groups == [[[(0, 2), (2, 3)]], [[(3, 4)], [(4, 5)]], [[(5, 6)]]]


def test_load_item_file_known_answers():
    out, ctx, ph, spk = abx.load_item_file(os.path.join(U.TEST_DATA, "dummy_item_file.item"))
    assert ph == {"n": 0, "d": 1, "ih": 2, "s": 3, "dh": 4}
    assert spk == {"8193": 0, "2222": 1, "12": 2}
    assert ctx == {"ae+d": 0, "n+l": 1, "l+n": 2, "ih+s": 3, "n+ax": 4, "ax+dh": 5, "s+ax": 6}
    assert out == {"2107": [[0.3225, 0.5225, 0, 0, 0], [0.4225, 0.5925, 1, 1, 1], [1.1025, 1.2925, 6, 4, 2]],
                   "42": [[0.4525, 0.6525, 1, 1, 1], [0.5225, 0.7325, 2, 2, 0], [0.5925, 0.8725, 3, 0, 0]],
                   "23": [[0.6525, 1.1025, 4, 3, 0], [0.7325, 1.1925, 4, 3, 1]],
                   "407": [[0.8725, 1.2425, 5, 3, 1]]}
    out, _, _, _ = abx.load_item_file(os.path.join(U.TEST_DATA, "dummy_item_within.item"))
    assert out == {"2107": [[0., 0.2, 0, 0, 0], [0.3225, 0.5225, 1, 0, 0], [0.6, 0.75, 1, 0, 0], [0.4225, 0.5925, 2, 1, 1]],
                   "42": [[0.4525, 0.6525, 2, 1, 1], [0.1301, 0.2501, 2, 2, 1], [0.5225, 0.7325, 2, 1, 0],
                          [0.0025, 0.3561, 3, 1, 1], [0.5925, 0.8725, 3, 1, 0]]}


def test_feature_loader_and_within_iterator_known_answers():
    seq = [(k, os.path.join(U.TEST_DATA, f"{k}.npy")) for k in ("2107", "42", "23", "407")]
    ds = abx.ABXFeatureLoader(os.path.join(U.TEST_DATA, "dummy_item_file.item"), seq, _npy_feature, 10, False)
    assert ds.feature_dim == 1 and len(ds) == 9 and ds.data.dim() == 2 and len(ds.data) == 16
    data, size, coords = ds[0]
    assert (size, coords, data.tolist()) == (1, (0, 0, 0), [[3]])
    data, size, coords = ds[3]
    assert (size, coords, data.tolist()) == (1, (1, 1, 1), [[5]])

    ds = abx.ABXFeatureLoader(os.path.join(U.TEST_DATA, "dummy_item_within.item"), seq[:2], _npy_feature, 10, False)
    it = ds.get_iterator("within", 40)
    assert it.index_csp == [0, 1, 2, 6, 3, 4, 5, 8, 7]
    assert it.groups_csp == [[[(0, 1)]], [[(1, 3)]], [[(3, 4)], [(4, 6), (6, 7)]], [[(7, 8)], [(8, 9)]]]
    assert len(it) == 1
    g = iter(it)
    c, (a, sa), (b, sb), (x, sx) = next(g)
    assert c == (1, 1, 2, 2)
    assert sa.tolist() == [1, 1] and a.tolist() == [[[4.]], [[5.]]]
    assert x.tolist() == a.tolist() and sx.tolist() == sa.tolist()
    assert b.tolist() == [[[1.]]] and sb.item() == 1
    assert next(g, False) is False
    assert it.get_board_size() == (2, 3, 3, 4)


def test_normalize_with_singularity():
    x = torch.tensor([[[1., 0., 0., 0.], [0., 0., 0., 0.]], [[0., 0., -1., 0.], [0.5, -0.5, 0.5, -0.5]]])
    keep = x.clone()
    y = abx.normalize_with_singularity(x)
    assert torch.equal(x, keep)
    assert y.shape == (2, 2, 5)
    assert torch.allclose(y[0, 1, :4], torch.full((4,), 0.5)) and y[0, 1, 4].item() == np.float32(-2e12)
    assert y[0, 0, 4].item() == pytest.approx(1e-12) and torch.allclose(y[1, 1, :4].norm(), torch.tensor(1.0))


@pytest.fixture(scope="module")
def fixture_set(tmp_path_factory):
    meta, arrays = U.load_golden()
    tmp = str(tmp_path_factory.mktemp("abx"))
    feats = U.file_features(meta["item_text"])
    item, seq = U.write_fixture_files(tmp, meta["item_text"], feats)
    ds = abx.ABXFeatureLoader(item, seq, lambda p: torch.load(p, map_location="cpu"), meta["step_feature"], True)
    return meta, arrays, ds


def test_fixture_set_covers_the_edge_cases(fixture_set):
    _, arrays, ds = fixture_set
    sizes = np.asarray(ds.features)[:, 1]
    assert sizes.min() == 1 and sizes.max() > 128
    assert (ds.data[:, :-1] == 1 / 16).all(dim=1).any()          # the null frame
    assert np.array_equal(np.asarray(ds.features, dtype=np.int64), arrays["features"])


@pytest.mark.parametrize("name", ["within:sampled", "within:full", "across:sampled", "across:full"])
def test_planner_draws_as_the_reference(fixture_set, name):
    meta, arrays, ds = fixture_set
    mode = name.split(":")[0]
    case = meta["cases"][name]
    random.seed(case["seed"])
    if mode == "within":
        plan = abx.plan_within(ds, case["max_size_group"])
    else:
        plan = abx.plan_across(ds, case["max_size_group"], 5)
    assert list(plan.board) == case["board"]
    assert np.array_equal(plan.coords, arrays[f"{name}:coords"])
    assert plan.a == U.csr(arrays, f"{name}:A")
    assert plan.b == U.csr(arrays, f"{name}:B")
    assert plan.x == U.csr(arrays, f"{name}:X")
    # a private generator with the same seed draws the same
    again = abx.plan_within(ds, case["max_size_group"], seed=case["seed"]) if mode == "within" else \
        abx.plan_across(ds, case["max_size_group"], 5, seed=case["seed"])
    assert again.a == plan.a and again.b == plan.b and again.x == plan.x


@pytest.mark.parametrize("name", ["within:sampled", "within:full", "across:sampled", "across:full"])
def test_reduction_reproduces_the_reference(fixture_set, name):
    meta, arrays, ds = fixture_set
    case = meta["cases"][name]
    plan = abx.Plan(name.split(":")[0], name.startswith("within"), case["board"], arrays[f"{name}:coords"], [], [], [])
    got = abx.reduce_scores(plan, arrays[f"{name}:score"])
    assert abs(got - case["score"]) < 1e-6
    assert got == abx.reduce_scores(plan, arrays[f"{name}:score"])


def test_theta_rounding_matches_the_reference(fixture_set):
    _, arrays, _ = fixture_set
    for name in ("within:sampled", "across:sampled"):
        for k in range(3):
            dxa, dxb = torch.from_numpy(arrays[f"{name}:dxa{k}"]), torch.from_numpy(arrays[f"{name}:dxb{k}"])
            theta = abx.theta_from_distances(dxa, dxb, name.startswith("within"))
            assert np.float32(1 - theta) == arrays[f"{name}:score"][k]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a GPU")
def test_abx_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        abx.ABX(lambda p: None, os.path.join(U.TEST_DATA, "dummy_item_file.item"), [], "cosine", 100, ["within"])
