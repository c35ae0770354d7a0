"""Linear-separability evaluation without a GPU: the parser against the reference's recorded namespaces, run() on a pass-through
feature maker with 128-wide criteria (their torch path) against the files the reference's run() wrote (tests/golden/linsep_meta.json,
tools/make_golden_linsep.py), the log averages, and the probe entry points' declarations and argument checks."""
import ctypes
import json
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

import linsep_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SYMBOLS = ("cpc_probe_layout", "cpc_probe_train_step", "cpc_probe_eval")


def _meta():
    with open(os.path.join(ROOT, "tests", "golden", "linsep_meta.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(U.ARGV))
def test_parse_args_matches_the_reference(name):
    from cpc_audio_amd import linear_separability as LS
    assert vars(LS.parse_args(list(U.ARGV[name]))) == _meta()["args"][name]


def test_parse_args_post_processing():
    from cpc_audio_amd import linear_separability as LS
    args = LS.parse_args(["db", "train.txt", "val.txt", "a.pt", "--n_epoch", "7", "--pathCheckpoint", "rel/out"])
    assert args.nGPU == 1 and args.save_step == 7                      # nGPU < 0 -> 1; save_step <= 0 -> n_epoch
    assert args.load == [os.path.abspath("a.pt")] and args.pathCheckpoint == os.path.abspath("rel/out")
    assert LS.parse_args(["db", "t", "v", "--save_step", "3"]).save_step == 3


def _run(case, tmp_path, n_train=U.N_TRAIN, epochs=U.N_EPOCHS, dim=128):
    """run() on CPU tensors: 128-wide criteria are on the torch path, optim.Adam hands CPU parameters to torch's update."""
    from cpc_audio_amd import criterion as C, linear_separability as LS, optim
    crit = U.build(C, case, dim=dim)
    assert not crit.hip_path
    train, val = U.batches(case, dim=dim)
    train = train[:n_train]
    steps = []
    crit.register_forward_hook(lambda m, i, o: steps.append((float(o[0].detach().mean()), float(o[1].detach().mean()), m.training)))
    opt = optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    logs = {"epoch": [], "iter": [], "saveStep": epochs}
    LS.run(U.PassThrough(), crit, train, val, opt, logs, epochs, str(tmp_path / "checkpoint"))
    return logs, steps, len(train), len(val)


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_run_writes_the_files_of_the_reference(case, tmp_path):
    ref = _meta()["cases"][case]
    logs, steps, n_train, n_val = _run(case, tmp_path)
    assert sorted(os.listdir(tmp_path)) == ref["files"]
    state = torch.load(tmp_path / f"checkpoint_{U.N_EPOCHS - 1}.pt", map_location="cpu", weights_only=False)
    tree = U.key_tree(state)

    def narrow(t):      # the fixture's criterion is 256 wide, this one 128: the same tree but for that dimension
        return json.loads(re.sub(r"\b256\b", "128", json.dumps(t)))

    assert tree == narrow(ref["checkpoint"])
    with open(tmp_path / "checkpoint_logs.json") as f:
        written = json.load(f)
    assert written == json.loads(json.dumps(logs))
    assert sorted(written) == sorted(ref["logs"])
    for key, value in ref["logs"].items():
        assert np.shape(written[key]) == np.shape(value), key
    assert written["epoch"] == ref["logs"]["epoch"] and written["iter"] == ref["logs"]["iter"] == [n_train - 1] * U.N_EPOCHS
    assert written["saveStep"] == ref["logs"]["saveStep"]
    # the averages divide by the number of batches (the reference: by the last step index)
    per_epoch = n_train + n_val
    for e in range(U.N_EPOCHS):
        tr = steps[e * per_epoch:e * per_epoch + n_train]
        va = steps[e * per_epoch + n_train:(e + 1) * per_epoch]
        assert all(s[2] for s in tr) and not any(s[2] for s in va)
        for key, part, col in (("locLoss_train", tr, 0), ("locAcc_train", tr, 1), ("locLoss_val", va, 0), ("locAcc_val", va, 1)):
            mean = sum(s[col] for s in part) / len(part)
            assert written[key][e][0] == pytest.approx(mean, rel=1e-6), (key, e)
            if key.endswith("train"):       # and not the reference's N / (N - 1) scaling
                assert abs(written[key][e][0] - mean * n_train / (n_train - 1)) > 1e-3 * abs(mean)


def test_an_epoch_of_one_batch_gives_finite_logs(tmp_path):
    logs, steps, _, _ = _run("speaker", tmp_path, n_train=1, epochs=1)
    assert logs["iter"] == [0]
    for key in ("locLoss_train", "locAcc_train", "locLoss_val", "locAcc_val"):
        assert len(logs[key]) == 1 and len(logs[key][0]) == 1 and math.isfinite(logs[key][0][0]), key
    assert logs["locLoss_train"][0][0] == pytest.approx(steps[0][0], rel=1e-6)


def test_save_rule_and_best_state(tmp_path):
    from cpc_audio_amd import criterion as C, linear_separability as LS, optim
    crit = U.build(C, "speaker", dim=128)
    train, val = U.batches("speaker", dim=128)
    opt = optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    logs = {"epoch": [], "iter": [], "saveStep": 2}
    LS.run(U.PassThrough(), crit, train[:2], val[:1], opt, logs, 4, str(tmp_path / "checkpoint"))
    # (epoch % saveStep == 0 and epoch > 0) or the last epoch: 2 and 3, not 0
    assert sorted(os.listdir(tmp_path)) == ["checkpoint_2.pt", "checkpoint_3.pt", "checkpoint_logs.json"]
    state = torch.load(tmp_path / "checkpoint_3.pt", map_location="cpu", weights_only=False)
    assert state["optimizer"]["state"][0]["step"] == 8 and state["best"] == {}


def test_more_than_one_checkpoint_raises(tmp_path):
    from cpc_audio_amd import linear_separability as LS
    with pytest.raises(ValueError, match="concatenated models"):
        LS.main([str(tmp_path), "train.txt", "val.txt", "a.pt", "b.pt", "--pathCheckpoint", str(tmp_path / "out")])


def test_module_docstring_states_the_two_differences():
    from cpc_audio_amd import linear_separability as LS
    assert "Log averages" in LS.__doc__ and "No per-step host reads" in LS.__doc__ and LS.FUSED_PROBE is True


def test_probe_symbols_are_declared_and_in_the_signature_table():
    from cpc_audio_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in PROBE_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _lib.SIGNATURES
    assert _lib.EXPECTED_ABI == 16                                      # adding symbols is compatible
    assert len(_lib.SIGNATURES["cpc_probe_train_step"][1]) == 24 and len(_lib.SIGNATURES["cpc_probe_eval"][1]) == 12


def _product_library():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    return _lib.bind(build.build())


def test_probe_symbols_are_exported_by_a_gfx950_build():
    lib = _product_library()
    for name in PROBE_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.cpc_abi_version() == 16


def test_probe_argument_and_shape_errors_answer_without_a_device():
    lib = _product_library()
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_probe_layout(1024, 41, sizes) == 0
    floats, slabs, rows = tuple(sizes)
    assert slabs == 32 and rows == 32 and floats >= 1024 + slabs * 41 * 257
    assert lib.cpc_probe_layout(8192, 41, sizes) == 0 and sizes[1] == 256
    for bad in [(0, 41), (4, 1), (4, 8193), (1 << 20, 4096)]:             # the range of cpc_supervised_layout
        assert lib.cpc_probe_layout(*bad, sizes) == 1, bad
    assert lib.cpc_probe_layout(4, 41, None) == 2
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    d = [2e-4, 0.9, 0.999, 2e-8, 0.1, 0.03]
    # every check sits in front of the first launch: host pointers are never dereferenced
    assert lib.cpc_probe_train_step(p, 256, p, 4, 1, p, p, p, p, p, p, *d, p, p, p, None, None, None, None) == 1
    assert lib.cpc_probe_train_step(p, 256, p, 4, 8193, p, p, p, p, p, p, *d, p, p, p, None, None, None, None) == 1
    assert lib.cpc_probe_train_step(None, 256, p, 4, 41, p, p, p, p, p, p, *d, p, p, p, None, None, None, None) == 2
    assert lib.cpc_probe_train_step(p, 255, p, 4, 41, p, p, p, p, p, p, *d, p, p, p, None, None, None, None) == 2
    assert lib.cpc_probe_train_step(p, 256, p, 4, 41, p, p, p, None, p, p, *d, p, p, p, None, None, None, None) == 2
    assert lib.cpc_probe_train_step(p, 256, p, 4, 41, p, p, p, p, p, p, *d, None, p, p, None, None, None, None) == 2
    assert lib.cpc_probe_train_step(p, 256, p, 4, 41, p, p, p, p, p, p, *d[:4], 0.0, 0.03, p, p, p, None, None, None, None) == 2
    assert lib.cpc_probe_eval(p, 256, p, 0, 41, p, p, p, p, p, None, None) == 1
    assert lib.cpc_probe_eval(p, 256, None, 4, 41, p, p, p, p, p, None, None) == 2
    assert lib.cpc_probe_eval(p, 256, p, 4, 41, p, p, p + 4, p, p, None, None) == 2      # workspace not 16-byte aligned
    assert bool((buf == 0).all())
