"""Linear-separability evaluation on an MI355X: the fixture's phone and speaker runs (tests/golden/linsep.npz: the float64
reference's per-step losses, accuracies and 20-step update, tools/make_golden_linsep.py) through train_step / val_step with the
fused probe step and without it, the optimiser state after fused steps, and the command end to end on a small seeded corpus.

Bounds: per-step loss within 1e-5 relative; accuracies equal (the fixture has no row with a top-2 margin under 1e-5 of its
scale); update after 20 steps within 4 x the deviation the float32 REFERENCE itself shows from its float64 run (recorded in
linsep_meta.json) -- both are fp32 evaluations of the same 20-step recurrence, where parameter rounding dominates."""
import json
import os
import random
import wave

import numpy as np
import pytest
import torch

import linsep_util as U
from cpc_audio_amd import criterion as C, harness, linear_separability as LS, ops, optim, train

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "linsep_meta.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(ROOT, "tests", "golden", "linsep.npz"))


@pytest.fixture
def fused_flag():
    keep = LS.FUSED_PROBE
    yield
    LS.FUSED_PROBE = keep


def _fixture_run(case, fused):
    """The fixture's 20 training and 3 validation batches, one batch per train_step / val_step call so that every step's loss
    and accuracy come back through the logs.  -> (steps (23, 2), update of [W, b], optimiser, criterion)."""
    LS.FUSED_PROBE = fused
    crit = U.build(C, case, device="cuda")
    assert crit.hip_path
    train_b, val_b = U.batches(case, device="cuda")
    W, b = U.parameters_of(crit, case)
    W0, b0 = W.detach().clone(), b.detach().clone()
    opt = optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    fm = U.PassThrough()
    steps = []
    for batch in train_b:
        logs = LS.train_step(fm, crit, [batch], opt)
        assert logs["iter"] == 0
        steps.append((logs["locLoss_train"][0], logs["locAcc_train"][0]))
    update = torch.cat([(W.detach() - W0).reshape(-1), b.detach() - b0]).double().cpu()
    for batch in val_b:
        logs = LS.val_step(fm, crit, [batch])
        steps.append((logs["locLoss_val"][0], logs["locAcc_val"][0]))
    return np.array(steps), update, opt, crit


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", sorted(U.CASES))
def test_fixture_runs_match_the_float64_reference(case, fused, fused_flag, monkeypatch):
    meta, gold = _golden()
    calls = {"train": 0, "eval": 0}
    real_train, real_eval = ops.probe_train_step, ops.probe_eval
    monkeypatch.setattr(ops, "probe_train_step", lambda *a, **k: (calls.__setitem__("train", calls["train"] + 1), real_train(*a, **k))[1])
    monkeypatch.setattr(ops, "probe_eval", lambda *a, **k: (calls.__setitem__("eval", calls["eval"] + 1), real_eval(*a, **k))[1])
    steps, update, opt, _ = _fixture_run(case, fused)
    assert calls == ({"train": U.N_TRAIN, "eval": U.N_VAL} if fused else {"train": 0, "eval": 0})     # the path that was asked for
    ref = gold[f"{case}:steps"]
    rel = np.abs(steps[:, 0] - ref[:, 0]) / np.abs(ref[:, 0])
    ref_update = torch.cat([torch.from_numpy(gold[f"{case}:dW"]).reshape(-1), torch.from_numpy(gold[f"{case}:db"])])
    dev = ((update - ref_update).norm() / ref_update.norm()).item()
    bound = 4 * meta["cases"][case]["fp32_update_deviation"]
    print(f"{case} fused={fused}: worst loss deviation {rel.max():.3e}, update deviation {dev:.3e} (bound {bound:.3e})")
    assert meta["cases"][case]["close_margin_rows"] == 0
    assert rel.max() <= 1e-5
    assert np.array_equal(steps[:, 1], ref[:, 1])
    assert dev <= bound
    ops.check_device_errors()


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_optimizer_state_after_fused_steps_has_the_layout_of_step(case, fused_flag):
    meta, _ = _golden()
    _, upd_f, opt_f, crit_f = _fixture_run(case, True)
    _, upd_u, opt_u, _ = _fixture_run(case, False)
    sd_f, sd_u = opt_f.state_dict(), opt_u.state_dict()
    assert sorted(sd_f) == sorted(sd_u) and sd_f["param_groups"] == sd_u["param_groups"]
    assert sorted(sd_f["state"]) == sorted(sd_u["state"]) == [0, 1]
    for i in (0, 1):
        assert sorted(sd_f["state"][i]) == sorted(sd_u["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        assert float(sd_f["state"][i]["step"]) == float(sd_u["state"][i]["step"]) == U.N_TRAIN
        assert sd_f["state"][i]["step"].dtype == sd_u["state"][i]["step"].dtype and not sd_f["state"][i]["step"].is_cuda
        for k in ("exp_avg", "exp_avg_sq"):
            a, b = sd_f["state"][i][k], sd_u["state"][i][k]
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
            assert ((a - b).norm() / b.norm()).item() < 1e-4
    # the reference's checkpoint layout for the "optimizer" entry, apart from the step count of a 2-epoch run
    ref = meta["cases"][case]["checkpoint"]
    tree = U.key_tree({"gEncoder": {}, "best": {}, "cpcCriterion": crit_f.state_dict(), "optimizer": sd_f})
    for key in ("cpcCriterion", "optimizer", "optimizer.param_groups", "optimizer.params"):
        assert tree[key] == ref[key], key
    assert {i: sorted(v) for i, v in tree["optimizer.state"].items()} == {i: sorted(v) for i, v in ref["optimizer.state"].items()}
    # and a plain step() continues from it
    opt_f.zero_grad()
    W, b = U.parameters_of(crit_f, case)
    (W.sum() + b.sum()).backward()
    opt_f.step()
    assert float(opt_f.state_dict()["state"][0]["step"]) == U.N_TRAIN + 1


def test_whole_epoch_equals_its_steps(fused_flag):
    """One train_step over the 20 batches: the same parameters, bit for bit, as 20 calls of one batch, and the epoch's log is
    the mean of the steps' losses (read once, from the device-side float64 sums)."""
    steps, _, _, crit_steps = _fixture_run("phone", True)
    crit = U.build(C, "phone", device="cuda")
    train_b, val_b = U.batches("phone", device="cuda")
    opt = optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    logs = LS.train_step(U.PassThrough(), crit, train_b, opt)
    assert logs["iter"] == U.N_TRAIN - 1
    for p, q in zip(crit.parameters(), crit_steps.parameters()):
        assert torch.equal(p, q)
    assert logs["locLoss_train"][0] == pytest.approx(steps[:U.N_TRAIN, 0].mean(), rel=1e-12)
    assert logs["locAcc_train"][0] == pytest.approx(steps[:U.N_TRAIN, 1].mean(), rel=1e-12)
    logs_val = LS.val_step(U.PassThrough(), crit, val_b)
    assert logs_val["locLoss_val"][0] == pytest.approx(steps[U.N_TRAIN:, 0].mean(), rel=1e-12)


def test_label_out_of_range_is_reported_at_the_end_of_the_epoch(fused_flag):
    LS.FUSED_PROBE = True
    crit = U.build(C, "speaker", device="cuda")
    train_b, _ = U.batches("speaker", device="cuda")
    x, y = train_b[0]
    y = y.clone()
    y[3] = U.N_SPEAKERS
    opt = optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    with pytest.raises(Exception, match="label outside"):
        LS.train_step(U.PassThrough(), crit, [(x, y)], opt)
    ops.check_device_errors()


# ------------------------------------------------------------------------------------------------- end to end
def _corpus(tmp_path, seed=0):
    """6 speakers x 2 files of 3 to 4 s, phone labels every 160 samples, train / val lists, a randomly initialised checkpoint."""
    rng = np.random.default_rng(seed)
    db = tmp_path / "db"
    names, phones = [], []
    for s in range(6):
        (db / f"spk{s}").mkdir(parents=True)
        for k in range(2):
            name = f"spk{s}-utt{k}"
            n = int(rng.integers(3 * 16000, 4 * 16000))
            x = (rng.uniform(-0.3, 0.3, n) * 32767).astype("<i2")
            with wave.open(str(db / f"spk{s}" / f"{name}.wav"), "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(16000)
                f.writeframes(x.tobytes())
            names.append(name)
            labels = np.repeat(rng.integers(0, 7, n // 160 // 5 + 1), 5)[:n // 160]
            phones.append(name + " " + " ".join(str(int(v)) for v in labels))
    (tmp_path / "phones.txt").write_text("\n".join(phones) + "\n")
    (tmp_path / "train.txt").write_text("\n".join(n for n in names if n.endswith("utt0")) + "\n")
    (tmp_path / "val.txt").write_text("\n".join(n for n in names if n.endswith("utt1")) + "\n")
    cdir = tmp_path / "cpc"
    cdir.mkdir()
    torch.manual_seed(seed)
    model = train.build_model(nLevelsGRU=1, arMode="GRU")
    harness.save_checkpoint(model.state_dict(), None, None, None, str(cdir / "checkpoint_0.pt"))
    (cdir / "checkpoint_args.json").write_text(json.dumps({"hiddenEncoder": 256, "hiddenGar": 256, "nLevelsGRU": 1, "arMode": "GRU"}))
    return db, cdir / "checkpoint_0.pt"


def _main(tmp_path, db, ckpt, out, phone, fused):
    LS.FUSED_PROBE = fused
    random.seed(11)
    torch.manual_seed(11)
    argv = [str(db), str(tmp_path / "train.txt"), str(tmp_path / "val.txt"), str(ckpt), "--pathCheckpoint", str(out),
            "--file_extension", ".wav", "--n_epoch", "2", "--batchSizeGPU", "4", "--ignore_cache"]
    LS.main(argv + (["--pathPhone", str(tmp_path / "phones.txt")] if phone else []))
    assert sorted(os.listdir(out)) == ["checkpoint_1.pt", "checkpoint_args.json", "checkpoint_logs.json"]
    with open(out / "checkpoint_logs.json") as f:
        logs = json.load(f)
    state = torch.load(out / "checkpoint_1.pt", map_location="cpu", weights_only=False)
    return logs, state


@pytest.mark.parametrize("phone", [False, True], ids=["speaker", "phone"])
def test_command_end_to_end(tmp_path, phone, fused_flag):
    db, ckpt = _corpus(tmp_path)
    logs_f, state_f = _main(tmp_path, db, ckpt, tmp_path / "out_fused", phone, True)
    logs_u, state_u = _main(tmp_path, db, ckpt, tmp_path / "out_unfused", phone, False)
    assert sorted(state_f) == ["best", "cpcCriterion", "gEncoder", "optimizer"]
    attr = U.CASES["phone" if phone else "speaker"][2]
    assert tuple(state_f["cpcCriterion"][f"{attr}.weight"].shape) == ((7, 256) if phone else (6, 256))
    assert sorted(state_f["gEncoder"]) == sorted(state_f["best"]) == sorted(state_u["gEncoder"])
    assert U.key_tree(state_f) == U.key_tree(state_u)
    assert state_f["optimizer"]["state"][0]["step"] == 2 * (logs_f["iter"][0] + 1)
    assert sorted(logs_f) == sorted(logs_u) == sorted(["epoch", "iter", "saveStep", "locLoss_train", "locAcc_train", "locLoss_val",
                                                         "locAcc_val"])
    assert logs_f["epoch"] == [0, 1] and logs_f["iter"] == logs_u["iter"] and logs_f["iter"][0] >= 1
    for key in ("locLoss_train", "locLoss_val", "locAcc_train", "locAcc_val"):
        a, b = np.array(logs_f[key]), np.array(logs_u[key])
        assert a.shape == b.shape == (2, 1) and np.isfinite(a).all() and np.isfinite(b).all(), key
        if "Loss" in key:
            assert (np.abs(a - b) <= 1e-5 * np.abs(b)).all(), (key, a, b)
    with open(tmp_path / "out_fused" / "checkpoint_args.json") as f:
        saved = json.load(f)
    assert saved["pathCheckpoint"] == str(tmp_path / "out_fused" / "checkpoint") and saved["nGPU"] == 1
    ops.check_device_errors()
