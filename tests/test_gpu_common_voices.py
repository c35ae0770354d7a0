"""The CommonVoice phone-recognition pipeline on an MI355X: CTCphone_criterion against the fixture on the device, and `train`
for 2 epochs then `per`, end to end on small synthetic sets -- through IDModule (pre-computed features) and through a small CPC
checkpoint with utterances of several seconds."""
import json
import math
import wave

import numpy as np
import pytest
import torch

import per_util as U
from cpc_audio_amd import common_voices_eval as CV, harness, train

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(4))
def test_ctc_phone_criterion_on_device_matches_fixture(k):
    meta, arrays = U.load_golden()
    case = meta["ctc"][k]
    crit = CV.CTCphone_criterion(16, 6, case["LSTM"], seqNorm=case["seqNorm"], reduction="sum").cuda().eval()
    crit.load_state_dict({n: torch.from_numpy(arrays[f"ctc{k}:sd:{n}"]) for n in case["keys"]})
    x = torch.from_numpy(arrays[f"ctc{k}:x"]).cuda()
    fs = torch.tensor(case["feature_size"], device="cuda")
    with torch.no_grad():
        pred = crit.getPrediction(x, fs)
        loss = crit(x, fs, torch.from_numpy(arrays[f"ctc{k}:label"]).cuda(), torch.tensor(case["label_size"], device="cuda"))
    assert (pred.cpu() - torch.from_numpy(arrays[f"ctc{k}:pred"])).abs().max() < 1e-4
    assert abs(loss.item() - case["loss"]) < 1e-4 * max(1.0, abs(case["loss"]))


def _phones(path, names, rng, n_phones=5):
    """Phone transcriptions, and the validation list (the reference's `per` reads it back from args_training.json)."""
    (path.parent / "val.txt").write_text("\n".join(names[:3]) + "\n")
    with open(path, "w") as f:
        for n in names:
            f.write(n + " " + " ".join(str(int(x)) for x in rng.integers(0, n_phones, int(rng.integers(3, 12)))) + "\n")


def _check_run(out, result):
    ckpt = torch.load(out / "checkpoint.pt", map_location="cpu")
    assert set(ckpt) == {"classifier", "model", "bestLoss"}
    assert all(k.startswith("module.") for k in ckpt["classifier"]) and all(k.startswith("module.") for k in ckpt["model"])
    assert "module.PhoneCriterionClassifier.weight" in ckpt["classifier"]
    mean, std = result
    assert math.isfinite(mean) and math.isfinite(std) and mean >= 0
    for f in ("args_training.json", "args_validation_0.json", "logs_train.txt", "logs_per_0.txt"):
        assert (out / f).exists(), f
    assert "Average PER" in (out / "logs_per_0.txt").read_text()


def test_train_then_per_on_precomputed_features(tmp_path):
    rng = np.random.default_rng(0)
    db = tmp_path / "db"
    db.mkdir()
    names = [f"s{k:02d}" for k in range(20)]
    for n in names:
        np.save(db / f"{n}.npy", rng.standard_normal((8, int(rng.integers(120, 400)))).astype(np.float32))
    _phones(tmp_path / "phones.txt", names, rng)
    out = tmp_path / "out"
    torch.manual_seed(0)
    assert CV.main(["train", str(db), str(tmp_path / "phones.txt"), "ID", "-o", str(out), "--nEpochs", "2", "--batchSize", "4",
                    "--in_dim", "8", "--file_extension", ".npy", "--pathVal", str(tmp_path / "val.txt")]) is None
    result = CV.main(["per", str(out)])
    _check_run(out, result)


def test_train_then_per_through_a_cpc_checkpoint(tmp_path):
    rng = np.random.default_rng(1)
    db = tmp_path / "db"
    db.mkdir()
    names = [f"u{k:02d}" for k in range(10)]
    for n in names:
        x = (rng.uniform(-0.3, 0.3, int(rng.integers(2 * 16000, 4 * 16000))) * 32767).astype("<i2")
        with wave.open(str(db / f"{n}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(x.tobytes())
    _phones(tmp_path / "phones.txt", names, rng)
    cdir = tmp_path / "cpc"
    cdir.mkdir()
    torch.manual_seed(1)
    model = train.build_model(nLevelsGRU=1, arMode="GRU")
    harness.save_checkpoint(model.state_dict(), None, None, None, str(cdir / "checkpoint_0.pt"))
    (cdir / "checkpoint_args.json").write_text(json.dumps({"hiddenEncoder": 256, "hiddenGar": 256, "nLevelsGRU": 1,
                                                           "arMode": "GRU"}))
    out = tmp_path / "out"
    assert CV.main(["train", str(db), str(tmp_path / "phones.txt"), str(cdir / "checkpoint_0.pt"), "-o", str(out),
                    "--nEpochs", "2", "--batchSize", "4", "--file_extension", ".wav", "--freeze",
                    "--pathVal", str(tmp_path / "val.txt")]) is None
    result = CV.main(["per", str(out)])
    _check_run(out, result)
