"""ZeroSpeech feature export end to end on an MI355X: python -m cpc_audio_amd.build_zeroSpeech_features' main() on a seeded
checkpoint (two-layer GRU, CTCPhoneCriterion(256, 41, False)) and two .wav files, against the plain composition written out here
-- FeatureModule, build_feature, the classifier's getPrediction in float64 on the CPU, then torch softmax / argmax.  Features
must be bit-equal, posteriors within 4 x f32_dev of tests/golden/zerospeech_meta.json (tests/test_emu_posterior.py), one-hot text
equal, no frame having a top-2 logit margin under 1e-4 of its scale."""
import json
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import zerospeech_util as U
from cpc_audio_amd import build_zeroSpeech_features as Z, criterion as C, dataset, harness, ops, train

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = {"utt_long": ("spk0", 64000 + 12345), "utt_short": ("", 8000)}
STEP = 160 / 16000


def _f32_dev():
    with open(os.path.join(ROOT, "tests", "golden", "zerospeech_meta.json")) as f:
        return json.load(f)["f32_dev"]


def _write_wav(path, n, seed):
    g = torch.Generator().manual_seed(seed)
    pcm = ((0.1 * torch.randn(n, generator=g)).clamp_(-1, 1) * 32767).round().to(torch.int16).numpy()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.astype("<i2").tobytes())


def _seeded_criterion(seed):
    crit = C.CTCPhoneCriterion(256, U.N_PHONES, False)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        crit.PhoneCriterionClassifier.weight.copy_((2 * torch.rand(U.N_PHONES + 1, 256, generator=g) - 1) / 16)
        crit.PhoneCriterionClassifier.bias.copy_((2 * torch.rand(U.N_PHONES + 1, generator=g) - 1) / 16)
    return crit


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The files, the checkpoint and the plain composition's results, computed once: per file and chunking (strict or not) the
    features (frames, 256) and the classifier's float64 logits."""
    root = tmp_path_factory.mktemp("zerospeech")
    db, ckpt_dir = str(root / "db"), str(root / "ckpt")
    for k, (stem, (sub, n)) in enumerate(FILES.items()):
        _write_wav(os.path.join(db, sub, stem + ".wav"), n, seed=50 + k)
    torch.manual_seed(11)
    model = train.build_model(arMode="GRU", nLevelsGRU=2)
    fm = harness.FeatureModule(model, False).cuda().eval()
    feats = {}
    for stem, (sub, _) in FILES.items():
        wav = dataset.loadFile((0, os.path.join(db, sub, stem + ".wav")))[2].view(1, -1)
        for strict in (False, True):
            feats[stem, strict] = harness.build_feature(fm, wav, strict=strict, max_size_seq=64000)[0]
    # a seeded classifier under which no frame's argmax hangs on the last bits (the first seed that gives none)
    for seed in range(20):
        crit = _seeded_criterion(seed)
        lin = crit.PhoneCriterionClassifier
        logits = {k: F.linear(f.double(), lin.weight.detach().double(), lin.bias.detach().double()) for k, f in feats.items()}
        if sum(U.close_rows(l) for l in logits.values()) == 0:
            break
    else:
        raise AssertionError("no seeded classifier without a close top-2 margin")
    os.makedirs(ckpt_dir)
    with open(os.path.join(ckpt_dir, "checkpoint_args.json"), "w") as f:
        json.dump({"arMode": "GRU", "nLevelsGRU": 2, "hiddenGar": 256, "hiddenEncoder": 256, "CTC": True, "onEncoder": False}, f)
    path = os.path.join(ckpt_dir, "checkpoint_4.pt")
    harness.save_checkpoint(model.state_dict(), crit.state_dict(), None, None, path)
    return {"root": root, "db": db, "checkpoint": path, "features": feats, "logits": logits}


def _run(corpus, name, *options):
    out = str(corpus["root"] / name)
    maker = Z.main([corpus["db"], out + os.sep, corpus["checkpoint"], *options])
    with open(out + ".json") as f:
        saved = json.load(f)
    assert saved == vars(Z.parse_args([corpus["db"], out + os.sep, corpus["checkpoint"], *options]))
    ops.check_device_errors()
    return out, maker, saved


def test_features_as_npy_are_the_bits_of_build_feature(corpus):
    out, maker, saved = _run(corpus, "features", "--format", "npy")
    assert isinstance(maker, harness.FeatureModule) and saved["format"] == "npy" and saved["addCriterion"] is False
    assert sorted(os.listdir(out)) == sorted(stem + ".npy" for stem in FILES)
    for stem in FILES:
        got = np.load(os.path.join(out, stem + ".npy"))
        ref = corpus["features"][stem, False].numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape == (FILES[stem][1] // 160, 256)
        assert np.array_equal(got, ref), stem


@pytest.mark.parametrize("options,path", [((), "hip"), (("--hipHead",), "hip"), (("--no-hipHead",), "torch")])
def test_posteriors_as_npz(corpus, options, path):
    out, maker, saved = _run(corpus, "posteriors_" + path + str(len(options)), "--addCriterion", "--format", "npz", *options)
    assert isinstance(maker, harness.ModelPhoneCombined) and maker.last_path == path
    assert saved["hipHead"] == {(): None, ("--hipHead",): True, ("--no-hipHead",): False}[options]
    for stem in FILES:
        ref = torch.softmax(corpus["logits"][stem, False], dim=1)
        with np.load(os.path.join(out, stem + ".npz")) as z:
            assert sorted(z.files) == ["features", "time", "totTime"]
            got, time, tot = z["features"], z["time"], z["totTime"]
        n = ref.shape[0]
        assert got.dtype == np.float32 and got.shape == (n, U.N_PHONES + 1)
        assert time.dtype == np.float64 and np.array_equal(time, np.array([STEP / 2 + k * STEP for k in range(n)]))
        assert tot.dtype == np.float32 and np.array_equal(tot, np.array([STEP * n], dtype=np.float32))
        err = np.abs(got.astype(np.float64) - ref.numpy()).max()
        print(f"{stem} ({path}): max abs err {err:.3e} (bound {4 * _f32_dev():.3e})")
        assert err <= 4 * _f32_dev()
        assert np.abs(got.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6


def test_one_hot_as_strict_fea_text(corpus):
    out, maker, saved = _run(corpus, "one_hot", "--addCriterion", "--oneHot", "--format", "fea", "--strict")
    assert maker.last_path == "hip" and maker.oneHot is True and saved["strict"] is True
    for stem in FILES:
        logits = corpus["logits"][stem, True]
        assert U.close_rows(logits) == 0
        hot = F.one_hot(logits.argmax(dim=1), U.N_PHONES + 1).tolist()
        text = "".join(" ".join(map(str, [STEP / 2 + k * STEP] + row)) + "\n" for k, row in enumerate(hot))
        with open(os.path.join(out, stem + ".fea")) as f:
            assert f.read() == text, stem


def test_the_hip_call_is_what_the_torch_ops_give(corpus):
    """ModelPhoneCombined on one batch of features, both paths: the same one-hot, posteriors within the two paths' bounds."""
    crit = harness.loadSupervisedCriterion(corpus["checkpoint"])[0].cuda()
    c = torch.stack([corpus["features"]["utt_short", False]] * 2).cuda()
    outs = {}
    for hip in (True, False):
        for one_hot in (False, True):
            m = harness.ModelPhoneCombined(U.Features(), crit, one_hot, hipHead=hip)
            outs[hip, one_hot] = m(c)
            assert m.last_path == ("hip" if hip else "torch") and tuple(outs[hip, one_hot].shape) == (2, 50, U.N_PHONES + 1)
    assert torch.equal(outs[True, True], outs[False, True]) and outs[True, True].dtype == torch.int64
    assert (outs[True, False].double() - outs[False, False].double()).abs().max().item() <= 8 * _f32_dev()
