"""ZeroSpeech feature export without a GPU: buildAllFeature, ModelPhoneCombined (torch path), toOneHot and the parser against
what the reference wrote and returned (tests/golden/zerospeech.npz + zerospeech_meta.json, tools/make_golden_zerospeech.py; inputs
in zerospeech_util), and the checkpoint loaders on temporary checkpoints."""
import json
import os

import numpy as np
import pytest
import torch

import zerospeech_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _gold():
    if not _cache:
        with open(os.path.join(ROOT, "tests", "golden", "zerospeech_meta.json")) as f:
            _cache["meta"] = json.load(f)
        with np.load(os.path.join(ROOT, "tests", "golden", "zerospeech.npz")) as z:
            _cache["arrays"] = {k: z[k] for k in z.files}
    return _cache["arrays"], _cache["meta"]


@pytest.fixture
def memory_files():
    """Files of extension zerospeech_util.EXTENSION are read from memory."""
    from cpc_audio_amd import dataset
    dataset.register_reader(U.EXTENSION, lambda path: U.waveform(os.path.splitext(os.path.basename(str(path)))[0])[0])
    yield
    dataset._READERS.pop(U.EXTENSION, None)


# ------------------------------------------------------------------------------------------------ (a) the files written
@pytest.mark.parametrize("fmt", U.FORMATS)
@pytest.mark.parametrize("norm", [False, True])
def test_build_all_feature_writes_the_files_of_the_reference(fmt, norm, tmp_path, memory_files):
    from cpc_audio_amd.build_zeroSpeech_features import buildAllFeature
    arrays, _ = _gold()
    buildAllFeature(U.Recorder(), "/nowhere", str(tmp_path), U.SEQ_LIST, stepSize=U.STEP_SIZE, strict=False,
                    maxSizeSeq=U.MAX_SIZE_SEQ, format=fmt, seqNorm=norm)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{stem}.{fmt}" for stem in U.FILES)
    for stem in U.FILES:
        path, key = tmp_path / f"{stem}.{fmt}", f"a:{int(norm)}:{stem}:{fmt}"
        if fmt == "fea":
            assert path.read_bytes() == arrays[key].tobytes(), (stem, norm)              # byte for byte
        elif fmt == "npy":
            got = np.load(path)
            assert got.dtype == arrays[key].dtype == np.float32 and got.shape == arrays[key].shape
            assert np.array_equal(got, arrays[key]), (stem, norm)
        else:
            with np.load(path) as z:
                assert sorted(z.files) == ["features", "time", "totTime"]
                for k in z.files:
                    ref = arrays[f"{key}:{k}"]
                    assert z[k].dtype == ref.dtype and z[k].shape == ref.shape, (k, z[k].dtype, ref.dtype)
                    assert np.array_equal(z[k], ref), (stem, norm, k)


def test_formats_outside_the_three_are_refused(tmp_path):
    from cpc_audio_amd.build_zeroSpeech_features import buildAllFeature
    with pytest.raises(ValueError):
        buildAllFeature(U.Recorder(), "/nowhere", str(tmp_path), [], format="af")


# ------------------------------------------------------------------------------------------------ (b), (c) the modules
@pytest.mark.parametrize("case", sorted(U.CRITERIA))
def test_model_phone_combined_matches_the_reference_on_torch_ops(case):
    from cpc_audio_amd import criterion as C
    from cpc_audio_amd.harness import ModelPhoneCombined
    arrays, meta = _gold()
    ref, ref_hot = torch.from_numpy(arrays[f"b:{case}:posteriors"]), torch.from_numpy(arrays[f"b:{case}:one_hot"])
    assert meta["posteriors"][case]["close_margin_rows"] == 0
    with torch.no_grad():
        m64 = ModelPhoneCombined(U.Features(), U.build(C, case, dtype=torch.float64), False, hipHead=False)
        p64 = m64(U.features(torch.float64))
        m32 = ModelPhoneCombined(U.Features(), U.build(C, case), False, hipHead=False)
        p32 = m32(U.features())
        hot = ModelPhoneCombined(U.Features(), U.build(C, case), True, hipHead=False)(U.features())
        auto = ModelPhoneCombined(U.Features(), U.build(C, case), False)                # hipHead=None: CPU tensors -> torch
        assert torch.equal(auto(U.features()), p32) and auto.last_path == "torch"
    assert m64.last_path == m32.last_path == "torch" and m32.getDownsamplingFactor() == U.DOWNSAMPLING
    assert p64.dtype == torch.float64 and tuple(p64.shape) == tuple(ref.shape) == tuple(meta["posteriors"][case]["shape"])
    assert (p64 - ref).abs().max().item() <= 1e-14
    assert p32.dtype == torch.float32 and (p32.double() - ref).abs().max().item() <= 4 * meta["f32_dev"]
    assert hot.dtype == torch.int64 and torch.equal(hot, ref_hot)


def test_to_one_hot_matches_the_reference():
    from cpc_audio_amd.harness import toOneHot
    arrays, _ = _gold()
    idx, n_items = U.indices()
    out = toOneHot(idx, n_items)
    assert out.dtype == torch.int64 and torch.equal(out, torch.from_numpy(arrays["c:one_hot"]))


def test_collapse_and_the_network_are_read_through_to_the_feature_module():
    from cpc_audio_amd import criterion as C
    from cpc_audio_amd.harness import FeatureModule, ModelPhoneCombined
    net = torch.nn.Linear(1, 1)
    fm = FeatureModule(net, False)
    m = ModelPhoneCombined(fm, U.build(C, "phone"), False)
    assert m.collapse is False and m.featureMaker is net
    fm.collapse = True
    assert m.collapse is True


def test_hip_head_true_on_cpu_tensors_raises():
    from cpc_audio_amd import criterion as C
    from cpc_audio_amd.harness import ModelPhoneCombined
    m = ModelPhoneCombined(U.Features(), U.build(C, "phone"), False, hipHead=True)
    with pytest.raises(NotImplementedError):
        m(U.features())


# ------------------------------------------------------------------------------------------------ (d) the arguments
@pytest.mark.parametrize("name", sorted(U.ARGV))
def test_parse_args_matches_the_reference(name):
    from cpc_audio_amd.build_zeroSpeech_features import parse_args
    got = vars(parse_args(list(U.ARGV[name])))
    assert got.pop("hipHead") is None                     # the one argument the reference does not have
    assert got == _gold()[1]["args"][name]


def test_hip_head_switches_and_the_missing_format():
    from cpc_audio_amd.build_zeroSpeech_features import parse_args
    base = U.ARGV["defaults"]
    assert parse_args(base + ["--hipHead"]).hipHead is True and parse_args(base + ["--no-hipHead"]).hipHead is False
    with pytest.raises(SystemExit):
        parse_args(base + ["--format", "af"])


def test_one_hot_with_seq_norm_is_refused_before_anything_is_read(tmp_path):
    from cpc_audio_amd.build_zeroSpeech_features import main
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="oneHot"):
        main([str(tmp_path / "no_such_db"), str(out), str(tmp_path / "no_such_checkpoint.pt"), "--addCriterion", "--oneHot",
              "--seqNorm"])
    assert not out.exists() and not (tmp_path / "out.json").exists()


# ------------------------------------------------------------------------------------------------ the checkpoint loaders
def _save(directory, name, args, model_state, criterion_state):
    from cpc_audio_amd.harness import save_checkpoint
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "checkpoint_args.json"), "w") as f:
        json.dump(args, f)
    path = os.path.join(directory, name)
    save_checkpoint(model_state, criterion_state, None, None, path)
    return path


@pytest.mark.parametrize("args,cls,n_classes,dim,n_phones,on_encoder", [
    ({"CTC": True, "onEncoder": False, "hiddenGar": 256}, "CTCPhoneCriterion", 42, 256, 41, False),
    ({"onEncoder": True, "hiddenGar": 256}, "PhoneCriterion", 41, 256, 41, True),
    # what linear_separability writes: no onEncoder, get_encoded instead; a width that is not hiddenGar's default
    ({"CTC": False, "get_encoded": True, "pathPhone": "/gone/phones.txt", "load": ["/elsewhere/checkpoint_3.pt"]},
     "PhoneCriterion", 13, 128, 13, True),
])
def test_load_supervised_criterion(args, cls, n_classes, dim, n_phones, on_encoder, tmp_path):
    from cpc_audio_amd import criterion as C
    from cpc_audio_amd.harness import loadSupervisedCriterion
    g = torch.Generator().manual_seed(n_classes)
    state = {"PhoneCriterionClassifier.weight": torch.randn(n_classes, dim, generator=g),
             "PhoneCriterionClassifier.bias": torch.randn(n_classes, generator=g)}
    path = _save(str(tmp_path), "checkpoint_7.pt", args, {}, state)
    crit, got = loadSupervisedCriterion(path)
    assert type(crit) is getattr(C, cls) and got == n_phones and crit.onEncoder is on_encoder
    assert torch.equal(crit.PhoneCriterionClassifier.weight, state["PhoneCriterionClassifier.weight"])
    assert torch.equal(crit.PhoneCriterionClassifier.bias, state["PhoneCriterionClassifier.bias"])
    if cls == "CTCPhoneCriterion":
        assert crit.BLANK_LABEL == n_phones


def test_load_supervised_criterion_needs_a_phone_classifier(tmp_path):
    from cpc_audio_amd.harness import loadSupervisedCriterion
    path = _save(str(tmp_path), "checkpoint_0.pt", {"get_encoded": False},
                 {}, {"linearSpeakerClassifier.weight": torch.zeros(12, 256), "linearSpeakerClassifier.bias": torch.zeros(12)})
    with pytest.raises(ValueError, match="PhoneCriterionClassifier"):
        loadSupervisedCriterion(path)


def test_load_model_reads_the_architecture_through_the_load_entry(tmp_path):
    """A classifier's checkpoint directory holds defaults (a one-layer LSTM) and points at the CPC checkpoint it was trained on,
    whose arguments describe a two-layer GRU: that is what must be built, with the weights of the path given."""
    from cpc_audio_amd.harness import loadModel
    from cpc_audio_amd.train import build_model
    torch.manual_seed(3)
    trained = build_model(arMode="GRU", nLevelsGRU=2)
    cpc_dir, top_dir = str(tmp_path / "cpc"), str(tmp_path / "linsep")
    base = _save(cpc_dir, "checkpoint_30.pt", {"arMode": "GRU", "nLevelsGRU": 2, "hiddenGar": 256, "hiddenEncoder": 256,
                                                "samplingType": "sequential", "load": None}, build_model(arMode="GRU").state_dict(), None)
    path = _save(top_dir, "checkpoint_9.pt", {"load": [base], "pathPhone": "/gone/phones.txt"}, trained.state_dict(), None)
    model, hidden_gar, hidden_encoder = loadModel([path])
    assert (hidden_gar, hidden_encoder) == (256, 256)
    assert isinstance(model.gAR.baseNet, torch.nn.GRU) and model.gAR.baseNet.num_layers == 2
    assert model.gAR.keepHidden is True                                   # samplingType "sequential", as getAR
    for k, v in trained.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    # without the indirection: the arguments beside the checkpoint, the reference's defaults for what they leave out
    plain, _, _ = loadModel([base])
    assert plain.gAR.baseNet.num_layers == 2 and plain.gAR.keepHidden is True
    bare = _save(str(tmp_path / "bare"), "checkpoint_0.pt", {}, {}, None)
    assert isinstance(loadModel([bare])[0].gAR.baseNet, torch.nn.LSTM) and loadModel([bare])[0].gAR.keepHidden is False


def test_load_model_refuses_concatenated_models(tmp_path):
    from cpc_audio_amd.harness import loadModel
    with pytest.raises(ValueError, match="concatenated"):
        loadModel([str(tmp_path / "a" / "checkpoint_0.pt"), str(tmp_path / "b" / "checkpoint_0.pt")])
    path = _save(str(tmp_path / "top"), "checkpoint_0.pt", {"load": ["/x/checkpoint_1.pt", "/y/checkpoint_2.pt"]}, {}, None)
    with pytest.raises(ValueError, match="concatenated"):
        loadModel([path])
