"""The Python surface of the encoder's normModes (no GPU): build_model(normMode=...) has the reference's state-dict keys and shapes,
a batchNorm checkpoint opens through harness.loadModel with its running statistics, the flag predicates, the evaluation CLIs'
--encoderKernel, and the float64 reference of tests/encoder_norms_util.py against this package's own torch modules."""
import json

import pytest
import torch

import encoder_norms_util as U
from oracle import cpc_oracle as O

MODES = ("layerNorm", "batchNorm", "instanceNorm", "ID")


@pytest.mark.parametrize("mode", MODES)
def test_build_model_has_the_reference_keys_and_shapes(mode):
    from cpc_audio_amd import train
    C = 40
    m = train.build_model(hiddenEncoder=C, normMode=mode, encoderKernel=True)
    sd = {k: tuple(v.shape) for k, v in m.gEncoder.state_dict().items()}
    want = {}
    for i, k in enumerate((10, 8, 4, 4, 4)):
        want[f"conv{i}.weight"] = (C, 1 if i == 0 else C, k)
        want[f"conv{i}.bias"] = (C,)
        if mode == "layerNorm":
            want[f"batchNorm{i}.weight"] = want[f"batchNorm{i}.bias"] = (1, C, 1)
        elif mode in ("batchNorm", "instanceNorm"):
            want[f"batchNorm{i}.weight"] = want[f"batchNorm{i}.bias"] = (C,)
        if mode == "batchNorm":
            want[f"batchNorm{i}.running_mean"] = want[f"batchNorm{i}.running_var"] = (C,)
            want[f"batchNorm{i}.num_batches_tracked"] = ()
    assert sd == want
    assert len(list(m.gEncoder.parameters())) == (10 if mode == "ID" else 20)


def test_the_flag_predicates():
    from cpc_audio_amd import train
    from cpc_audio_amd.model import CPCEncoder
    for mode in ("batchNorm", "instanceNorm", "ID"):
        for C in (2, 40, 256, 512):
            enc = CPCEncoder(C, mode, encoderKernel=True)
            assert enc.hip_norm is True and enc.hip is False and enc.hip_wide is False, (mode, C)
        for C in (1, 513):
            assert CPCEncoder(C, mode, encoderKernel=True).hip_norm is False
        assert CPCEncoder(40, mode).hip_norm is False and CPCEncoder(256, mode).hip_norm is False           # off by default
        assert train.build_model(hiddenEncoder=40, normMode=mode).gEncoder.hip_norm is False
        assert train.build_model(hiddenEncoder=256, normMode=mode, encoderKernel=True).gEncoder.hip_norm is True
    # layerNorm keeps its own attributes
    assert CPCEncoder(40, "layerNorm", encoderKernel=True).hip_norm is False
    assert CPCEncoder(40, "layerNorm", encoderKernel=True).hip_wide is True
    same = CPCEncoder(256, "layerNorm", encoderKernel=True)
    assert same.hip is True and same.hip_wide is False and same.hip_norm is False
    assert train.build_model().gEncoder.hip is True and train.build_model().gEncoder.hip_norm is False
    with pytest.raises(ValueError):
        train.build_model(normMode="groupNorm")


def test_a_batch_norm_checkpoint_opens_with_its_running_statistics(tmp_path):
    from cpc_audio_amd import harness, train
    torch.manual_seed(3)
    m = train.build_model(hiddenEncoder=40, hiddenGar=256, nLevelsGRU=2, arMode="GRU", normMode="batchNorm")
    with torch.no_grad():
        for i in range(5):
            bn = getattr(m.gEncoder, f"batchNorm{i}")
            bn.running_mean.copy_(torch.randn(40))
            bn.running_var.copy_(torch.rand(40) + 0.5)
            bn.weight.copy_(torch.randn(40))
            bn.num_batches_tracked.fill_(7 + i)
    path = str(tmp_path / "checkpoint_3.pt")
    torch.save({"gEncoder": m.state_dict()}, path)
    with open(str(tmp_path / "checkpoint_args.json"), "w") as f:
        json.dump({"hiddenEncoder": 40, "hiddenGar": 256, "nLevelsGRU": 2, "arMode": "GRU", "normMode": "batchNorm"}, f)
    for kw in (False, True):
        loaded, hiddenGar, hiddenEncoder = harness.loadModel([path], encoderKernel=kw)
        assert (hiddenGar, hiddenEncoder) == (256, 40)
        assert isinstance(loaded.gEncoder.batchNorm0, torch.nn.BatchNorm1d)
        assert loaded.gEncoder.hip_norm is kw and loaded.gEncoder.hip is False and loaded.gEncoder.hip_wide is False
        got, want = loaded.state_dict(), m.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        assert int(loaded.gEncoder.batchNorm2.num_batches_tracked) == 9
    # without the entry the arguments describe a layerNorm model, as before: the (C,) weights do not fit it
    with open(str(tmp_path / "checkpoint_args.json"), "w") as f:
        json.dump({"hiddenEncoder": 40, "hiddenGar": 256, "nLevelsGRU": 2, "arMode": "GRU"}, f)
    with pytest.raises(RuntimeError):
        harness.loadModel([path])


def test_the_evaluation_clis_parse_encoder_kernel():
    from cpc_audio_amd import abx, build_zeroSpeech_features, common_voices_eval, linear_separability
    a = abx.parse_args(["from_checkpoint", "ckpt.pt", "items.item", "db", "--encoderKernel"])
    assert a.encoderKernel is True
    assert not hasattr(abx.parse_args(["from_checkpoint", "ckpt.pt", "items.item", "db"]), "encoderKernel")
    a = linear_separability.parse_args(["db", "train.txt", "val.txt", "ckpt.pt", "--encoderKernel"])
    assert a.encoderKernel is True
    assert not hasattr(linear_separability.parse_args(["db", "train.txt", "val.txt", "ckpt.pt"]), "encoderKernel")
    a = common_voices_eval.parse_args(["train", "db", "phones.txt", "ckpt.pt", "--encoderKernel"])
    assert a.encoderKernel is True
    assert not hasattr(common_voices_eval.parse_args(["train", "db", "phones.txt", "ckpt.pt"]), "encoderKernel")
    a = build_zeroSpeech_features.parse_args(["db", "out", "ckpt.pt", "--encoderKernel"])
    assert a.encoderKernel is True
    assert not hasattr(build_zeroSpeech_features.parse_args(["db", "out", "ckpt.pt"]), "encoderKernel")


def test_cpu_input_runs_the_torch_modules():
    from cpc_audio_amd.model import CPCEncoder
    x = torch.randn(2, 1, 1280, generator=torch.Generator().manual_seed(1))
    for mode in ("batchNorm", "instanceNorm", "ID"):
        torch.manual_seed(0)
        enc = CPCEncoder(40, mode, encoderKernel=True)
        plain = CPCEncoder(40, mode)
        plain.load_state_dict(enc.state_dict())
        y, yp = enc(x), plain(x)                            # (one call each: a batchNorm forward moves the running buffers)
        assert tuple(y.shape) == (2, 40, 8) and torch.equal(y, yp)
        y.sum().backward()
        yp.sum().backward()
        for a, b in zip(enc.parameters(), plain.parameters()):
            assert torch.equal(a.grad, b.grad)
        for (k, a), (_, b) in zip(enc.state_dict().items(), plain.state_dict().items()):
            assert torch.equal(a, b), k
    # where torch raises, the module raises: one value per channel
    with pytest.raises(ValueError):
        CPCEncoder(40, "instanceNorm", encoderKernel=True)(torch.randn(1, 1, 170))
    with pytest.raises(ValueError):
        CPCEncoder(40, "batchNorm", encoderKernel=True)(torch.randn(1, 1, 170))


@pytest.mark.parametrize("mode,training", U.VARIANTS)
def test_the_float64_reference_is_the_packages_torch_path(mode, training):
    """tests/encoder_norms_util.reference64 against CPCEncoder(C, mode).double() -- the torch modules the reference builds -- to
    1e-12: outputs, every gradient, the running buffers."""
    from cpc_audio_amd.model import CPCEncoder
    C, B, L = 30, 3, 1290
    params, running = U.make_params(C, mode)
    wave = O.make_waveform(B, L, seed=5)
    dz = torch.randn(B, 8, C, generator=torch.Generator().manual_seed(11))
    z_ref, _, leaves, run_ref, _ = U.reference64(mode, training, params, running, wave, dz)
    enc = CPCEncoder(C, mode).double()
    sd = {k: v.double() for k, v in params.items()}
    if running is not None:
        for i in range(5):
            sd[f"batchNorm{i}.running_mean"], sd[f"batchNorm{i}.running_var"] = running[2 * i].double(), running[2 * i + 1].double()
    missing = enc.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys)
    enc.train(training)
    with torch.backends.mkldnn.flags(enabled=False):
        z = enc(wave.double()).permute(0, 2, 1)
        (z * dz.double()).sum().backward()
    assert (z - z_ref).abs().max().item() < 1e-12
    for n, q in enc.named_parameters():
        assert (q.grad - leaves[n].grad).abs().max().item() <= 1e-12 * max(1.0, leaves[n].grad.abs().max().item()), n
    if running is not None:
        for i in range(5):
            bn = getattr(enc, f"batchNorm{i}")
            assert (bn.running_mean - run_ref[2 * i]).abs().max().item() < 1e-12
            assert (bn.running_var - run_ref[2 * i + 1]).abs().max().item() < 1e-12
            assert int(bn.num_batches_tracked) == (1 if training else 0)
