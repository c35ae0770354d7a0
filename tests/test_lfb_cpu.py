"""The learned-filter-bank encoder and the identity autoregressor on the CPU: the modules' surface, the builders and loaders that
must accept them, the module's torch path against the reference fixture (tests/golden/lfb.npz, tools/make_golden_lfb.py) and
the workspace condition of the HIP kernels (nothing of the conv output's size is ever stored)."""
import json
import os
import shutil

import pytest
import torch

import lfb_util as U
from cpc_audio_amd import harness, model, train


def test_state_dict_and_attributes_are_the_references():
    enc = model.LFBEnconder(32)
    sd = enc.state_dict()
    assert list(sd.keys()) == ["han", "conv.weight", "conv.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(1, 1, 400), (64, 1, 400), (64,)]
    assert torch.equal(sd["han"].view(-1), torch.hann_window(400))
    assert enc.dimEncoded == 32 and enc.DOWNSAMPLING == 160 and enc.getDimOutput() == 32
    assert isinstance(enc.instancenorm, torch.nn.InstanceNorm1d) and not list(enc.instancenorm.state_dict())
    assert model.LFBEnconder(32, normalize=False).instancenorm is None
    assert [n for n, _ in enc.named_parameters()] == ["conv.weight", "conv.bias"]


@pytest.mark.parametrize("L,F", [(400, 2), (418, 2), (419, 3), (578, 3), (579, 4), (20480, 128), (64000, 400)])
def test_frame_count(L, F):
    enc = model.LFBEnconder(32)
    with torch.no_grad():
        y = enc(torch.zeros(1, 1, L))
    assert tuple(y.shape) == (1, 32, F)
    assert bool(torch.isfinite(y).all())
    from cpc_audio_amd import ops
    assert ops.lfb_frames(L) == F == U.frames(L)


def test_a_window_shorter_than_the_filter_raises():
    with pytest.raises(ValueError):
        model.LFBEnconder(32)(torch.zeros(1, 1, 399))


def test_noar_is_the_identity_without_parameters():
    ar = model.NoAr(32, 32, False, 1)
    x = torch.randn(2, 5, 32)
    assert ar(x) is x
    assert not list(ar.parameters()) and not ar.state_dict()
    assert ar.hip is False and ar.reverse is False and ar.keepHidden is False and ar.hidden is None
    ar.keepHidden = True                      # what the evaluation scripts set on any autoregressor
    assert ar(x) is x and ar.hidden is None


def test_build_model_accepts_lfb_and_no_ar_and_refuses_mfcc():
    m = train.build_model(hiddenEncoder=32, hiddenGar=64, arMode="no_ar", encoder_type="lfb")
    assert type(m.gEncoder) is model.LFBEnconder and type(m.gAR) is model.NoAr and m.gEncoder.dimEncoded == 32
    c, z, label = m(0.1 * torch.randn(2, 1, 1040), None)
    assert c is z and tuple(z.shape) == (2, 6, 32)
    g = train.build_model(hiddenEncoder=32, hiddenGar=48, nLevelsGRU=1, arMode="GRU", encoder_type="lfb")
    assert type(g.gAR) is model.CPCAR and tuple(g(torch.zeros(1, 1, 1040), None)[0].shape) == (1, 6, 48)
    assert type(train.build_model().gEncoder) is model.CPCEncoder                    # the default stays the CPC encoder
    with pytest.raises(NotImplementedError, match="torchaudio"):
        train.build_model(encoder_type="mfcc")
    with pytest.raises(ValueError):
        train.build_model(encoder_type="wav2vec")


def test_load_model_rebuilds_an_lfb_checkpoint(tmp_path):
    src = train.build_model(hiddenEncoder=32, arMode="no_ar", encoder_type="lfb")
    with open(tmp_path / "checkpoint_args.json", "w") as f:
        json.dump({"encoder_type": "lfb", "arMode": "no_ar", "hiddenEncoder": 32}, f)
    path = str(tmp_path / "checkpoint_3.pt")
    torch.save({"gEncoder": src.state_dict()}, path)
    m, hidden_gar, hidden_encoder = harness.loadModel([path])
    assert (hidden_gar, hidden_encoder) == (32, 32)
    assert type(m.gEncoder) is model.LFBEnconder and type(m.gAR) is model.NoAr
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in m.state_dict().items()) and len(m.state_dict()) == 3
    with open(tmp_path / "checkpoint_args.json", "w") as f:                 # a file without the key is a CPC encoder
        json.dump({"arMode": "no_ar", "hiddenEncoder": 256}, f)
    torch.save({"gEncoder": train.build_model(arMode="no_ar").state_dict()}, path)
    assert type(harness.loadModel([path])[0].gEncoder) is model.CPCEncoder


@pytest.mark.parametrize("tag", ["small", "wide"])
def test_torch_path_reproduces_the_reference(tag):
    arrays, meta = U.golden()
    c = meta["cases"][tag]
    enc = model.LFBEnconder(c["D"])
    assert list(enc.state_dict().keys()) == c["keys"]
    enc.load_state_dict(U.golden_state(arrays, meta, tag), strict=True)
    U.check_against_golden(enc, arrays, meta, tag, "cpu", y_tol=2e-6, grad_tol=1e-5)


def test_torch_path_matches_the_float64_formula_without_the_norm():
    x, W, b, han, gs = U.energy_case(2, 1040, 32, seed=11)
    enc = model.LFBEnconder(32, normalize=False)
    enc.load_state_dict({"han": han.view(1, 1, 400), "conv.weight": W.view(64, 1, 400), "conv.bias": b})
    want = U.lognorm_oracle(U.energy_oracle(x, W, b, han)["s"].float(), normalise=False)["y"].permute(0, 2, 1)
    assert U.rel_err(enc(x[:, None, :]).detach(), want) < 1e-5


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs the built library")
def test_workspaces_stay_far_below_the_conv_output():
    """Nothing of size N D (L - 399) is stored: at (64, 20480, 256) the conv output is 2.63 GB; both workspaces are below an
    eighth of it, and the forward's does not grow with L beyond O(N F D)."""
    from cpc_audio_amd import _lib
    lib = _lib.get()
    N, L, D = 64, 20480, 256
    rc, (F, fwd, bwd) = U.layout(lib, N, L, D)
    assert rc == 0 and F == 128
    conv_bytes = N * 2 * D * (L - 399) * 4
    assert conv_bytes > 2.6e9
    assert 0 <= fwd < conv_bytes // 8 and 0 < bwd < conv_bytes // 8
    for L2 in (64000, 640000):
        rc, (F2, fwd2, bwd2) = U.layout(lib, N, L2, D)
        assert rc == 0 and fwd2 <= 4 * N * F2 * D * 4 and bwd2 < conv_bytes // 8
