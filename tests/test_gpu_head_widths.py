"""The PER phone classifier and the phone posteriors at any feature width on an MI355X: the kernels through the C ABI with the
cases, oracles and bounds of tests/head_widths_util.py (which tests/test_emu_head_widths.py runs on the host emulator), then
the autograd functions, CTCphone_criterion(wideKernel=True), ModelPhoneCombined(wideKernel=True) and the two command lines on
40 features -- always against torch in float64 on the CPU, never against the HIP path itself."""
import gc
import itertools
import json
import math
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_widths_util as U
import zerospeech_util as ZU
from cpc_audio_amd import _lib, build_zeroSpeech_features as Z, common_voices_eval as CV, criterion as C, dataset, harness, ops, train
from seqnorm_util import LSTM_KEYS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def lib():
    return _lib.get()


@pytest.fixture(scope="module", autouse=True)
def collect_cycles_behind_this_module():
    """An exception caught by pytest.raises keeps its frames, and the device tensors of their locals, in a reference cycle until
    the collector runs.  Later modules that read torch.cuda.memory_allocated() around a call must not see them freed in between."""
    yield
    gc.collect()


# ------------------------------------------------------------------------------------------------ the kernels, C ABI
@pytest.mark.parametrize("D,B,S,C", U.HEAD_CASES)
def test_head_matches_conv1d_float64(D, B, S, C):
    U.check_head(lib(), DEV, D, B, S, C)


@pytest.mark.parametrize("B,S,C", [(2, 11, 7), (2, 37, 41), (1, 77, 65)])
def test_head_d_at_256_is_the_256_head(B, S, C):
    U.check_head_at_256(lib(), DEV, B, S, C)


@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_head_and_ctc_with_ragged_lengths(reduction):
    case = U.ragged_ctc_case()
    U.check_ctc_results(U.run_head_ctc(lib(), DEV, *case, reduction), *case, reduction)
    x, W, b, in_len, targets, tgt_len, blank = case                        # the same through the autograd function
    xr, Wr, br = (t.cuda().requires_grad_(True) for t in (x, W, b))
    loss = ops.PhoneHeadCtcFunction.apply(xr, Wr, br, in_len.cuda(), targets.cuda(), tgt_len.cuda(), blank, reduction)
    loss.sum().backward()
    U.check_ctc_results(tuple(t.detach().cpu() for t in (loss, Wr.grad, br.grad, xr.grad)), *case, reduction)
    logits = ops.phone_head_logits(x.cuda(), W.cuda(), b.cuda()).cpu()
    assert logits.shape == (4, 31, 65) and U.rel_err(logits.double(), U.oracle_head(x, W, b)) < 1e-5
    ops.check_device_errors()


@pytest.mark.parametrize("D,shape", list(itertools.product(U.WIDTHS, U.SEQNORM_SHAPES)))
def test_seqnorm_matches_float64(D, shape):
    for with_scale, normalise, scalar in [(True, True, False), (False, True, True), (True, False, False), (True, False, True)]:
        U.check_seqnorm(lib(), DEV, D, *shape, with_scale, normalise, scalar)


@pytest.mark.parametrize("D", U.WIDTHS)
@pytest.mark.parametrize("scalar", [False, True])
def test_seqnorm_columns_have_the_bits_of_a_256_wide_call(D, scalar):
    for shape in ((3, 33), (2, 70)):
        U.check_seqnorm_columns(lib(), DEV, D, *shape, scalar)


@pytest.mark.parametrize("scalar", [False, True])
def test_seqnorm_d_at_256_is_the_256_seqnorm(scalar):
    for shape in U.SEQNORM_SHAPES:
        U.check_seqnorm_at_256(lib(), DEV, *shape, scalar)


@pytest.mark.parametrize("D", [13, 257, 260])
def test_seqnorm_short_and_overlong_lengths(D):
    ops.check_device_errors()
    U.check_seqnorm_lengths(lib(), DEV, D)
    x, _, _ = U.seqnorm_case(D, 2, 31)                                     # the same through the function: reported once, clamped
    good = ops.SeqNormFunction.apply(x.cuda(), torch.tensor([31, 2]).cuda(), None, True)
    ops.check_device_errors()
    y = ops.SeqNormFunction.apply(x.cuda(), torch.tensor([32, 2]).cuda(), None, True)
    assert torch.equal(y, good)
    with pytest.raises(RuntimeError, match="length outside"):
        ops.check_device_errors()
    ops.check_device_errors()


@pytest.mark.parametrize("D,shape", list(itertools.product(U.WIDTHS, U.POSTERIOR_SHAPES)))
def test_posteriors_and_one_hot_match_torch_float64(D, shape):
    U.check_posterior(lib(), DEV, D, *shape)
    x, W, b, logits = U.posterior_case(D, *shape)                          # the same through ops.posterior
    post = ops.posterior(x.cuda(), W.cuda(), b.cuda(), wide=True).cpu()
    assert (post.double() - torch.softmax(logits, dim=1)).abs().max().item() <= 4 * U.f32_dev()
    hot = ops.posterior(x.cuda(), W.cuda(), b.cuda(), one_hot=True, wide=True).cpu()
    assert torch.equal(hot, F.one_hot(logits.argmax(dim=1), shape[1]))
    with pytest.raises(NotImplementedError):
        ops.posterior(x.cuda(), W.cuda(), b.cuda())
    ops.check_device_errors()


@pytest.mark.parametrize("R,C", [(33, 42), (70, 65), (5, 385)])
def test_posterior_at_13_is_16_with_zero_columns(R, C):
    U.check_posterior_zero_columns(lib(), DEV, R, C)


@pytest.mark.parametrize("R,C", [(33, 42), (70, 65), (40, 400)])
def test_posterior_d_at_256_is_the_256_posterior(R, C):
    U.check_posterior_at_256(lib(), DEV, R, C)


def test_posterior_reads_the_last_frame_of_every_window_in_place():
    """cFeature[:, -1, :]: rows S * D floats apart."""
    D, R, Cn = 40, 33, 42
    x, W, b, logits = U.posterior_case(D, R, Cn)
    c = torch.full((R, 3, D), float("nan"))
    c[:, -1, :] = x
    c = c.cuda()
    view = c[:, -1, :]
    assert view.stride(0) == 3 * D and not view.is_contiguous()
    post = ops.posterior(view, W.cuda(), b.cuda(), wide=True).cpu()
    assert torch.equal(post, ops.posterior(x.cuda(), W.cuda(), b.cuda(), wide=True).cpu())
    assert (post.double() - torch.softmax(logits, dim=1)).abs().max().item() <= 4 * U.f32_dev()
    with pytest.raises(NotImplementedError, match="512"):
        ops.posterior(torch.zeros(4, 513, device="cuda"), torch.zeros(41, 513, device="cuda"), torch.zeros(41, device="cuda"), wide=True)
    with pytest.raises(ValueError, match="weight"):
        ops.posterior(x.cuda(), torch.zeros(41, 64, device="cuda"), torch.zeros(41, device="cuda"), wide=True)


# ---------------------------------------------------------------------------------------------------------- the modules
DIM = 40


def _module_oracle(state, lstm, seq_norm, x, sizes, label, label_size, mask=None):
    """The module's arithmetic in float64 on the CPU: its own torch front and head on a float64 copy; ``mask`` (B, DIM) stands
    in for the dropout, as the factor Dropout2d would have drawn (tests/test_gpu_phone_front.py)."""
    ref = CV.CTCphone_criterion(DIM, 6, lstm, seqNorm=seq_norm, reduction="sum", hipHead=False, hipFront=False).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in state.items()})
    ref.train(mask is not None)
    if mask is not None:
        ref.dropout = lambda t: t * mask.double()[:, :, None]
    xr = x.double().clone().requires_grad_(True)
    loss = ref(xr, sizes, label, label_size)
    loss.sum().backward()
    with torch.no_grad():
        pred = ref.getPrediction(x.double(), sizes)
    return loss.detach(), {k: p.grad for k, p in ref.named_parameters()}, xr.grad, pred


def _check_module(crit, want, x, sizes, label, label_size, lstm):
    loss_w, grads_w, dx_w, _ = want
    xr = x.cuda().requires_grad_(True)
    loss = crit(xr, sizes.cuda(), label.cuda(), label_size.cuda())
    assert crit.last_path == "hip" and crit.last_front == "hip" and crit.last_lstm == ("torch" if lstm else None)
    assert loss.shape == (1, 1)
    loss.sum().backward()
    print(f"loss {loss.item()} against {loss_w.item()}")
    assert abs(loss.item() - loss_w.item()) <= 1e-5 * abs(loss_w.item()), (loss.item(), loss_w.item())
    got = dict(crit.named_parameters())
    for k in ["PhoneCriterionClassifier.weight", "PhoneCriterionClassifier.bias"] + (list(LSTM_KEYS) if lstm else []):
        err = U.rel_err(got[k].grad.cpu().double(), grads_w[k])
        print(f"{k}: gradient error {err:.3g}")
        assert err < 1e-4, k
    err = U.rel_err(xr.grad.cpu().double(), dx_w)
    print(f"dx: gradient error {err:.3g}")
    assert err < 1e-4
    assert torch.equal(xr.detach().cpu(), x)


def _module_inputs(B, sizes):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 45, DIM, generator=g) + 2.0 * torch.randn(DIM, generator=g)
    label = torch.randint(0, 6, (B, 6), generator=g)
    return x, torch.tensor(sizes), label, torch.tensor([4, 3, 2, 4, 3, 1, 3, 1][:B])


@pytest.mark.parametrize("lstm,seq_norm", [(False, True), (True, False), (True, True)], ids=["seqNorm", "LSTM", "LSTM-seqNorm"])
def test_module_on_40_features_agrees_with_the_float64_oracle(lstm, seq_norm):
    torch.manual_seed(7)
    crit = CV.CTCphone_criterion(DIM, 6, lstm, seqNorm=seq_norm, reduction="sum", hipHead=True, hipFront=True,
                                 wideKernel=True).cuda()
    x, sizes, label, label_size = _module_inputs(3, [45, 38, 21])
    want = _module_oracle(crit.state_dict(), lstm, seq_norm, x, sizes, label, label_size)
    _check_module(crit, want, x, sizes, label, label_size, lstm)
    assert crit.last_channel_scale is None
    with torch.no_grad():
        pred = crit.getPrediction(x.cuda(), sizes.cuda())
    assert crit.last_path == "hip" and crit.last_front == "hip" and pred.shape == (3, 10, 7)
    assert U.rel_err(pred.cpu().double(), want[3]) < 1e-5
    auto = CV.CTCphone_criterion(DIM, 6, lstm, seqNorm=seq_norm, reduction="sum").cuda()     # without the keyword: torch, as before
    auto.load_state_dict(crit.state_dict())
    with torch.no_grad():
        pred = auto.getPrediction(x.cuda(), sizes.cuda())
    assert auto.last_path == "torch" and auto.last_front == "torch" and U.rel_err(pred.cpu().double(), want[3]) < 1e-5
    ops.check_device_errors()


@pytest.mark.parametrize("lstm,seq_norm", [(False, False), (False, True), (True, True)], ids=["dropout", "seqNorm", "LSTM-seqNorm"])
def test_dropout_on_40_features_matches_the_oracle_with_the_mask_drawn(lstm, seq_norm):
    torch.manual_seed(11)
    crit = CV.CTCphone_criterion(DIM, 6, lstm, seqNorm=seq_norm, dropout=True, reduction="sum", hipHead=True, hipFront=True,
                                 wideKernel=True).cuda().train()
    x, sizes, label, label_size = _module_inputs(8, [45, 38, 21, 45, 30, 12, 40, 9])
    torch.manual_seed(12)
    loss = crit(x.cuda(), sizes.cuda(), label.cuda(), label_size.cuda())
    mask = crit.last_channel_scale
    assert mask is not None and mask.shape == (8, DIM) and crit.last_front == "hip"
    assert bool(((mask == 0) | (mask == 2)).all()) and bool((mask == 0).any()) and bool((mask == 2).any())
    want = _module_oracle(crit.state_dict(), lstm, seq_norm, x, sizes, label, label_size, mask=mask.cpu())
    assert abs(loss.item() - want[0].item()) <= 1e-5 * abs(want[0].item())
    torch.manual_seed(12)
    _check_module(crit, want, x, sizes, label, label_size, lstm)
    assert torch.equal(crit.last_channel_scale, mask)
    ops.check_device_errors()


def _write_wav(path, n, seed):
    g = torch.Generator().manual_seed(seed)
    pcm = ((0.1 * torch.randn(n, generator=g)).clamp_(-1, 1) * 32767).round().to(torch.int16).numpy()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.astype("<i2").tobytes())


def _mfcc_checkpoint(cdir, criterion=None, **extra):
    """A seeded MFCC encoder without a context network (it has no parameter that a seed reaches): 40 features per frame."""
    os.makedirs(cdir)
    torch.manual_seed(5)
    model = train.build_model(hiddenEncoder=DIM, hiddenGar=DIM, arMode="no_ar", encoder_type="mfcc", mfccKernel=True)
    path = os.path.join(cdir, "checkpoint_0.pt")
    harness.save_checkpoint(model.state_dict(), None if criterion is None else criterion.state_dict(), None, None, path)
    with open(os.path.join(cdir, "checkpoint_args.json"), "w") as f:
        json.dump({"hiddenEncoder": DIM, "hiddenGar": DIM, "arMode": "no_ar", "encoder_type": "mfcc", **extra}, f)
    return model, path


def test_train_then_per_with_wide_kernels_on_an_mfcc_checkpoint(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    db = str(tmp_path / "db")
    names = [f"s{k:02d}" for k in range(8)]
    for k, n in enumerate(names):
        _write_wav(os.path.join(db, n + ".wav"), int(rng.integers(40, 90)) * 160, seed=70 + k)
    (tmp_path / "val.txt").write_text("\n".join(names[:3]) + "\n")
    with open(tmp_path / "phones.txt", "w") as f:
        for n in names:
            f.write(n + " " + " ".join(str(int(v)) for v in rng.integers(0, 5, int(rng.integers(2, 6)))) + "\n")
    _, ckpt = _mfcc_checkpoint(str(tmp_path / "mfcc"))
    made = []

    class Recorded(CV.CTCphone_criterion):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(CV, "CTCphone_criterion", Recorded)
    out = tmp_path / "out"
    torch.manual_seed(0)
    assert CV.main(["train", db, str(tmp_path / "phones.txt"), ckpt, "-o", str(out), "--nEpochs", "2", "--batchSize", "4", "--freeze",
                    "--LSTM", "--seqNorm", "--dropout", "--hipFront", "--hipHead", "--wideKernel", "--file_extension", ".wav",
                    "--pathVal", str(tmp_path / "val.txt")]) is None
    assert len(made) == 1 and made[0].wideKernel is True and made[0].PhoneCriterionClassifier.in_channels == DIM
    assert made[0].last_path == "hip" and made[0].last_front == "hip" and made[0].last_lstm == "torch"
    stored = json.load(open(out / "args_training.json"))
    assert stored["wideKernel"] is True and stored["hipFront"] is True and stored["hipHead"] is True
    mean, std = CV.main(["per", str(out)])
    assert len(made) == 2 and made[1].wideKernel is True
    assert made[1].last_path == "hip" and made[1].last_front == "hip" and made[1].last_lstm == "torch"
    assert made[1].last_channel_scale is None
    assert json.load(open(out / "args_validation_0.json"))["wideKernel"] is True
    ckpt_out = torch.load(out / "checkpoint.pt", map_location="cpu")
    assert tuple(ckpt_out["classifier"]["module.PhoneCriterionClassifier.weight"].shape) == (6, DIM, 8)
    assert math.isfinite(ckpt_out["bestLoss"]) and math.isfinite(mean) and math.isfinite(std) and mean >= 0
    assert "Average PER" in (out / "logs_per_0.txt").read_text()
    ops.check_device_errors()


def _seeded_linear(crit, n_cls, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        crit.PhoneCriterionClassifier.weight.copy_((2 * torch.rand(n_cls, DIM, generator=g) - 1) / math.sqrt(DIM))
        crit.PhoneCriterionClassifier.bias.copy_((2 * torch.rand(n_cls, generator=g) - 1) / 16)
    return crit


@pytest.mark.parametrize("case", ["phone", "ctc"])
def test_model_phone_combined_on_40_features(case):
    n_cls = ZU.N_PHONES + (1 if case == "ctc" else 0)
    g = torch.Generator().manual_seed(21)
    c = torch.randn(2, 50, DIM, generator=g)
    for seed in range(20):                                  # a seeded classifier without a close top-2 margin
        crit = _seeded_linear(getattr(C, ZU.CRITERIA[case])(DIM, ZU.N_PHONES, False), n_cls, seed)
        lin = crit.PhoneCriterionClassifier
        logits = F.linear(c.double(), lin.weight.detach().double(), lin.bias.detach().double())
        if ZU.close_rows(logits) == 0:
            break
    else:
        raise AssertionError("no seeded classifier without a close top-2 margin")
    crit = crit.cuda()
    for one_hot in (False, True):
        m = harness.ModelPhoneCombined(ZU.Features(), crit, one_hot, hipHead=True, wideKernel=True)
        out = m(c.cuda()).cpu()
        assert m.last_path == "hip" and tuple(out.shape) == (2, 50, n_cls)
        if one_hot:
            assert out.dtype == torch.int64 and torch.equal(out, F.one_hot(logits.argmax(dim=2), n_cls))
        else:
            assert (out.double() - torch.softmax(logits, dim=2)).abs().max().item() <= 4 * U.f32_dev()
            assert (out.double().sum(dim=2) - 1).abs().max().item() <= 1e-6
        auto = harness.ModelPhoneCombined(ZU.Features(), crit, one_hot)      # without the keyword: torch, as before
        auto(c.cuda())
        assert auto.last_path == "torch"
        with pytest.raises(NotImplementedError):
            harness.ModelPhoneCombined(ZU.Features(), crit, one_hot, hipHead=True)(c.cuda())
    ops.check_device_errors()


def test_zerospeech_export_with_wide_kernels(tmp_path):
    """The posteriors' bound (4 x f32_dev) is what float32 deviates on unit-scale features under nn.Linear's initial scale, that
    is on logits of variance 1/3.  MFCC frames are tens of decibels large, so the seeded classifier is divided by the features'
    root mean square: the logits have the scale the bound was derived for."""
    db = str(tmp_path / "db")
    files = {"utt_a": 16000 + 777, "utt_b": 8000}
    for k, (stem, n) in enumerate(files.items()):
        _write_wav(os.path.join(db, stem + ".wav"), n, seed=90 + k)
    torch.manual_seed(5)
    model = train.build_model(hiddenEncoder=DIM, hiddenGar=DIM, arMode="no_ar", encoder_type="mfcc", mfccKernel=True)
    fm = harness.FeatureModule(model, False).cuda().eval()
    feats = {}
    for stem in files:
        wav = dataset.loadFile((0, os.path.join(db, stem + ".wav")))[2].view(1, -1)
        feats[stem] = harness.build_feature(fm, wav, strict=False, max_size_seq=64000)[0].double().cpu()
    rms = float(torch.cat(list(feats.values())).pow(2).mean().sqrt())
    for seed in range(20):                                  # a seeded classifier without a close top-2 margin
        crit = _seeded_linear(C.CTCPhoneCriterion(DIM, ZU.N_PHONES, False), ZU.N_PHONES + 1, seed)
        lin = crit.PhoneCriterionClassifier
        with torch.no_grad():
            lin.weight.div_(rms)
        logits = {k: F.linear(f, lin.weight.detach().double(), lin.bias.detach().double()) for k, f in feats.items()}
        if sum(ZU.close_rows(l) for l in logits.values()) == 0:
            break
    else:
        raise AssertionError("no seeded classifier without a close top-2 margin")
    _, ckpt = _mfcc_checkpoint(str(tmp_path / "mfcc"), crit, CTC=True, onEncoder=False)
    outs = {}
    for name, options in (("hip", ("--hipHead", "--wideKernel")), ("torch", ("--no-hipHead",))):
        out = str(tmp_path / name)
        maker = Z.main([db, out + os.sep, ckpt, "--addCriterion", "--format", "npy", *options])
        assert isinstance(maker, harness.ModelPhoneCombined) and maker.last_path == name
        assert json.load(open(out + ".json")).get("wideKernel", False) is (name == "hip")
        outs[name] = {stem: np.load(os.path.join(out, stem + ".npy")).astype(np.float64) for stem in files}
    with pytest.raises(NotImplementedError):                # without the option the HIP call refuses 40 features, as before
        Z.main([db, str(tmp_path / "refused") + os.sep, ckpt, "--addCriterion", "--format", "npy", "--hipHead"])
    for stem, n in files.items():
        ref = torch.softmax(logits[stem], dim=1).numpy()
        hip, plain = outs["hip"][stem], outs["torch"][stem]
        assert hip.shape == plain.shape == ref.shape == (feats[stem].shape[0], ZU.N_PHONES + 1) and feats[stem].shape[0] >= n // 160
        err, err_t, between = np.abs(hip - ref).max(), np.abs(plain - ref).max(), np.abs(hip - plain).max()
        print(f"{stem}: features rms {rms:.3g}; max abs err hip {err:.3e}, torch {err_t:.3e}, between the two {between:.3e} "
              f"(bound {4 * U.f32_dev():.3e})")
        assert err <= 4 * U.f32_dev()
        assert between <= 4 * U.f32_dev()
        assert np.abs(hip.sum(axis=1) - 1).max() <= 1e-6
    ops.check_device_errors()
