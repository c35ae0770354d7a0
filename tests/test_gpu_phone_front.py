"""The PER phone classifier's front on an MI355X (csrc/seqnorm.hip, csrc/lstm.hip): ops.SeqNormFunction,
CTCphone_criterion(hipFront=True) for every combination of --LSTM / --seqNorm / --dropout, the reference's fixture and
`train` + `per` end to end -- always against torch in float64 on the CPU (the module's own torch front, hipFront=False) or
the reference's stored results, never against the HIP path itself.

Tolerances are the project's own (tests/test_gpu_supervised.py, tests/test_gpu_phone_head.py): forward 1e-5 and gradients
1e-4 as norm-relative error, losses 1e-5 relative."""
import json
import math

import numpy as np
import pytest
import torch

from cpc_audio_amd import common_voices_eval as CV, ops
from seqnorm_util import (BACKWARD_CASES, FORWARD_CASES, LSTM_KEYS, case, check_against_golden, golden, golden_criterion, oracle,
                          rel_err)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_function_forward_matches_float64(name):
    B, S, lengths, offset = FORWARD_CASES[name]
    x, lens, _, scale = case(B, S, lengths, offset, seed=B + S)
    xc = x.cuda()
    for sc in (None, scale):
        y = ops.SeqNormFunction.apply(xc, lens.cuda(), None if sc is None else sc.cuda(), True)
        again = ops.SeqNormFunction.apply(xc, lens.cuda(), None if sc is None else sc.cuda(), True)
        err = rel_err(y.cpu().double(), oracle(x, lens, sc)["y"])
        print(f"{name} scale={sc is not None}: forward error {err:.3g}")
        assert err < 1e-5
        assert torch.equal(y, again) and not y.requires_grad
    assert torch.equal(xc.cpu(), x)
    y = ops.SeqNormFunction.apply(xc, None, scale.cuda(), False)                 # the dropout alone
    assert torch.equal(y.cpu(), x * scale[:, None, :])
    ops.check_device_errors()


@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_function_backward_matches_autograd_float64(name):
    B, S, lengths, offset = BACKWARD_CASES[name]
    x, lens, dy, scale = case(B, S, lengths, offset, seed=B + S + 1)
    for sc in (None, scale):
        grads = []
        for _ in range(2):
            xr = x.cuda().requires_grad_(True)
            y = ops.SeqNormFunction.apply(xr, lens.cuda(), None if sc is None else sc.cuda(), True)
            (y * dy.cuda()).sum().backward()
            grads.append(xr.grad)
        err = rel_err(grads[0].cpu().double(), oracle(x, lens, sc, dy=dy)["dx"])
        print(f"{name} scale={sc is not None}: backward error {err:.3g}")
        assert err < 1e-4
        assert torch.equal(grads[0], grads[1])
    xr = x.cuda().requires_grad_(True)
    (ops.SeqNormFunction.apply(xr, None, scale.cuda(), False) * dy.cuda()).sum().backward()
    assert torch.equal(xr.grad.cpu(), dy * scale[:, None, :])
    ops.check_device_errors()


def test_frozen_features_keep_no_statistics_and_get_no_gradient():
    x, lens, dy, scale = case(3, 45, [45, 38, 3], 0.0, seed=2)
    xc, w = x.cuda(), torch.ones(256, device="cuda", requires_grad=True)
    y = ops.SeqNormFunction.apply(xc, lens.cuda(), scale.cuda(), True)
    assert not y.requires_grad and y.grad_fn is None
    ((y * w) * dy.cuda()).sum().backward()
    assert xc.grad is None and w.grad is not None
    with pytest.raises(RuntimeError):
        ops.SeqNormFunction.apply(x, lens, scale, True)                           # no CPU path


def test_a_single_frame_gives_nan_and_a_length_past_the_end_is_reported():
    x, lens, _, _ = case(3, 45, [45, 38, 3], 0.0, seed=3)
    good = ops.SeqNormFunction.apply(x.cuda(), lens.cuda(), None, True)
    y = ops.SeqNormFunction.apply(x.cuda(), torch.tensor([45, 1, 3]).cuda(), None, True)
    assert bool(torch.isnan(y[1]).all()) and torch.equal(y[0], good[0]) and torch.equal(y[2], good[2])
    ops.check_device_errors()
    y = ops.SeqNormFunction.apply(x.cuda(), torch.tensor([46, 38, 3]).cuda(), None, True)
    assert torch.equal(y, good)                                                   # clamped to S
    with pytest.raises(RuntimeError, match="length outside"):
        ops.check_device_errors()
    ops.check_device_errors()


def _module_oracle(state, lstm, seq_norm, x, sizes, label, label_size, mask=None):
    """The module's arithmetic in float64 on the CPU: its own torch front and head (hipHead=False, hipFront=False) on a
    float64 copy; `mask` (B, 256) stands in for the dropout, as the factor Dropout2d would have drawn (train(), where the
    module applies its dropout; nothing else of it depends on the mode), eval() without one."""
    ref = CV.CTCphone_criterion(256, 6, lstm, seqNorm=seq_norm, reduction="sum", hipHead=False, hipFront=False).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in state.items()})
    ref.train(mask is not None)
    if mask is not None:
        ref.dropout = lambda t: t * mask.double()[:, :, None]                     # t: (B, 256, S)
    xr = x.double().clone().requires_grad_(True)
    loss = ref(xr, sizes, label, label_size)
    loss.sum().backward()
    grads = {k: p.grad for k, p in ref.named_parameters()}
    with torch.no_grad():
        pred = ref.getPrediction(x.double(), sizes)
    return loss.detach(), grads, xr.grad, pred


def _check_module(crit, want, x, sizes, label, label_size, lstm):
    loss_w, grads_w, dx_w, _ = want
    xr = x.cuda().requires_grad_(True)
    loss = crit(xr, sizes.cuda(), label.cuda(), label_size.cuda())
    assert crit.last_front == "hip" and crit.last_path == "hip" and loss.shape == (1, 1)
    loss.sum().backward()
    print(f"loss {loss.item()} against {loss_w.item()}")
    assert abs(loss.item() - loss_w.item()) <= 1e-5 * abs(loss_w.item()), (loss.item(), loss_w.item())
    keys = ["PhoneCriterionClassifier.weight", "PhoneCriterionClassifier.bias"] + (list(LSTM_KEYS) if lstm else [])
    got = dict(crit.named_parameters())
    for k in keys:
        err = rel_err(got[k].grad.cpu().double(), grads_w[k])
        print(f"{k}: gradient error {err:.3g}")
        assert err < 1e-4, k
    err = rel_err(xr.grad.cpu().double(), dx_w)
    print(f"dx: gradient error {err:.3g}")
    assert err < 1e-4
    assert torch.equal(xr.detach().cpu(), x)                                      # the front never writes into its input


def _module_inputs(B, sizes):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 45, 256, generator=g) + 2.0 * torch.randn(256, generator=g)
    label = torch.randint(0, 6, (B, 6), generator=g)
    label_size = torch.tensor([4, 3, 2, 4, 3, 1, 3, 1][:B])                       # each fits into its utterance's windows
    return x, torch.tensor(sizes), label, label_size


@pytest.mark.parametrize("lstm,seq_norm", [(False, True), (True, False), (True, True)], ids=["seqNorm", "LSTM", "LSTM-seqNorm"])
def test_module_with_the_hip_front_agrees_with_the_float64_oracle(lstm, seq_norm):
    torch.manual_seed(7)
    crit = CV.CTCphone_criterion(256, 6, lstm, seqNorm=seq_norm, reduction="sum", hipHead=True, hipFront=True).cuda()
    x, sizes, label, label_size = _module_inputs(3, [45, 38, 21])
    want = _module_oracle(crit.state_dict(), lstm, seq_norm, x, sizes, label, label_size)
    _check_module(crit, want, x, sizes, label, label_size, lstm)
    assert crit.last_channel_scale is None
    xc = x.cuda()
    with torch.no_grad():
        pred = crit.getPrediction(xc, sizes.cuda())
    assert crit.last_front == "hip" and pred.shape == (3, 10, 7) and torch.equal(xc.cpu(), x)
    assert rel_err(pred.cpu().double(), want[3]) < 1e-5
    torch_head = CV.CTCphone_criterion(256, 6, lstm, seqNorm=seq_norm, reduction="sum", hipHead=False, hipFront=True).cuda()
    torch_head.load_state_dict(crit.state_dict())                                 # either head reads the HIP front's output
    with torch.no_grad():
        pred = torch_head.getPrediction(xc, sizes.cuda())
    assert torch_head.last_front == "hip" and torch_head.last_path == "torch"
    assert rel_err(pred.cpu().double(), want[3]) < 1e-5
    ops.check_device_errors()


@pytest.mark.parametrize("lstm,seq_norm", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["dropout", "seqNorm", "LSTM", "LSTM-seqNorm"])
def test_dropout_draws_a_channel_mask_and_matches_the_oracle_with_that_mask(lstm, seq_norm):
    torch.manual_seed(11)
    crit = CV.CTCphone_criterion(256, 6, lstm, seqNorm=seq_norm, dropout=True, reduction="sum", hipHead=True,
                                 hipFront=True).cuda().train()
    x, sizes, label, label_size = _module_inputs(8, [45, 38, 21, 45, 30, 12, 40, 9])
    torch.manual_seed(12)
    loss = crit(x.cuda(), sizes.cuda(), label.cuda(), label_size.cuda())
    mask = crit.last_channel_scale
    assert mask is not None and mask.shape == (8, 256) and crit.last_front == "hip"
    assert bool(((mask == 0) | (mask == 2)).all())
    keep = (mask == 2).float().mean().item()
    assert abs(keep - 0.5) <= 0.06, keep                                          # 5 sigma of 2048 draws
    torch.manual_seed(12)                                                         # torch's generator governs the mask
    crit(x.cuda(), sizes.cuda(), label.cuda(), label_size.cuda())
    assert torch.equal(crit.last_channel_scale, mask)
    want = _module_oracle(crit.state_dict(), lstm, seq_norm, x, sizes, label, label_size, mask=mask.cpu())
    assert abs(loss.item() - want[0].item()) <= 1e-5 * abs(want[0].item())
    torch.manual_seed(12)
    _check_module(crit, want, x, sizes, label, label_size, lstm)
    assert torch.equal(crit.last_channel_scale, mask)
    crit.eval()
    with torch.no_grad():
        loss = crit(x.cuda(), sizes.cuda(), label.cuda(), label_size.cuda())
    assert crit.last_channel_scale is None and crit.last_front == ("hip" if lstm or seq_norm else None)
    plain = _module_oracle(crit.state_dict(), lstm, seq_norm, x, sizes, label, label_size)
    assert abs(loss.item() - plain[0].item()) <= 1e-5 * abs(plain[0].item())
    ops.check_device_errors()


@pytest.mark.parametrize("lstm", [False, True], ids=["plain", "lstm"])
def test_hip_front_matches_the_reference_fixture(lstm):
    arrays, meta = golden()
    crit = golden_criterion(meta, lstm, hipFront=True, hipHead=True).cuda()
    check_against_golden(crit, arrays, meta, lstm, "cuda", 1e-5, 1e-4)
    assert crit.last_front == "hip" and crit.last_path == "hip"
    ops.check_device_errors()


def test_train_then_per_on_the_hip_front(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    db = tmp_path / "db"
    db.mkdir()
    names = [f"s{k:02d}" for k in range(12)]
    for n in names:
        np.save(db / f"{n}.npy", rng.standard_normal((256, int(rng.integers(80, 200)))).astype(np.float32))
    (tmp_path / "val.txt").write_text("\n".join(names[:3]) + "\n")
    with open(tmp_path / "phones.txt", "w") as f:
        for n in names:
            f.write(n + " " + " ".join(str(int(v)) for v in rng.integers(0, 5, int(rng.integers(3, 12)))) + "\n")
    made = []

    class Recorded(CV.CTCphone_criterion):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(CV, "CTCphone_criterion", Recorded)
    out = tmp_path / "out"
    torch.manual_seed(0)
    assert CV.main(["train", str(db), str(tmp_path / "phones.txt"), "ID", "-o", str(out), "--nEpochs", "2", "--batchSize", "4",
                    "--in_dim", "256", "--LSTM", "--seqNorm", "--dropout", "--hipFront", "--hipHead", "--file_extension", ".npy",
                    "--pathVal", str(tmp_path / "val.txt")]) is None
    assert len(made) == 1 and made[0].hipFront is True and made[0].last_front == "hip" and made[0].last_path == "hip"
    assert made[0].useLSTM and made[0].seqNorm and made[0].dropout is not None
    stored = json.load(open(out / "args_training.json"))
    assert stored["hipFront"] is True and stored["hipHead"] is True
    mean, std = CV.main(["per", str(out)])
    assert len(made) == 2 and made[1].hipFront is True and made[1].last_front == "hip" and made[1].last_path == "hip"
    assert made[1].last_channel_scale is None                                     # eval(): no mask
    ckpt = torch.load(out / "checkpoint.pt", map_location="cpu")
    assert "module.conv1.weight_ih_l0" in ckpt["classifier"] and math.isfinite(ckpt["bestLoss"])
    assert math.isfinite(mean) and math.isfinite(std) and mean >= 0
    assert "Average PER" in (out / "logs_per_0.txt").read_text()
    ops.check_device_errors()
