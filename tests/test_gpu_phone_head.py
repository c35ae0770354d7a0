"""The PER phone classifier on an MI355X (csrc/phone_head.hip): the autograd function, CTCphone_criterion(hipHead=True), the
reference's fixture and `train` + `per` end to end, always against torch in float64 on the CPU (F.conv1d, F.log_softmax,
F.ctc_loss) or the reference's stored results -- never against the HIP path itself.

Tolerances are those of the project's other supervised kernels (tests/test_gpu_supervised.py): losses 1e-5 relative, gradients
through the CTC loss 1e-4, the head's logits 1e-5."""
import json
import math
import os

import numpy as np
import pytest
import torch

from cpc_audio_amd import common_voices_eval as CV, ops
from phone_head_util import head_case, oracle_full, ragged_targets

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_err(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _run(x, W, b, in_len, targets, tgt_len, blank, reduction):
    xr, Wr, br = (t.cuda().requires_grad_(True) for t in (x, W, b))
    loss = ops.PhoneHeadCtcFunction.apply(xr, Wr, br, in_len.cuda(), targets.cuda(), tgt_len.cuda(), blank, reduction)
    loss.sum().backward()
    return tuple(t.detach().cpu() for t in (loss, Wr.grad, br.grad, xr.grad))


@pytest.mark.parametrize("B,S,C,reduction", [(3, 12, 7, "sum"), (2, 37, 41, "mean"), (4, 130, 65, "none")])
def test_function_matches_torch_float64(B, S, C, reduction):
    """Ragged input and target lengths; (4, 130, 65): 31 windows, a second class tile, one sequence without any frame."""
    T = (S - 8) // 4 + 1
    x, W, b = head_case(B, S, C, seed=S)
    Lmax = max(1, min(T // 2, 9))
    targets, tgt_len = ragged_targets(B, Lmax, C - 1, seed=S + 1)
    in_len = torch.tensor([T, max(T - 1, 1), max(T // 2, 1), 0][:B])
    got = _run(x, W, b, in_len, targets, tgt_len, C - 1, reduction)
    again = _run(x, W, b, in_len, targets, tgt_len, C - 1, reduction)
    rl, logits, rdW, rdb, rdx = oracle_full(x, W, b, in_len, targets, tgt_len, C - 1, reduction)
    assert bool(((got[0].double().view(-1) - rl.view(-1)).abs() <= 1e-5 * rl.view(-1).abs()).all()), (got[0], rl)
    assert rel_err(got[1].double(), rdW) < 1e-4
    assert rel_err(got[2].double(), rdb) < 1e-4
    assert rel_err(got[3].double(), rdx) < 1e-4
    for g, a in zip(got, again):
        assert torch.equal(g, a)
    got_logits = ops.phone_head_logits(x.cuda(), W.cuda(), b.cuda()).cpu()
    assert got_logits.shape == (B, T, C) and rel_err(got_logits.double(), logits) < 1e-5
    if B == 4:
        assert bool((got[3][3] == 0).all()) and bool((rdx[3] == 0).all())      # in_len 0: no gradient reaches its frames
    ops.check_device_errors()


def test_frozen_features_get_no_gradient_buffer():
    x, W, b = head_case(2, 37, 41, seed=3)
    targets, tgt_len = ragged_targets(2, 4, 40, seed=4)
    Wr, br = W.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    xc = x.cuda()
    loss = ops.PhoneHeadCtcFunction.apply(xc, Wr, br, torch.tensor([8, 6]).cuda(), targets.cuda(), tgt_len.cuda(), 40, "sum")
    loss.sum().backward()
    _, _, rdW, rdb, _ = oracle_full(x, W, b, torch.tensor([8, 6]), targets, tgt_len, 40, "sum")
    assert xc.grad is None and rel_err(Wr.grad.cpu().double(), rdW) < 1e-4 and rel_err(br.grad.cpu().double(), rdb) < 1e-4


def test_bad_target_raises_through_check_device_errors():
    x, W, b = head_case(2, 12, 7, seed=5)
    targets = torch.tensor([[1, 6], [2, 3]])                       # 6 is the blank
    loss = ops.PhoneHeadCtcFunction.apply(x.cuda(), W.cuda(), b.cuda(), torch.tensor([2, 2]).cuda(), targets.cuda(),
                                          torch.tensor([2, 1]).cuda(), 6, "none")
    assert torch.isnan(loss[0]) and not torch.isnan(loss[1])
    with pytest.raises(RuntimeError, match="label outside"):
        ops.check_device_errors()
    ops.check_device_errors()


def _module_oracle(crit, x, sizes, label, label_size, reduction):
    """The module's arithmetic in float64 on the CPU: its own torch path, hipHead=False, on a float64 copy."""
    ref = CV.CTCphone_criterion(256, 6, crit.useLSTM, reduction=reduction, hipHead=False).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in crit.state_dict().items()})
    xr = x.double().clone().requires_grad_(True)
    loss = ref(xr, sizes, label, label_size)
    loss.sum().backward()
    head = ref.PhoneCriterionClassifier
    return loss.detach(), head.weight.grad, head.bias.grad, xr.grad


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("lstm", [False, True])
def test_module_paths_agree_with_the_float64_oracle(reduction, lstm):
    torch.manual_seed(7)
    made = CV.CTCphone_criterion(256, 6, lstm, reduction=reduction)
    state = {k: v.clone() for k, v in made.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 45, 256, generator=g)
    sizes, label, label_size = torch.tensor([45, 38, 21]), torch.randint(0, 6, (3, 6), generator=g), torch.tensor([6, 4, 2])
    want = None
    for hip_head, path in ((True, "hip"), (False, "torch")):
        crit = CV.CTCphone_criterion(256, 6, lstm, reduction=reduction, hipHead=hip_head).cuda()
        crit.load_state_dict(state)
        if want is None:
            want = _module_oracle(crit, x, sizes, label, label_size, reduction)
        xr = x.cuda().requires_grad_(True)
        loss = crit(xr, sizes.cuda(), label.cuda(), label_size.cuda())
        assert crit.last_path == path and loss.shape == (1, 1)
        loss.sum().backward()
        head = crit.PhoneCriterionClassifier
        assert abs(loss.item() - want[0].item()) <= 1e-5 * abs(want[0].item()), (path, loss.item(), want[0].item())
        assert rel_err(head.weight.grad.cpu().double(), want[1]) < 1e-4, path
        assert rel_err(head.bias.grad.cpu().double(), want[2]) < 1e-4, path
        assert rel_err(xr.grad.cpu().double(), want[3]) < 1e-4, path
        with torch.no_grad():
            pred = crit.getPrediction(x.cuda(), sizes.cuda())
        assert crit.last_path == path and pred.shape == (3, 10, 7)
    ops.check_device_errors()


def test_hip_head_matches_the_reference_fixture():
    meta = json.load(open(os.path.join(GOLDEN, "phone_head_meta.json")))
    data = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "phone_head.npz")).items()}
    crit = CV.CTCphone_criterion(meta["dimEncoder"], meta["nPhones"], reduction=meta["reduction"], hipHead=True).cuda().eval()
    assert list(crit.state_dict().keys()) == meta["keys"]
    head = crit.PhoneCriterionClassifier
    with torch.no_grad():
        head.weight.copy_(data["weight"])
        head.bias.copy_(data["bias"])
    fs, ls = torch.tensor(meta["feature_size"]).cuda(), torch.tensor(meta["label_size"]).cuda()
    x = data["x"].cuda().requires_grad_(True)
    with torch.no_grad():
        pred = crit.getPrediction(x.detach(), fs)
    loss = crit(x, fs, data["label"].cuda(), ls)
    loss.sum().backward()
    assert crit.last_path == "hip"
    assert rel_err(pred.cpu().double(), data["pred"].double()) < 1e-5
    assert abs(loss.item() - meta["loss"]) <= 1e-5 * abs(meta["loss"])
    assert rel_err(head.weight.grad.cpu().double(), data["dweight"].double()) < 1e-4
    assert rel_err(head.bias.grad.cpu().double(), data["dbias"].double()) < 1e-4
    assert rel_err(x.grad.cpu().double(), data["dx"].double()) < 1e-4
    ops.check_device_errors()


def test_train_then_per_on_the_hip_head(tmp_path, monkeypatch):
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
                    "--in_dim", "256", "--hipHead", "--file_extension", ".npy", "--pathVal", str(tmp_path / "val.txt")]) is None
    assert len(made) == 1 and made[0].hipHead is True and made[0].last_path == "hip"
    assert json.load(open(out / "args_training.json"))["hipHead"] is True
    mean, std = CV.main(["per", str(out)])
    assert len(made) == 2 and made[1].hipHead is True and made[1].last_path == "hip"
    ckpt = torch.load(out / "checkpoint.pt", map_location="cpu")
    assert set(ckpt) == {"classifier", "model", "bestLoss"}
    assert all(k.startswith("module.") for k in ckpt["classifier"]) and all(k.startswith("module.") for k in ckpt["model"])
    assert "module.PhoneCriterionClassifier.weight" in ckpt["classifier"] and math.isfinite(ckpt["bestLoss"])
    assert math.isfinite(mean) and math.isfinite(std) and mean >= 0
    for f in ("args_training.json", "args_validation_0.json", "logs_train.txt", "logs_per_0.txt"):
        assert (out / f).exists(), f
    assert "Average PER" in (out / "logs_per_0.txt").read_text()
    ops.check_device_errors()
