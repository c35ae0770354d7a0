"""The linear probes and supervised criteria at feature widths other than 256 on an MI355X.

  * the C ABI (cpc_probe_*_d, cpc_classifier_*_d, cpc_ctc_forward_d) on the cases of tests/probe_widths_util.py against torch in
    float64 on the CPU, with its bounds, and D = 256 against the 256 entry points bit for bit;
  * the fixture's phone (40 features) and speaker (13 features) runs -- tests/golden/linsep_widths.npz: the float64 reference's
    per-step losses, accuracies and 20-step update, tools/make_golden_linsep_widths.py -- through train_step / val_step on
    ``wideKernel`` criteria with the fused probe step and without it.  Bounds as in test_gpu_linsep.py: per-step loss within
    1e-5 relative, accuracies equal (no row of the fixture has a top-2 margin under 1e-5 of its scale), update after 20 steps
    within 4 x the deviation the float32 reference itself shows from its float64 run;
  * 512 features without a fixture: the same bounds against nn.Linear + cross-entropy + torch.optim.Adam in float64 on the CPU,
    the update's bound from the same torch code in float32;
  * the autograd Functions at 13, 40 and 512 features against float64 with the bounds of test_gpu_supervised.py;
  * the command end to end on an MFCC + no_ar checkpoint (40 features) with --wideKernel."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linsep_util as LU
import linsep_widths_util as UW
import probe_widths_util as U
from cpc_audio_amd import _lib, criterion as C, harness, linear_separability as LS, ops, optim, train

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("D,R,C_", U.CASES)
def test_probe_matches_torch_float64(D, R, C_):
    U.check_probe_case(_lib.get(), U.Case(D, R, C_, seed=1000 * D + R + C_), "cuda")
    ops.check_device_errors()


@pytest.mark.parametrize("name", sorted(U.LAYOUTS))
def test_probe_reads_x_in_place(name):
    D, R, C_, ldx, off = U.LAYOUTS[name]
    U.check_probe_case(_lib.get(), U.Case(D, R, C_, seed=7 + D + off, ldx=ldx, off=off), "cuda")
    ops.check_device_errors()


def test_d256_gives_the_bits_of_the_256_entry_points():
    U.check_d256_gives_the_bits_of_the_256_entry_points(_lib.get(), "cuda")
    ops.check_device_errors()


@pytest.mark.parametrize("D", [13, 40, 512])
def test_classifier_and_ctc_entry_points_match_torch_float64(D):
    U.check_classifier_case(_lib.get(), D, "cuda")
    U.check_ctc_case(_lib.get(), D, "cuda")
    ops.check_device_errors()


# ------------------------------------------------------------------------------------------------- the fixture
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "linsep_widths_meta.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(ROOT, "tests", "golden", "linsep_widths.npz"))


@pytest.fixture
def fused_flag():
    keep = LS.FUSED_PROBE
    yield
    LS.FUSED_PROBE = keep


@pytest.fixture
def probe_calls(monkeypatch):
    calls = {"train": 0, "eval": 0}
    real_train, real_eval = ops.probe_train_step, ops.probe_eval
    monkeypatch.setattr(ops, "probe_train_step", lambda *a, **k: (calls.__setitem__("train", calls["train"] + 1), real_train(*a, **k))[1])
    monkeypatch.setattr(ops, "probe_eval", lambda *a, **k: (calls.__setitem__("eval", calls["eval"] + 1), real_eval(*a, **k))[1])
    return calls


def _run(crit, W, b, train_b, val_b, fused):
    """One batch per train_step / val_step call, so that every step's loss and accuracy come back through the logs.
    -> (steps (n, 2), update of [W, b], optimiser)."""
    LS.FUSED_PROBE = fused
    W0, b0 = W.detach().clone(), b.detach().clone()
    opt = optim.Adam(list(crit.parameters()), lr=LU.LR, betas=LU.BETAS, eps=LU.EPS)
    fm = LU.PassThrough()
    steps = []
    for batch in train_b:
        logs = LS.train_step(fm, crit, [batch], opt)
        steps.append((logs["locLoss_train"][0], logs["locAcc_train"][0]))
    update = torch.cat([(W.detach() - W0).reshape(-1), b.detach() - b0]).double().cpu()
    for batch in val_b:
        logs = LS.val_step(fm, crit, [batch])
        steps.append((logs["locLoss_val"][0], logs["locAcc_val"][0]))
    return np.array(steps), update, opt


def _fixture_run(case, fused):
    crit = UW.build(C, case, device="cuda", wideKernel=True)
    assert crit.hip_wide and not crit.hip_path
    train_b, val_b = UW.batches(case, device="cuda")
    W, b = LU.parameters_of(crit, case)
    assert W.shape[1] == UW.DIMS[case]
    return _run(crit, W, b, train_b, val_b, fused) + (crit,)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", sorted(UW.DIMS))
def test_fixture_runs_match_the_float64_reference(case, fused, fused_flag, probe_calls):
    meta, gold = _golden()
    steps, update, _, _ = _fixture_run(case, fused)
    assert probe_calls == ({"train": LU.N_TRAIN, "eval": LU.N_VAL} if fused else {"train": 0, "eval": 0})
    ref = gold[f"{case}:steps"]
    rel = np.abs(steps[:, 0] - ref[:, 0]) / np.abs(ref[:, 0])
    ref_update = torch.cat([torch.from_numpy(gold[f"{case}:dW"]).reshape(-1), torch.from_numpy(gold[f"{case}:db"])])
    dev = ((update - ref_update).norm() / ref_update.norm()).item()
    bound = 4 * meta["cases"][case]["fp32_update_deviation"]
    print(f"{case} dim {UW.DIMS[case]} fused={fused}: worst loss deviation {rel.max():.3e}, update deviation {dev:.3e} (bound {bound:.3e})")
    assert meta["cases"][case]["close_margin_rows"] == 0 and meta["cases"][case]["dim"] == UW.DIMS[case]
    assert meta["cases"][case]["seed_offset"] == UW.SEED_OFFSET[case]
    assert rel.max() <= 1e-5
    assert np.array_equal(steps[:, 1], ref[:, 1])
    assert dev <= bound
    ops.check_device_errors()


@pytest.mark.parametrize("case", sorted(UW.DIMS))
def test_optimizer_state_after_fused_steps_has_the_layout_of_step(case, fused_flag):
    _, _, opt_f, crit_f = _fixture_run(case, True)
    _, _, opt_u, _ = _fixture_run(case, False)
    sd_f, sd_u = opt_f.state_dict(), opt_u.state_dict()
    assert sorted(sd_f) == sorted(sd_u) and sd_f["param_groups"] == sd_u["param_groups"]
    assert sorted(sd_f["state"]) == sorted(sd_u["state"]) == [0, 1]
    for i in (0, 1):
        assert sorted(sd_f["state"][i]) == sorted(sd_u["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        assert float(sd_f["state"][i]["step"]) == float(sd_u["state"][i]["step"]) == LU.N_TRAIN
        assert sd_f["state"][i]["step"].dtype == sd_u["state"][i]["step"].dtype and not sd_f["state"][i]["step"].is_cuda
        for k in ("exp_avg", "exp_avg_sq"):
            a, b = sd_f["state"][i][k], sd_u["state"][i][k]
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
            assert ((a - b).norm() / b.norm()).item() < 1e-4
    opt_f.zero_grad()                                     # and a plain step() continues from it
    W, b = LU.parameters_of(crit_f, case)
    (W.sum() + b.sum()).backward()
    opt_f.step()
    assert float(opt_f.state_dict()["state"][0]["step"]) == LU.N_TRAIN + 1
    ops.check_device_errors()


# ------------------------------------------------------------------------------------------------- 512 features, no fixture
def _torch_run(train_b, val_b, state, dtype):
    """nn.Linear + cross-entropy + torch.optim.Adam on the CPU: per-step (loss, acc), close-margin rows, the update."""
    lin = torch.nn.Linear(512, LU.N_PHONES).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(state[0].to(dtype))
        lin.bias.copy_(state[1].to(dtype))
    opt = torch.optim.Adam(lin.parameters(), lr=LU.LR, betas=LU.BETAS, eps=LU.EPS)
    steps, close = [], 0
    for i, (x, y) in enumerate(train_b + val_b):
        rows, lab = x.to(dtype).reshape(-1, 512), y.reshape(-1)
        logits = lin(rows)
        loss = F.cross_entropy(logits, lab)
        steps.append((loss.item(), (logits.argmax(1) == lab).double().mean().item()))
        close += U.close_rows(logits.detach().double())
        if i < len(train_b):
            opt.zero_grad()
            loss.backward()
            opt.step()
        if i == len(train_b) - 1:
            update = torch.cat([(lin.weight.detach() - state[0].to(dtype)).reshape(-1), lin.bias.detach() - state[1].to(dtype)]).double()
    return np.array(steps), close, update


@pytest.fixture(scope="module")
def dim512():
    """20 training and 3 validation batches of (2, 64, 512) phone features, the classifier's initial state, and the float64 and
    float32 torch runs on the CPU (computed once)."""
    g = torch.Generator().manual_seed(512)
    emb = torch.randn(LU.N_PHONES, 512, generator=g)
    data = []
    for _ in range(LU.N_TRAIN + LU.N_VAL):
        label = torch.randint(0, LU.N_PHONES, (2, 16), generator=g).repeat_interleave(4, dim=1)
        data.append((torch.randn(2, 64, 512, generator=g) + 0.3 * emb[label], label))
    state = (0.05 * torch.randn(LU.N_PHONES, 512, generator=g), 0.05 * torch.randn(LU.N_PHONES, generator=g))
    train_b, val_b = data[:LU.N_TRAIN], data[LU.N_TRAIN:]
    s64, close, u64 = _torch_run(train_b, val_b, state, torch.float64)
    s32, _, u32 = _torch_run(train_b, val_b, state, torch.float32)
    return dict(train=train_b, val=val_b, state=state, steps=s64, close=close, update=u64,
                fp32_update_deviation=((u32 - u64).norm() / u64.norm()).item())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_dim_512_matches_torch_float64(fused, dim512, fused_flag, probe_calls):
    crit = C.PhoneCriterion(512, LU.N_PHONES, False, wideKernel=True)
    with torch.no_grad():
        crit.PhoneCriterionClassifier.weight.copy_(dim512["state"][0])
        crit.PhoneCriterionClassifier.bias.copy_(dim512["state"][1])
    crit.cuda()
    assert crit.hip_wide
    lin = crit.PhoneCriterionClassifier
    to = lambda bs: [(x.cuda(), y.cuda()) for x, y in bs]
    steps, update, _ = _run(crit, lin.weight, lin.bias, to(dim512["train"]), to(dim512["val"]), fused)
    assert probe_calls == ({"train": LU.N_TRAIN, "eval": LU.N_VAL} if fused else {"train": 0, "eval": 0})
    ref = dim512["steps"]
    rel = np.abs(steps[:, 0] - ref[:, 0]) / np.abs(ref[:, 0])
    dev = ((update - dim512["update"]).norm() / dim512["update"].norm()).item()
    bound = 4 * dim512["fp32_update_deviation"]
    print(f"dim 512 fused={fused}: worst loss deviation {rel.max():.3e}, update deviation {dev:.3e} (bound {bound:.3e})")
    assert dim512["close"] == 0
    assert rel.max() <= 1e-5
    assert np.array_equal(steps[:, 1], ref[:, 1])
    assert dev <= bound
    ops.check_device_errors()


# ------------------------------------------------------------------------------------------------- the autograd path
@pytest.mark.parametrize("D", [13, 40, 512])
def test_autograd_functions_match_torch_float64(D):
    """ClassifierXentFunction with x.requires_grad and CtcXentFunction, B = 4, S = 16: loss 1e-5, gradients 1e-5 (1e-4 behind the
    CTC loss), accuracy equal."""
    Bq, S, n_phones = 4, 16, 41
    g = torch.Generator().manual_seed(40 + D)
    x = torch.randn(Bq, S, D, generator=g)
    y = torch.randint(0, n_phones, (Bq, S // 2), generator=g).repeat_interleave(2, dim=1)
    for ctc in (False, True):
        Cn = n_phones + (1 if ctc else 0)
        W, b = 0.1 * torch.randn(Cn, D, generator=g), 0.1 * torch.randn(Cn, generator=g)
        xg, Wg, bg = (t.cuda().requires_grad_(True) for t in (x, W, b))
        if ctc:
            loss = ops.CtcXentFunction.apply(xg, y.cuda(), Wg, bg)
            rl, _, rdW, rdb, rdx = U.ctc_oracle(x, W, b, y)
            tol = 1e-4
        else:
            loss, acc = ops.ClassifierXentFunction.apply(xg.reshape(Bq * S, D), y.cuda().reshape(-1), Wg, bg)
            rl, logits, rdW, rdb, rdx = U.oracle(x.reshape(Bq * S, D), W, b, y.reshape(-1))
            assert U.close_rows(logits) == 0
            assert acc.dtype == torch.float64 and acc.item() == (logits.argmax(1) == y.reshape(-1)).double().mean().item()
            tol = 1e-5
        assert loss.shape == (1, 1) and loss.dtype == torch.float32
        loss.sum().backward()
        errs = dict(loss=abs(loss.item() - rl.item()) / abs(rl.item()), dW=U.rel_err(Wg.grad.double().cpu(), rdW),
                    db=U.rel_err(bg.grad.double().cpu(), rdb), dX=U.rel_err(xg.grad.double().cpu().view_as(rdx), rdx))
        print(f"autograd D={D} ctc={ctc}: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
        assert errs["loss"] <= 1e-5 and errs["dW"] < tol and errs["db"] < tol and errs["dX"] < tol
    ops.check_device_errors()


def test_criteria_take_cuda_input_through_the_functions():
    """A wideKernel criterion on CUDA fp32 input equals the Function on its parameters; on float64 input it runs its torch ops."""
    torch.manual_seed(3)
    crit = C.SpeakerCriterion(13, 12, wideKernel=True).cuda()
    c = torch.randn(8, 3, 13, device="cuda")
    y = torch.randint(0, 12, (8,), device="cuda")
    loss, acc = crit(c, c, y)
    lin = crit.linearSpeakerClassifier
    ref = ops.ClassifierXentFunction.apply(c[:, -1, :], y, lin.weight, lin.bias)
    assert torch.equal(loss, ref[0]) and torch.equal(acc, ref[1])
    loss.sum().backward()
    assert lin.weight.grad is not None and tuple(lin.weight.grad.shape) == (12, 13)
    loss64, _ = crit.double()(c.double(), c.double(), y)
    assert loss64.dtype == torch.float64 and abs(loss64.item() - loss.item()) <= 1e-5 * abs(loss64.item())
    ops.check_device_errors()


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("phone", [False, True], ids=["speaker", "phone"])
def test_command_end_to_end_on_an_mfcc_checkpoint(tmp_path, phone, fused_flag, probe_calls):
    """The small seeded corpus of test_gpu_linsep.py and a checkpoint of the MFCC encoder without a context network: 40 features."""
    from test_gpu_linsep import _corpus
    db, _ = _corpus(tmp_path)
    cdir = tmp_path / "mfcc"
    cdir.mkdir()
    args = {"hiddenEncoder": 40, "hiddenGar": 40, "arMode": "no_ar", "encoder_type": "mfcc"}
    model = train.build_model(hiddenEncoder=40, hiddenGar=40, arMode="no_ar", encoder_type="mfcc", mfccKernel=True)
    harness.save_checkpoint(model.state_dict(), None, None, None, str(cdir / "checkpoint_0.pt"))
    (cdir / "checkpoint_args.json").write_text(json.dumps(args))
    LS.FUSED_PROBE = True
    random.seed(11)
    torch.manual_seed(11)
    out = tmp_path / "out"
    argv = [str(db), str(tmp_path / "train.txt"), str(tmp_path / "val.txt"), str(cdir / "checkpoint_0.pt"), "--pathCheckpoint", str(out),
            "--file_extension", ".wav", "--n_epoch", "2", "--batchSizeGPU", "4", "--ignore_cache", "--wideKernel"]
    LS.main(argv + (["--pathPhone", str(tmp_path / "phones.txt")] if phone else []))
    assert probe_calls["train"] > 0 and probe_calls["eval"] > 0                     # the fused probe ran
    assert sorted(os.listdir(out)) == ["checkpoint_1.pt", "checkpoint_args.json", "checkpoint_logs.json"]
    with open(out / "checkpoint_logs.json") as f:
        logs = json.load(f)
    state = torch.load(out / "checkpoint_1.pt", map_location="cpu", weights_only=False)
    attr = LU.CASES["phone" if phone else "speaker"][2]
    assert tuple(state["cpcCriterion"][f"{attr}.weight"].shape) == ((7, 40) if phone else (6, 40))
    assert sorted(state) == ["best", "cpcCriterion", "gEncoder", "optimizer"]
    assert state["optimizer"]["state"][0]["step"] == probe_calls["train"]
    assert logs["epoch"] == [0, 1]
    for key in ("locLoss_train", "locLoss_val", "locAcc_train", "locAcc_val"):
        a = np.array(logs[key])
        assert a.shape == (2, 1) and np.isfinite(a).all(), key
    with open(out / "checkpoint_args.json") as f:
        assert json.load(f)["wideKernel"] is True
    ops.check_device_errors()
