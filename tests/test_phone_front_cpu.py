"""The PER phone classifier's front without a GPU: the surface of CTCphone_criterion(hipFront=...), the command line, and the
torch front on the CPU against the reference's stored results (tests/golden/phone_front.npz, tools/make_golden_phone_front.py:
the reference's CTCphone_criterion(256, 6, LSTM, seqNorm=True) in eval(), LSTM off and on)."""
import json

import pytest
import torch

from cpc_audio_amd import common_voices_eval as CV
from seqnorm_util import check_against_golden, golden, golden_criterion


def test_hip_front_keeps_the_state_dict_and_refuses_other_widths():
    assert CV.HIP_FRONT_DEFAULT is False
    torch.manual_seed(0)
    plain = CV.CTCphone_criterion(256, 6, LSTM=True, seqNorm=True, dropout=True)
    hip = CV.CTCphone_criterion(256, 6, LSTM=True, seqNorm=True, dropout=True, hipFront=True)
    off = CV.CTCphone_criterion(256, 6, hipFront=False)
    assert list(plain.state_dict()) == list(hip.state_dict()) == list(off.state_dict())
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == {k: tuple(v.shape) for k, v in hip.state_dict().items()}
    hip.load_state_dict(plain.state_dict(), strict=True)
    assert hip.hipFront is True and plain.hipFront is None and off.hipFront is False
    assert hip.last_front is None and hip.last_channel_scale is None
    with pytest.raises(NotImplementedError):
        CV.CTCphone_criterion(16, 6, seqNorm=True, hipFront=True)
    CV.CTCphone_criterion(16, 6, seqNorm=True, hipFront=None)
    CV.CTCphone_criterion(16, 6, seqNorm=True, hipFront=False)
    CV.CTCphone_criterion(256, 6, sizeKernel=4, hipFront=True, hipHead=False)         # the front does not depend on the head


def test_cpu_features_take_the_torch_front_and_hip_front_true_refuses_them():
    torch.manual_seed(1)
    x = torch.randn(2, 20, 256)
    sizes, label, label_size = torch.tensor([20, 16]), torch.tensor([[1, 2], [3, 0]]), torch.tensor([2, 1])
    auto = CV.CTCphone_criterion(256, 6, LSTM=True, seqNorm=True, dropout=True).eval()
    off = CV.CTCphone_criterion(256, 6, LSTM=True, seqNorm=True, dropout=True, hipFront=False).eval()
    off.load_state_dict(auto.state_dict())
    assert torch.equal(auto(x, sizes, label, label_size), off(x, sizes, label, label_size))
    assert auto.last_front == "torch" and off.last_front == "torch" and auto.last_channel_scale is None
    assert torch.equal(auto.getPrediction(x, sizes), off.getPrediction(x, sizes))
    bare = CV.CTCphone_criterion(256, 6, dropout=True).eval()                          # dropout in eval(): no front op at all
    bare.getPrediction(x, sizes)
    assert bare.last_front is None
    bare.train().getPrediction(x, sizes)
    assert bare.last_front == "torch"
    hip = CV.CTCphone_criterion(256, 6, seqNorm=True, hipFront=True, hipHead=False)
    with pytest.raises(NotImplementedError):
        hip(x, sizes, label, label_size)
    with pytest.raises(NotImplementedError):
        hip.getPrediction(x, sizes)
    CV.CTCphone_criterion(256, 6, hipFront=True, hipHead=False).getPrediction(x, sizes)    # no front op: nothing to refuse


def test_the_torch_front_runs_the_ops_it_ran_before():
    """With the front folded into one method the torch path draws the same dropout bits and gives the same numbers as the
    inline code it replaces (seqNorm loop, LSTM, Dropout2d on the (B, 256, S) view, Conv1d)."""
    torch.manual_seed(2)
    x = torch.randn(3, 24, 256) + 3.0
    sizes = torch.tensor([24, 17, 9])
    crit = CV.CTCphone_criterion(256, 6, LSTM=True, seqNorm=True, dropout=True, hipHead=False, hipFront=False).train()
    torch.manual_seed(3)
    got = crit.getPrediction(x, sizes)
    torch.manual_seed(3)
    rows = []
    for b in range(3):
        size = int(sizes[b])
        m = x[b, :size].mean(dim=0, keepdim=True)
        v = x[b, :size].var(dim=0, keepdim=True)
        rows.append((x[b] - m) / torch.sqrt(v + crit.epsilon))
    f = crit.conv1(torch.stack(rows))[0].permute(0, 2, 1)
    want = crit.PhoneCriterionClassifier(crit.dropout(f)).permute(0, 2, 1)
    assert torch.equal(got, want)


def test_train_takes_the_hip_front_switch_and_per_reads_it_back(tmp_path):
    base = ["train", "db", "phones.txt", "ID"]
    assert CV.parse_args(base).hipFront is None
    assert CV.parse_args(base + ["--hipFront"]).hipFront is True
    assert CV.parse_args(base + ["--no-hipFront"]).hipFront is False
    assert CV.parse_args(base + ["--hipFront", "--no-hipHead"]).hipHead is False
    stored_args = json.loads(json.dumps(vars(CV.parse_args(base + ["--hipFront", "--LSTM"]))))     # what _main writes
    assert stored_args["hipFront"] is True
    for stored in (True, False, None):
        (tmp_path / "args_training.json").write_text(json.dumps({"pathDB": "db", "file_extension": ".npy", "pathPhone": "p",
                                                                 "pathVal": "v", "pathCheckpoint": "ID", "no_pretraining": False,
                                                                 "hipFront": stored}))
        args = CV.get_PER_args(CV.parse_args(["per", str(tmp_path)]))
        assert args.hipFront is stored
    (tmp_path / "args_training.json").write_text(json.dumps({"pathDB": "db", "file_extension": ".npy", "pathPhone": "p",
                                                             "pathVal": "v", "pathCheckpoint": "ID", "no_pretraining": False}))
    assert CV.get_PER_args(CV.parse_args(["per", str(tmp_path)])).hipFront is None     # a run of an earlier version


@pytest.mark.parametrize("lstm", [False, True], ids=["plain", "lstm"])
def test_the_torch_front_reproduces_the_reference_fixture(lstm):
    """The same torch ops on the same CPU as the reference: 1e-5 on predictions, 1e-4 on gradients."""
    arrays, meta = golden()
    crit = golden_criterion(meta, lstm, hipFront=False, hipHead=False)
    check_against_golden(crit, arrays, meta, lstm, "cpu", 1e-5, 1e-4)
    assert crit.last_front == "torch" and crit.last_path == "torch"
