"""bench.py --dump-outputs: what dump_outputs writes (no GPU: a CPU model stands in for the trained one)."""
import os

import numpy as np
import pytest
import torch

import bench
from cpc_audio_amd.train import build_criterion, build_model


def test_dump_outputs_writes_the_step_results_and_every_parameter_as_float32(tmp_path):
    torch.manual_seed(0)
    model, crit = build_model(), build_criterion()
    losses, acc = torch.rand(1, 12), torch.rand(1, 12)
    out = str(tmp_path / "dump")
    info = bench.dump_outputs(out, losses, acc, model, crit)
    names = {"losses", "accuracies"} | {f"param.criterion.{n}" for n, _ in crit.named_parameters()} \
        | {f"param.model.{n}" for n, _ in model.named_parameters()}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    assert info["arrays"] == len(names) and info["bytes"] <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(np.load(os.path.join(out, "losses.npy")), losses.numpy())
    w = np.load(os.path.join(out, "param.model.gEncoder.conv1.weight.npy"))
    assert w.dtype == np.float32 and np.array_equal(w, model.gEncoder.conv1.weight.detach().numpy())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) < bench.DUMP_LIMIT_BYTES


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "dump"), torch.zeros(1, 12), torch.zeros(1, 12), build_model(), build_criterion())
    assert not (tmp_path / "dump").exists()
