"""Inputs of the linear-separability fixture (tests/golden/linsep.npz + linsep_meta.json, written by tools/make_golden_linsep.py
from the reference's cpc/eval/linear_separability.py) -- seeded, so the fixture holds the reference's results only."""
import torch

B, S, DIM = 8, 128, 256
N_PHONES, N_SPEAKERS = 41, 12
N_TRAIN, N_VAL, N_EPOCHS = 20, 3, 2
LR, BETAS, EPS = 2e-4, (0.9, 0.999), 2e-8

# name -> (criterion class, constructor arguments for a feature width, the classifier's attribute)
CASES = {
    "phone": ("PhoneCriterion", lambda dim: (dim, N_PHONES, False), "PhoneCriterionClassifier"),
    "speaker": ("SpeakerCriterion", lambda dim: (dim, N_SPEAKERS), "linearSpeakerClassifier"),
}
SEEDS = {"phone": 720, "speaker": 800}

# argument lists whose parsed namespaces the fixture records (absolute paths: Path.resolve() leaves them alone)
ARGV = {
    "defaults": ["/data/db", "/data/train.txt", "/data/val.txt", "/ckpt/checkpoint_30.pt", "--nGPU", "1", "--pathCheckpoint", "/out"],
    "all": ["/data/db", "/data/train.txt", "/data/val.txt", "/ckpt/checkpoint_5.pt", "--pathPhone", "/data/phones.txt", "--CTC",
            "--pathCheckpoint", "/out/linsep", "--nGPU", "2", "--batchSizeGPU", "16", "--n_epoch", "3", "--save_step", "2",
            "--debug", "--unfrozen", "--no_pretraining", "--file_extension", ".wav", "--get_encoded", "--lr", "1e-3",
            "--beta1", "0.8", "--beta2", "0.99", "--epsilon", "1e-7", "--ignore_cache", "--size_window", "10240"],
}


class PassThrough(torch.nn.Module):
    """A frozen feature maker whose features are its input: (features, None) -> (features, features, None)."""

    def __init__(self):
        super().__init__()
        self.optimize = False

    def forward(self, batch, label):
        return batch, batch, label


def batches(case, dim=DIM, dtype=torch.float32, device="cpu"):
    """-> (training batches, validation batches): lists of (features (B, S, dim), labels (B, S) phones / (B,) speakers).  The
    features carry a class direction, so the probe has something to learn."""
    n_cls = N_PHONES if case == "phone" else N_SPEAKERS
    g = torch.Generator().manual_seed(SEEDS[case] + dim)
    emb = torch.randn(n_cls, dim, generator=g)
    out = []
    for _ in range(N_TRAIN + N_VAL):
        if case == "phone":
            label = torch.randint(0, n_cls, (B, S // 4), generator=g).repeat_interleave(4, dim=1)   # runs of four frames
            x = torch.randn(B, S, dim, generator=g) + 0.3 * emb[label]
        else:
            label = torch.randint(0, n_cls, (B,), generator=g)
            x = torch.randn(B, S, dim, generator=g) + 0.3 * emb[label][:, None, :]
        out.append((x.to(dtype).to(device), label.to(device)))
    return out[:N_TRAIN], out[N_TRAIN:]


def initial_state(case, dim=DIM):
    """Seeded classifier parameters under the criterion's own state-dict keys."""
    n_cls = N_PHONES if case == "phone" else N_SPEAKERS
    g = torch.Generator().manual_seed(SEEDS[case] + 1)
    attr = CASES[case][2]
    return {f"{attr}.weight": 0.05 * torch.randn(n_cls, dim, generator=g), f"{attr}.bias": 0.05 * torch.randn(n_cls, generator=g)}


def build(module, case, dim=DIM, dtype=torch.float32, device="cpu"):
    """The criterion of ``module`` (the reference's cpc.criterion.criterion or cpc_audio_amd.criterion) for a case, loaded with
    initial_state."""
    cls, args, _ = CASES[case]
    crit = getattr(module, cls)(*args(dim))
    crit.load_state_dict(initial_state(case, dim), strict=True)
    return crit.to(dtype).to(device)


def parameters_of(crit, case):
    lin = getattr(crit, CASES[case][2])
    return lin.weight, lin.bias


def key_tree(state):
    """What a checkpoint_<epoch>.pt holds, without the values: names, shapes, the optimiser's state layout and step count."""
    opt = state["optimizer"]
    return {
        "top": sorted(state.keys()),
        "gEncoder": {k: list(v.shape) for k, v in state["gEncoder"].items()},
        "best": {k: list(v.shape) for k, v in state["best"].items()},
        "cpcCriterion": {k: list(v.shape) for k, v in state["cpcCriterion"].items()},
        "optimizer": sorted(opt.keys()),
        "optimizer.state": {str(i): {k: (list(v.shape) if torch.is_tensor(v) and v.dim() else float(v)) for k, v in sorted(st.items())
                                     if k != "step"} | {"step": float(st["step"])} for i, st in sorted(opt["state"].items())},
        "optimizer.param_groups": [sorted(k for k in g.keys()) for g in opt["param_groups"]],
        "optimizer.params": [list(g["params"]) for g in opt["param_groups"]],
    }
