"""Fixture for the linear-separability evaluation -- tests/golden/linsep.npz + linsep_meta.json.  Runs where the reference is
importable (oracle.ref_import); the fixture holds the REFERENCE's results only (inputs: tests/linsep_util.py):

    python tools/make_golden_linsep.py

The reference's cpc/eval/linear_separability.py runs unmodified -- train_step, val_step, run and parse_args -- on a pass-through
feature maker, lists of (features, label) batches, its own PhoneCriterion(256, 41, False) / SpeakerCriterion(256, 12) and
torch.optim.Adam(lr=2e-4, eps=2e-8).  Per case (B = 8, S = 128, 20 training batches, 3 validation batches):
  * per-step loss and accuracy of the float64 run (a forward hook on the criterion) over one train_step + one val_step;
  * the parameter update W_20 - W_0, b_20 - b_0 of the float64 run;
  * the float32 run's own deviation from it: relative norm of the update difference, largest relative loss difference;
  * the number of rows whose top-2 logit margin is under 1e-5 of the row's scale (asserted 0: accuracies compare exactly);
  * what run() wrote over 2 epochs: file names, the checkpoint's key tree, the logs JSON.
And vars(parse_args(argv)) for the argument lists of linsep_util.ARGV.
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import linsep_util as U                           # noqa: E402
from oracle import ref_import                     # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def one_pass(LS, RC, case, dtype):
    """One train_step + one val_step of the reference -> per-step (loss, acc), close-margin rows, the update."""
    crit = U.build(RC, case, dtype=dtype)
    train, val = U.batches(case, dtype=dtype)
    W, b = U.parameters_of(crit, case)
    W0, b0 = W.detach().clone(), b.detach().clone()
    steps, close = [], [0]

    def hook(module, inputs, outputs):
        steps.append((float(outputs[0].detach().mean()), float(outputs[1].detach().mean())))
        with torch.no_grad():
            c = inputs[0]
            rows = c[:, -1, :] if case == "speaker" else c.reshape(-1, c.shape[-1])
            logits = torch.nn.functional.linear(rows.double(), W.double(), b.double())
            top2 = logits.topk(2, dim=1).values
            scale = logits.abs().max(dim=1).values.clamp_min(1e-30)
            close[0] += int(((top2[:, 0] - top2[:, 1]) < 1e-5 * scale).sum())

    crit.register_forward_hook(hook)
    fm = U.PassThrough()
    opt = torch.optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    logs_train = LS.train_step(fm, crit, train, opt)
    dW, db = (W.detach() - W0).clone(), (b.detach() - b0).clone()
    logs_val = LS.val_step(fm, crit, val)
    return np.array(steps, dtype=np.float64), close[0], dW, db, logs_train, logs_val


def files_of_run(LS, RC, case):
    crit = U.build(RC, case)
    train, val = U.batches(case)
    opt = torch.optim.Adam(list(crit.parameters()), lr=U.LR, betas=U.BETAS, eps=U.EPS)
    logs = {"epoch": [], "iter": [], "saveStep": U.N_EPOCHS}
    with tempfile.TemporaryDirectory() as td:
        LS.run(U.PassThrough(), crit, train, val, opt, logs, U.N_EPOCHS, os.path.join(td, "checkpoint"))
        names = sorted(os.listdir(td))
        state = torch.load(os.path.join(td, f"checkpoint_{U.N_EPOCHS - 1}.pt"), map_location="cpu", weights_only=False)
        with open(os.path.join(td, "checkpoint_logs.json")) as f:
            written = json.load(f)
    return names, U.key_tree(state), written


def main():
    ref_import.import_reference()
    import cpc.criterion.criterion as RC
    import cpc.eval.linear_separability as LS
    arrays, meta = {}, {"torch": torch.__version__, "B": U.B, "S": U.S, "n_train": U.N_TRAIN, "n_val": U.N_VAL, "epochs": U.N_EPOCHS,
                        "cases": {}, "args": {}}
    for case in U.CASES:
        s64, close, dW64, db64, lt, lv = one_pass(LS, RC, case, torch.float64)
        s32, _, dW32, db32, _, _ = one_pass(LS, RC, case, torch.float32)
        assert close == 0, (case, close)
        assert np.array_equal(s64[:, 1], s32[:, 1]), case                      # the accuracies do not depend on the precision
        u64, u32 = torch.cat([dW64.reshape(-1), db64]), torch.cat([dW32.reshape(-1).double(), db32.double()])
        dev_update = float((u32 - u64).norm() / u64.norm())
        dev_loss = float(np.max(np.abs(s32[:, 0] - s64[:, 0]) / np.abs(s64[:, 0])))
        names, tree, written = files_of_run(LS, RC, case)
        arrays[f"{case}:steps"] = s64
        arrays[f"{case}:dW"] = dW64.numpy()
        arrays[f"{case}:db"] = db64.numpy()
        meta["cases"][case] = {"close_margin_rows": close, "fp32_update_deviation": dev_update, "fp32_loss_deviation": dev_loss,
                               "reference_logs_train": {k: np.asarray(v).tolist() for k, v in lt.items()},
                               "reference_logs_val": {k: np.asarray(v).tolist() for k, v in lv.items()},
                               "files": names, "checkpoint": tree, "logs": written}
        print(case, "fp32 deviation: update", dev_update, "loss", dev_loss, "first / last loss", s64[0, 0], s64[U.N_TRAIN - 1, 0])
    for name, argv in U.ARGV.items():
        meta["args"][name] = vars(LS.parse_args(list(argv)))
    np.savez_compressed(os.path.join(GOLDEN_DIR, "linsep.npz"), **arrays)
    with open(os.path.join(GOLDEN_DIR, "linsep_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
