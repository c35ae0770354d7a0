"""Fixture for the linear-separability evaluation at feature widths other than 256 -- tests/golden/linsep_widths.npz +
linsep_widths_meta.json.  Runs where the reference is importable (oracle.ref_import); the fixture holds the REFERENCE's results
only (inputs: tests/linsep_widths_util.py, which is tests/linsep_util.py at its DIMS and seed offsets):

    python tools/make_golden_linsep_widths.py

Built like tools/make_golden_linsep.py, whose one_pass it uses: the reference's train_step and val_step run unmodified on a
pass-through feature maker, its own PhoneCriterion(40, 41, False) / SpeakerCriterion(13, 12) -- the learned-filter-bank width and
the smallest MFCC width -- and torch.optim.Adam(lr=2e-4, eps=2e-8), from linsep_util.initial_state(case, dim) over
linsep_util.batches(case, dim).  Per case:
  * per-step loss and accuracy of the float64 run over one train_step + one val_step;
  * the 20-step parameter update of the float64 run;
  * the float32 run's own deviation from it (``fp32_update_deviation``, ``fp32_loss_deviation``);
  * ``close_margin_rows``: rows whose top-2 logit margin is under 1e-5 of the row's scale -- asserted 0 here, so that the
    accuracies compare exactly (a case that has one gets another seed offset in linsep_widths_util.SEED_OFFSET).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import linsep_util as U                           # noqa: E402
import linsep_widths_util as UW                   # noqa: E402
from oracle import ref_import                     # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


class _AtWidth:
    """linsep_util with ``build`` and ``batches`` taken from linsep_widths_util: what make_golden_linsep.one_pass calls."""

    def __getattr__(self, name):
        return getattr(U, name)

    build = staticmethod(UW.build)
    batches = staticmethod(UW.batches)


def main():
    import make_golden_linsep as G
    ref_import.import_reference()
    import cpc.criterion.criterion as RC
    import cpc.eval.linear_separability as LS
    arrays, meta = {}, {"torch": torch.__version__, "B": U.B, "S": U.S, "n_train": U.N_TRAIN, "n_val": U.N_VAL, "cases": {}}
    for case, dim in UW.DIMS.items():
        G.U = _AtWidth()
        try:
            s64, close, dW64, db64, _, _ = G.one_pass(LS, RC, case, torch.float64)
            s32, _, dW32, db32, _, _ = G.one_pass(LS, RC, case, torch.float32)
        finally:
            G.U = U
        assert tuple(dW64.shape) == ((U.N_PHONES if case == "phone" else U.N_SPEAKERS), dim)
        assert close == 0, (case, close)
        assert np.array_equal(s64[:, 1], s32[:, 1]), case                      # the accuracies do not depend on the precision
        u64, u32 = torch.cat([dW64.reshape(-1), db64]), torch.cat([dW32.reshape(-1).double(), db32.double()])
        dev_update = float((u32 - u64).norm() / u64.norm())
        dev_loss = float(np.max(np.abs(s32[:, 0] - s64[:, 0]) / np.abs(s64[:, 0])))
        arrays[f"{case}:steps"] = s64
        arrays[f"{case}:dW"] = dW64.numpy()
        arrays[f"{case}:db"] = db64.numpy()
        meta["cases"][case] = {"dim": dim, "close_margin_rows": close, "fp32_update_deviation": dev_update,
                               "seed_offset": UW.SEED_OFFSET[case], "fp32_loss_deviation": dev_loss}
        print(case, dim, "fp32 deviation: update", dev_update, "loss", dev_loss, "first / last loss", s64[0, 0], s64[U.N_TRAIN - 1, 0])
    np.savez_compressed(os.path.join(GOLDEN_DIR, "linsep_widths.npz"), **arrays)
    with open(os.path.join(GOLDEN_DIR, "linsep_widths_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
