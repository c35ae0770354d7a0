"""Fixture for the supervised criteria (SpeakerCriterion, PhoneCriterion, CTCPhoneCriterion of the reference's
cpc/criterion/criterion.py:182-283) -- tests/golden/supervised.npz + supervised_meta.json.  Runs where the reference is
importable (oracle.ref_import); the fixture holds the REFERENCE's outputs only:

    python tools/make_golden_supervised.py

Every case of tests/supervised_util.CASES is built from the reference's class, loaded with seeded parameters under its own
state-dict keys and run on seeded features and labels (B = 4, S = 128, 41 phones, 12 speakers): loss, accuracy, the gradient of
every parameter, and the gradients of cFeature / encodedData projected on seeded directions.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import supervised_util as U                       # noqa: E402
from oracle import ref_import                     # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def main():
    _, ref_criterion = ref_import.import_reference()
    import cpc.criterion.criterion as RC
    assert all(hasattr(ref_criterion, n) for n in ("SpeakerCriterion", "PhoneCriterion", "CTCPhoneCriterion", "NoneCriterion"))
    plabels, slabels = U.frame_labels(), U.speaker_labels()
    arrays = {"phone_labels": plabels.numpy(), "speaker_labels": slabels.numpy()}
    meta = {"torch": torch.__version__, "B": U.B, "S": U.S, "phones": U.N_PHONES, "speakers": U.N_SPEAKERS, "cases": {}}
    for i, (name, (cls, args, dim)) in enumerate(U.CASES.items()):
        crit = getattr(RC, cls)(*args)
        shapes = {k: list(v.shape) for k, v in crit.state_dict().items()}
        crit.load_state_dict(U.seeded_state(shapes, 300 + i), strict=True)
        c, enc = U.features(dim, 400 + i)
        if name in U.FLOAT64_CASES:        # the reference's CTC in float32 carries ~1e-4 of its own rounding in its gradients
            crit, c, enc = crit.double(), c.double(), enc.double()
        loss, acc, grads, dc, de = U.run(crit, name, c, enc, plabels, slabels)
        P = U.projection(dim).to(c.dtype)
        arrays[f"{name}:loss"] = loss.numpy().astype(np.float32)
        arrays[f"{name}:acc"] = acc.numpy().astype(np.float64)
        for k, g in grads.items():
            if name not in U.FULL_GRADS and g.dim() == 2 and g.shape[1] >= 128:
                g = g @ U.projection(g.shape[1]).to(g.dtype)               # (C, dim) weight gradients of the other cases: projected
            arrays[f"{name}:grad:{k}"] = g.numpy().astype(np.float32)
        if dc is not None:
            arrays[f"{name}:dc"] = (dc @ P).numpy().astype(np.float32)
        if de is not None:
            arrays[f"{name}:de"] = (de @ P).numpy().astype(np.float32)
        meta["cases"][name] = {"class": cls, "args": list(args), "param_seed": 300 + i, "input_seed": 400 + i, "keys": shapes, "float64": name in U.FLOAT64_CASES,
                               "dc_norm": None if dc is None else float(dc.norm()), "de_norm": None if de is None else float(de.norm())}
        print(name, "loss", float(loss), "acc", float(acc), "keys", list(shapes))
    np.savez_compressed(os.path.join(GOLDEN_DIR, "supervised.npz"), **arrays)
    with open(os.path.join(GOLDEN_DIR, "supervised_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
