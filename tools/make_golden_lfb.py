"""Fixture of the learned-filter-bank encoder (the reference's cpc/model.py, LFBEnconder) -- tests/golden/lfb.npz +
lfb_meta.json.  Runs only where the reference is importable:

    python tools/make_golden_lfb.py

Two cases, LFBEnconder(D, normalize=True) in train mode (its instance norm keeps no statistics, so eval mode computes the same):
    small  D = 32,  N = 2, L = 2000: the output y (N, D, 12) and, for a seeded dy, the gradients of conv.weight and conv.bias
    wide   D = 256, N = 1, L = 1040: y (N, D, 6) only
conv.weight and conv.bias are oracle.make_golden_predictors.seeded_state(shapes, seed) over those two keys in state-dict order
(the seeds are in the meta file; the wide case's weights alone would be 800 KB), ``han`` is the module's own buffer and is
stored.  The input is 0.1 * randn clamped to [-1, 1], as the synthetic loader's.
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np          # noqa: E402
import torch                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden_predictors import seeded_state  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"small": dict(D=32, N=2, L=2000, seed=520, grads=True), "wide": dict(D=256, N=1, L=1040, seed=521, grads=False)}


def main():
    ref_model, _ = import_reference()
    arrays, meta = {}, {"torch": torch.__version__, "cases": {}}
    for tag, c in CASES.items():
        enc = ref_model.LFBEnconder(c["D"], normalize=True)
        keys = list(enc.state_dict().keys())
        shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items() if k != "han"}
        state = seeded_state(shapes, c["seed"])
        state["han"] = enc.han.clone()
        enc.load_state_dict(state, strict=True)
        g = torch.Generator().manual_seed(c["seed"] + 1)
        x = (0.1 * torch.randn(c["N"], 1, c["L"], generator=g)).clamp_(-1, 1)
        y = enc(x)
        arrays.update({f"{tag}_x": x.numpy().copy(), f"{tag}_y": y.detach().numpy().copy(), f"{tag}_han": enc.han.numpy().copy()})
        meta["cases"][tag] = {"D": c["D"], "N": c["N"], "L": c["L"], "seed": c["seed"], "keys": keys, "shapes": shapes,
                              "grads": c["grads"]}
        if c["grads"]:
            dy = torch.randn(y.shape, generator=g)
            (y * dy).sum().backward()
            arrays.update({f"{tag}_dy": dy.numpy().copy(), f"{tag}_dweight": enc.conv.weight.grad.numpy().copy(),
                           f"{tag}_dbias": enc.conv.bias.grad.numpy().copy()})
    path = os.path.join(GOLDEN, "lfb.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(GOLDEN, "lfb_meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print({k: v.shape for k, v in arrays.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
