"""Fixture of the CPC criterion at encoder / context widths other than 256 and with a speaker embedding (the reference's
cpc/criterion/criterion.py, CPCUnsupersivedCriterion) -- tests/golden/criterion_widths.npz + criterion_widths_meta.json.  Runs
only where the reference is importable:

    python tools/make_golden_criterion_widths.py

Three cases (H = hiddenGar, C = hiddenEncoder, E = speakerEmbedding) at B = 2, S = 20, K = 5, N = 16, linear heads:
    h24c40   (24, 40, 0)      C > H: no multiple of 64, one channel block
    h32c72   (32, 72, 0)      two channel blocks
    spk      (16, 16, 8)      5 speakers: the context the heads read is 24 wide
Parameters are oracle.make_golden_predictors.seeded_state over the criterion's state dict in key order; c = randn (B, S, H),
z = relu(randn) (B, S, C), label = randint(nSpeakers).  The negatives are the reference's own draws under torch.manual_seed(seed)
(stored; oracle.cpc_oracle.draw_negative_indices under the same seed reproduces them -- checked here).  Stored per case: c, z,
label, batchIdx, seqIdx, every parameter, losses, acc, gloss and the gradients of (losses * gloss).sum() with respect to c, z and
every parameter.
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np          # noqa: E402
import torch                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cpc_oracle as O  # noqa: E402
from oracle.make_golden_predictors import seeded_state  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
B, S, K, N = 2, 20, 5, 16
CASES = {"h24c40": dict(H=24, C=40, E=0, speakers=0, seed=610),
         "h32c72": dict(H=32, C=72, E=0, speakers=0, seed=620),
         "spk": dict(H=16, C=16, E=8, speakers=5, seed=630)}


def main():
    _, ref_criterion = import_reference()
    arrays, meta = {}, {"torch": torch.__version__, "B": B, "S": S, "K": K, "N": N, "cases": {}}
    W = S - K
    for tag, cs in CASES.items():
        crit = ref_criterion.CPCUnsupersivedCriterion(K, cs["H"], cs["C"], N, mode=None, rnnMode="linear", dropout=False,
                                                      nSpeakers=cs["speakers"], speakerEmbedding=cs["E"], sizeInputSeq=S)
        shapes = {k: tuple(v.shape) for k, v in crit.state_dict().items()}
        crit.load_state_dict(seeded_state(shapes, cs["seed"]), strict=True)
        g = torch.Generator().manual_seed(cs["seed"] + 1)
        c = torch.randn(B, S, cs["H"], generator=g).requires_grad_(True)
        z = torch.relu(torch.randn(B, S, cs["C"], generator=g)).requires_grad_(True)
        label = torch.randint(0, max(cs["speakers"], 1), (B,), generator=g)
        gloss = torch.randn(1, K, generator=g)
        torch.manual_seed(cs["seed"] + 2)
        losses, acc = crit(c, z, label)
        (losses * gloss).sum().backward()
        torch.manual_seed(cs["seed"] + 2)
        bi, si = O.draw_negative_indices(B, S, W, N)
        # the stored draws are the reference's: the oracle formula on them gives the reference's losses
        heads = {k: v.detach() for k, v in crit.state_dict().items()}
        ctx = c.detach()
        if cs["E"]:
            emb = heads["speakerEmb.weight"][label].view(B, 1, cs["E"]).expand(B, S, cs["E"])
            ctx = torch.cat([ctx, emb], dim=2)
        lo, ao = O.criterion_forward(heads, ctx, z.detach(), O.negative_rows(bi, si, B, S, W, N), K)
        assert (lo - losses.detach()).abs().max().item() < 2e-6 and torch.equal(ao, acc.detach()), (tag, lo, losses)
        arrays.update({f"{tag}_c": c.detach().numpy().copy(), f"{tag}_z": z.detach().numpy().copy(), f"{tag}_label": label.numpy().copy(),
                       f"{tag}_batchIdx": bi.numpy().copy(), f"{tag}_seqIdx": si.numpy().copy(),
                       f"{tag}_losses": losses.detach().numpy().copy(), f"{tag}_acc": acc.detach().numpy().copy(),
                       f"{tag}_gloss": gloss.numpy().copy(), f"{tag}_dc": c.grad.numpy().copy(), f"{tag}_dz": z.grad.numpy().copy()})
        for k, p in crit.named_parameters():
            arrays[f"{tag}_param_{k}"] = p.detach().numpy().copy()
            arrays[f"{tag}_grad_{k}"] = p.grad.numpy().copy()
        meta["cases"][tag] = {"H": cs["H"], "C": cs["C"], "E": cs["E"], "speakers": cs["speakers"], "seed": cs["seed"],
                              "draw_seed": cs["seed"] + 2, "keys": list(shapes.keys()), "shapes": shapes}
    path = os.path.join(GOLDEN, "criterion_widths.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(GOLDEN, "criterion_widths_meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print({k: v.shape for k, v in arrays.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
