"""Fixture of the PER evaluation (the reference's cpc/criterion/seq_alignment.py) -- tests/golden/per.npz + per_meta.json.
Runs only where the reference is importable:

    python tools/make_golden_per.py

Stored: every probability table (in its own dtype, so the bits arrive as they were) with the reference's full beam_search
list for it, in float32 and float64 -- peaked tables (a trained classifier), flat tables whose float32 scores underflow to
all-zero ties, tables of multiples of 1/8 with exact non-zero ties, subnormal tables, the reference unit tests' tables, and
cases found by a seed search in which a prefix leaves the beam and comes back while its extension stayed (the tool asserts that
it found one); NeedlemanWunschAlignScore / get_seq_PER on random pairs with integer and float (d, m, r), empty hypotheses
included; collapseLabelChain on random frame labels; CTCphone_criterion.getPrediction and its CTC loss (LSTM, seqNorm
each off and on, seeded weights, eval mode, integer lengths); and the reference's wall time per beam_search call on this host.
"""
import json
import os
import platform
import sys
import time

sys.dont_write_bytecode = True

import numpy as np          # noqa: E402
import torch                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def import_reference_seq_alignment():
    ref_import.import_reference()
    import cpc.criterion.seq_alignment as sa      # noqa: E402
    return sa


def import_reference_cv_eval():
    ref_import.import_reference()
    sys.modules["torchaudio"].load = None
    import cpc.eval.common_voices_eval as cve     # noqa: E402
    return cve


def softmax(x):
    x = x - x.max(axis=1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=1, keepdims=True)


def table(kind, T, P, seed, dtype):
    rng = np.random.default_rng(seed)
    if kind == "peaked":               # a trained classifier: one or two classes dominate each frame
        x = softmax(rng.standard_normal((T, P)) * 4.0)
    elif kind == "flat":               # near-uniform rows: float32 scores underflow to exactly 0
        x = rng.random((T, P)) + 0.5
        x /= x.sum(axis=1, keepdims=True)
    elif kind == "ties":               # multiples of 1/8: exact non-zero ties
        x = rng.integers(0, 9, (T, P)) / 8.0
    elif kind == "subnormal":
        x = rng.random((T, P)) * 1e-20
    elif kind == "uniform":
        x = rng.random((T, P))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=dtype)


def kept_sets(sa, tab, K, blank):
    """The kept list after every step: beam_search on the first t + 1 frames returns exactly the step's kept beams."""
    return [{tuple(b) for _, b in sa.beam_search(tab[:t + 1], K, blank)} for t in range(tab.shape[0])]


def has_reentry(sets, P, blank):
    """A prefix s absent from step t - 1 while s + c was kept there, and both s and s + c kept at step t."""
    for t in range(1, len(sets)):
        prev, cur = sets[t - 1], sets[t]
        for s in cur:
            if s in prev:
                continue
            if any((s + (c,)) in prev and (s + (c,)) in cur for c in range(P) if c != blank):
                return True
    return False


CASES = [  # kind, T, P, n_keep, dtype, seed
    ("peaked", 60, 41, 20, "f32", 1), ("peaked", 16, 128, 100, "f32", 2), ("peaked", 30, 12, 2, "f32", 3),
    ("peaked", 20, 3, 1, "f32", 4), ("peaked", 20, 41, 100, "f64", 5), ("peaked", 40, 12, 20, "f64", 6),
    ("peaked", 24, 128, 1, "f64", 7),
    ("flat", 90, 41, 20, "f32", 11), ("flat", 120, 12, 4, "f32", 12), ("flat", 30, 128, 100, "f32", 13),
    ("flat", 60, 41, 20, "f64", 14), ("flat", 70, 3, 2, "f32", 15),
    ("ties", 10, 5, 4, "f32", 21), ("ties", 12, 12, 20, "f32", 22), ("ties", 8, 41, 100, "f64", 23), ("ties", 14, 3, 2, "f64", 24),
    ("subnormal", 4, 12, 20, "f32", 31), ("subnormal", 6, 41, 20, "f64", 32),
]


def main():
    sa = import_reference_seq_alignment()
    meta = {"host": platform.processor() or platform.machine(), "numpy": np.__version__, "beam": [], "nw": [], "timing": []}
    arrays = {}

    def add_beam(tab, K, blank, kind, note=None):
        idx = len(meta["beam"])
        arrays[f"beam{idx}"] = tab
        out = sa.beam_search(tab, K, blank)
        assert all(type(s) in (np.float32, np.float64) or s == 0 for s, _ in out)
        meta["beam"].append({"kind": kind, "T": tab.shape[0], "P": tab.shape[1], "n_keep": K, "blank": blank,
                             "dtype": "f32" if tab.dtype == np.float32 else "f64", "note": note,
                             "scores": [float(s) for s, _ in out], "labels": [list(map(int, b)) for _, b in out],
                             "all_zero": bool(all(float(s) == 0.0 for s, _ in out))})

    # the reference unit tests' tables (cpc/unit_tests.py: test_beam_search, test_big_beam_search)
    add_beam(np.array([[0.1, 0.2, 0.], [0.4, 0.2, 0.6], [0.01, 0.3, 0.]]), 10, 2, "unit", "test_beam_search")
    add_beam(np.array([[0.1, 0.2, 0., 0., 0., 0., 0., 0.01, 0., 0.1, 0.99, 0.1],
                       [0.1, 0.2, 0.6, 0.1, 0.9, 0., 0., 0.01, 0., 0.9, 1., 0.]]), 10, 11, "unit", "test_big_beam_search")
    for kind, T, P, K, dt, seed in CASES:
        tab = table(kind, T, P, seed, np.float32 if dt == "f32" else np.float64)
        add_beam(tab, K, int(np.random.default_rng(seed + 1000).integers(0, P)), kind)
    # re-entry: a prefix leaves the beam and comes back while its extension stayed
    found = 0
    for seed in range(400):
        rng = np.random.default_rng(10_000 + seed)
        P, K = int(rng.integers(3, 6)), int(rng.integers(2, 5))
        tab = table("uniform", 8, P, 10_000 + seed, np.float32)
        blank = int(rng.integers(0, P))
        if has_reentry(kept_sets(sa, tab, K, blank), P, blank):
            add_beam(tab, K, blank, "reentry", f"seed {10_000 + seed}")
            found += 1
            if found == 3:
                break
    assert found >= 1, "no re-entry case found"

    # Needleman-Wunsch / get_seq_PER
    rng = np.random.default_rng(77)
    params = [(-1, -1, 0), (-0.3, -0.7, 0.25), (-2, 1, 3), (-0.1, -0.1, 0.0)]
    for k in range(60):
        n1, n2 = int(rng.integers(0, 30)), int(rng.integers(0, 30)) if k % 7 else 0
        a, b = rng.integers(0, 6, n1).tolist(), rng.integers(0, 6, n2).tolist()
        d, m, r = params[k % len(params)]
        norm = bool(k % 3)
        try:
            v = sa.NeedlemanWunschAlignScore(a, b, d, m, r, normalize=norm)
            meta["nw"].append({"ref": a, "hyp": b, "d": d, "m": m, "r": r, "normalize": norm, "out": v,
                               "int": isinstance(v, int)})
        except ZeroDivisionError:
            meta["nw"].append({"ref": a, "hyp": b, "d": d, "m": m, "r": r, "normalize": norm, "out": None, "int": False})
    meta["per_unit"] = sa.get_seq_PER([0, 1, 1, 2, 0, 2, 2], [1, 1, 2, 2, 0, 0])

    # collapseLabelChain
    g = torch.Generator().manual_seed(5)
    lab = torch.repeat_interleave(torch.randint(0, 5, (6, 20), generator=g), 3, dim=1)[:, :50]
    out, sizes = sa.collapseLabelChain(lab)
    arrays["collapse:in"], arrays["collapse:out"], arrays["collapse:sizes"] = lab.numpy(), out.numpy(), sizes.numpy()

    # CTCphone_criterion (cpc/eval/common_voices_eval.py): getPrediction and the CTC loss under integer lengths, seeded weights,
    # eval mode; the lengths are those after // downsampling, the loss follows forward() with // 4 and the batch-maximum clamp
    cve = import_reference_cv_eval()
    meta["ctc"] = []
    for k, (lstm, seq_norm) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        torch.manual_seed(100 + k)
        crit = cve.CTCphone_criterion(16, 6, lstm, seqNorm=seq_norm, reduction="sum").eval()
        g = torch.Generator().manual_seed(200 + k)
        x = torch.randn(3, 40, 16, generator=g)
        feature_size = torch.tensor([40, 33, 21])
        label = torch.randint(0, 6, (3, 7), generator=g)
        label_size = torch.tensor([7, 5, 3])
        with torch.no_grad():
            pred = crit.getPrediction(x.clone(), feature_size)
            fs = feature_size // 4
            cut = pred[:, :int(fs.max())]
            fs = torch.clamp(fs, max=cut.size(1))
            loss = crit.lossCriterion(torch.nn.functional.log_softmax(cut, dim=2).permute(1, 0, 2),
                                      label[:, :int(label_size.max())], fs, label_size)
        for name, v in crit.state_dict().items():
            arrays[f"ctc{k}:sd:{name}"] = v.numpy()
        arrays[f"ctc{k}:x"], arrays[f"ctc{k}:pred"] = x.numpy(), pred.numpy()
        arrays[f"ctc{k}:label"] = label.numpy()
        meta["ctc"].append({"LSTM": lstm, "seqNorm": seq_norm, "feature_size": feature_size.tolist(),
                            "label_size": label_size.tolist(), "loss": float(loss), "keys": list(crit.state_dict().keys())})

    # wall time of one reference call on this host (orientation only)
    for T, K in ((60, 20), (200, 20), (100, 100)):
        tab = table("peaked", T, 41, 99, np.float32)
        t0 = time.perf_counter()
        sa.beam_search(tab, K, 40)
        meta["timing"].append({"T": T, "P": 41, "n_keep": K, "seconds": time.perf_counter() - t0})

    np.savez_compressed(os.path.join(GOLDEN, "per.npz"), **arrays)
    with open(os.path.join(GOLDEN, "per_meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(f"{len(meta['beam'])} beam cases ({found} re-entry), {len(meta['nw'])} alignments, timing {meta['timing']}")


if __name__ == "__main__":
    main()
