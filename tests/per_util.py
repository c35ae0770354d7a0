"""Shared loading of the PER fixture (tools/make_golden_per.py writes tests/golden/per.npz + per_meta.json)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden():
    meta = json.load(open(os.path.join(GOLDEN, "per_meta.json")))
    arrays = dict(np.load(os.path.join(GOLDEN, "per.npz")))
    return meta, arrays


def beam_cases():
    """[(case meta, table)] of every stored beam_search case."""
    meta, arrays = load_golden()
    return [(c, arrays[f"beam{k}"]) for k, c in enumerate(meta["beam"])]


def same_bits(got, want, dtype):
    return np.asarray(got, dtype=dtype).tobytes() == np.asarray(want, dtype=dtype).tobytes()


def check_list(got, case):
    """got: [(score, labels)] against the fixture's list, scores compared as bits of the case's dtype."""
    dtype = np.float32 if case["dtype"] == "f32" else np.float64
    assert len(got) == len(case["scores"]), (len(got), len(case["scores"]))
    for k, ((s, lab), ws, wl) in enumerate(zip(got, case["scores"], case["labels"])):
        assert list(lab) == wl, (k, list(lab), wl)
        assert same_bits(s, ws, dtype), (k, float(s), ws)
