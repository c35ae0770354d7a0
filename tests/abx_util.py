"""Shared recipe of the ABX fixture (tools/make_golden_abx.py writes tests/golden/abx.npz + abx_meta.json from it): the item
file text and the per-file features are regenerated from seeds, so the fixture stores no features."""
import json
import os
import random

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TEST_DATA = os.path.join(GOLDEN, "abx_test_data")
STEP = 100            # frames per second
H = 256
N_FILES, T_FILE = 12, 420
PHONES, CONTEXTS, SPEAKERS = ["aa", "b", "iy", "k", "s"], [("p", "t"), ("m", "n"), ("l", "r")], ["s1", "s2", "s3", "s4"]


def item_text(seed=1234):
    """The item file: ~20 items per file, one speaker per file; lengths 1 .. 30 frames plus one of 150 frames."""
    rng = random.Random(seed)
    lines = ["#file onset offset #phone prev-phone next-phone speaker"]
    for f in range(N_FILES):
        spk = SPEAKERS[f % len(SPEAKERS)]
        t = 2
        while True:
            n = 150 if (f == 5 and t == 2) else rng.choice([1, 1, 2, 3, 5, 8, 12, 17, 24, 30])
            if t + n + 2 > T_FILE:
                break
            ph, ctx = rng.choice(PHONES), rng.choice(CONTEXTS)
            lines.append(f"f{f} {(t + 0.2) / STEP:.4f} {(t + n + 0.7) / STEP:.4f} {ph} {ctx[0]} {ctx[1]} {spk}")
            t += n + rng.randint(0, 3)
    return "\n".join(lines) + "\n"


def parse_items(text):
    """[(file, first frame, frames, phone, speaker)] of the item text (the frame cut of ABXFeatureLoader at STEP)."""
    out = []
    for line in text.splitlines()[1:]:
        f, on, off, ph, _, _, spk = line.split()
        i0 = int(np.ceil(STEP * float(on) - 0.5))
        i1 = min(T_FILE, int(np.floor(STEP * float(off) - 0.5)))
        out.append((f, i0, i1 - i0, ph, spk))
    return out


def file_features(text, seed=99):
    """{file id: (1, T_FILE, H) float32}: phone means + speaker offsets + noise, a null frame, and exact duplicates (an item
    whose (phone, speaker, length) was seen before copies the first such item's frames)."""
    g = torch.Generator().manual_seed(seed)
    means = {p: 0.5 * torch.randn(H, generator=g) for p in PHONES}
    offs = {s: 0.6 * torch.randn(H, generator=g) for s in SPEAKERS}
    feats = {f"f{f}": 4.0 * torch.randn(1, T_FILE, H, generator=g) for f in range(N_FILES)}
    items = parse_items(text)
    for f, i0, n, ph, spk in items:
        feats[f][0, i0:i0 + n] += means[ph] + offs[spk]
    f, i0, n, _, _ = items[3]
    feats[f][0, i0] = 0.0                                      # a null frame
    seen = {}
    for f, i0, n, ph, spk in items:                            # exact duplicates inside (phone, speaker) groups
        key = (ph, spk, n)
        if key in seen and n > 1:
            sf, s0 = seen[key]
            feats[f][0, i0:i0 + n] = feats[sf][0, s0:s0 + n]
        else:
            seen[key] = (f, i0)
    return feats


def write_fixture_files(tmp, text, feats):
    """The item file and one .pt per file in ``tmp`` -> (item path, seq_list)."""
    item = os.path.join(tmp, "set.item")
    with open(item, "w") as f:
        f.write(text)
    seq = []
    for k, v in feats.items():
        p = os.path.join(tmp, f"{k}.pt")
        torch.save(v, p)
        seq.append((k, p))
    return item, seq


def load_golden():
    meta = json.load(open(os.path.join(GOLDEN, "abx_meta.json")))
    arrays = dict(np.load(os.path.join(GOLDEN, "abx.npz")))
    return meta, arrays


def csr(arrays, name):
    """Member lists stored as CSR: name:ptr, name:ids -> list of lists."""
    ptr, ids = arrays[f"{name}:ptr"], arrays[f"{name}:ids"]
    return [ids[ptr[i]:ptr[i + 1]].tolist() for i in range(len(ptr) - 1)]
