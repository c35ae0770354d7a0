"""ABX scoring throughput on the GPU (csrc/abx.hip through cpc_audio_amd.abx): one JSON line.

A synthetic item set of C contexts x S speakers x P phones, 1-6 segments of 3-40 frames per (context, speaker, phone), D = 257
normalised frames, max_size_group = 10, max_x_across = 5: at least 1e5 groups in each pass.  Per mode: planning (host), the
kernels (device events around each launch pair, with the plan's upload), the reduction, groups/s, DTW pairs/s and the frame-
distance product's algorithmic FLOP/s (2 D per frame pair, counted from the plan) against the 157 TF exact-f32 roof.

    python tools/bench_abx.py [--contexts 30 --speakers 8 --phones 24] [--out profiles/abx_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpc_audio_amd import abx, ops    # noqa: E402

F32_ROOF_TF = 157.3


def synthetic(C, S, P, D=256, seed=0):
    rng = np.random.default_rng(seed)
    feats, total = [], 0
    for c in range(C):
        for s in range(S):
            for p in range(P):
                for _ in range(int(rng.integers(1, 7))):
                    n = int(rng.integers(3, 41))
                    feats.append([total, n, c, p, s])
                    total += n
    rng.shuffle(feats := np.asarray(feats, dtype=np.int64))
    ds = abx.ABXFeatureLoader.__new__(abx.ABXFeatureLoader)
    ds.features = feats.tolist()
    g = torch.Generator().manual_seed(seed)
    ds.data = abx.normalize_with_singularity(torch.randn(1, total, D, generator=g))[0]
    ds.feature_dim = D + 1
    ds.context_match = {str(i): i for i in range(C)}
    ds.speaker_match = {str(i): i for i in range(S)}
    ds.phone_match = {str(i): i for i in range(P)}
    return ds


def plan_flops(ds, plan):
    lens = np.asarray(ds.features, dtype=np.int64)[:, 1]
    D = ds.feature_dim
    flops = pairs = 0
    for a, b, x in zip(plan.a, plan.b, plan.x):
        la, lb, lx = lens[a], lens[b], lens[x]
        if plan.symmetric:
            flops += (la.sum() ** 2 - (la ** 2).sum()) // 2 + lx.sum() * lb.sum()
            pairs += len(a) * (len(a) - 1) // 2 + len(x) * len(b)
        else:
            flops += lx.sum() * (la.sum() + lb.sum())
            pairs += len(x) * (len(a) + len(b))
    return 2 * D * int(flops), int(pairs)


def run(ds, mode, reps):
    t0 = time.perf_counter()
    plan = abx.plan_within(ds, 10, seed=1) if mode == "within" else abx.plan_across(ds, 10, 5, seed=1)
    t_plan = time.perf_counter() - t0
    flops, pairs = plan_flops(ds, plan)
    feats = np.asarray(ds.features, dtype=np.int64)
    segs = abx._Segments(ds.data, feats[:, 0], feats[:, 1])
    abx.score_groups(segs, plan.a, plan.b, plan.x, plan.symmetric, 0)          # warm-up
    best, wall = None, None
    for _ in range(reps):
        events = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = abx.score_groups(segs, plan.a, plan.b, plan.x, plan.symmetric, 0, events=events)
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
        k = sum(a.elapsed_time(b) for a, b in events) / 1e3
        best = k if best is None else min(best, k)
        wall = w if wall is None else min(wall, w)
    t0 = time.perf_counter()
    score = abx.reduce_scores(plan, scores.numpy())
    t_red = time.perf_counter() - t0
    ops.check_device_errors()
    return {"groups": len(plan), "dtw_pairs": pairs, "plan_s": round(t_plan, 3), "kernels_s": round(best, 4),
            "score_groups_wall_s": round(wall, 4), "reduce_s": round(t_red, 4), "groups_per_s": round(len(plan) / best),
            "pairs_per_s": round(pairs / best), "distance_tflops": round(flops / best / 1e12, 2),
            "fraction_of_f32_roof": round(flops / best / 1e12 / F32_ROOF_TF, 4), "abx": score}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=30)
    ap.add_argument("--speakers", type=int, default=8)
    ap.add_argument("--phones", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ds = synthetic(a.contexts, a.speakers, a.phones)
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "abx_meta.json")))
    res = {"bench": "abx", "device": torch.cuda.get_device_name(), "D": ds.feature_dim, "segments": len(ds.features),
           "frames": int(ds.data.size(0)), "max_size_group": 10, "max_x_across": 5,
           "within": run(ds, "within", a.reps), "across": run(ds, "across", a.reps),
           "reference_cpu_seconds_per_1k_groups": {
               "where": "the reference's ABX() (Cython DTW) on the CPU of the container that wrote tests/golden/abx.npz, "
                        "fixture set (D = 257, max_size_group 3 / 1000); not a GPU-machine number",
               **{k: round(v, 3) for k, v in meta["reference_cpu"].items() if k.endswith("per_1k_groups")}}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
