"""Time the MFCC encoder on an MI355X: model.MFCCEncoder on its HIP path (csrc/mfcc.hip) against the module's own torch path
(hip=False: torch.stft, two matmuls and the pointwise steps between them as library kernels -- what a user would otherwise run)
on the same GPU.

    python tools/bench_mfcc.py [--rounds 9] [--iters 10] [--out profiles/mfcc_bench.json]

D = 256, L = 20480, N in {8, 64}; forward under no_grad (the encoder has no backward).  Both paths run in ONE process and
alternate round by round; each path gets a warm-up of its own first (the torch path's first call builds an FFT plan).  A round
times ``iters`` calls between two device events.  Per path the JSON holds the median over the rounds, the fastest and slowest
round and the run-to-run spread (max - min) / median; per batch size the algorithmic FLOPs 2 N F (321 * 322 + 161 M + M D), the
bytes that must move (x, db written and read, y), the achieved rate against the exact-f32 MFMA roof (157 TF, DESIGN.md section
4.17), the ratio torch / HIP with ``won`` = the HIP path's slowest round is faster than the torch path's fastest, the largest
deviation between the two paths' results and the peak device memory of each path above what was allocated before it ran."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc_audio_amd import model, ops  # noqa: E402

D, L = 256, 20480
ROOF_TFLOPS = 157.0        # exact-f32 MFMA (v_mfma_f32_32x32x2_f32), the arithmetic of csrc/mfcc.hip


def forward_only(enc, x):
    with torch.no_grad():
        return enc(x)


def time_round(enc, x, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        forward_only(enc, x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def peak_memory(enc, x):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    forward_only(enc, x)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(ts):
    med = statistics.median(ts)
    return {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "spread": (max(ts) - min(ts)) / med, "rounds": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    hip = model.MFCCEncoder(D).cuda()
    ref = model.MFCCEncoder(D, hip=False).cuda()
    F, M = ops.mfcc_frames(L), ops.mfcc_mels(D)
    out = {"device": torch.cuda.get_device_name(0), "D": D, "L": L, "F": F, "M": M, "roof_tflops": ROOF_TFLOPS,
           "rounds": args.rounds, "iters": args.iters, "batches": {}}
    for N in args.batches:
        x = (0.1 * torch.randn(N, 1, L, device="cuda")).clamp_(-1, 1)
        flops = 2.0 * N * F * (321 * 322 + 161 * M + M * D)
        nbytes = 4.0 * N * (L + 2 * F * M + F * D)
        runs = [("hip", hip), ("torch", ref)]
        for _, enc in runs:                                                      # each path's own warm-up (FFT plan, allocator)
            for _ in range(3):
                forward_only(enc, x)
            torch.cuda.synchronize()
        ts = {"hip": [], "torch": []}
        for _ in range(args.rounds):                                             # alternate between the two paths
            for name, enc in runs:
                ts[name].append(time_round(enc, x, args.iters))
        r = {name: summary(t) for name, t in ts.items()}
        r["flops"], r["bytes"] = flops, nbytes
        r["hip"]["tflops"] = flops / (r["hip"]["median_ms"] * 1e-3) / 1e12
        r["hip"]["share_of_roof"] = r["hip"]["tflops"] / ROOF_TFLOPS
        r["hip"]["gbytes_per_s"] = nbytes / (r["hip"]["median_ms"] * 1e-3) / 1e9
        r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
        r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
        a, b = forward_only(hip, x).double(), forward_only(ref, x).double()
        r["paths_rel_diff"] = ((a - b).norm() / b.norm()).item()
        for name, enc in runs:
            r[name]["peak_bytes"] = peak_memory(enc, x)
        out["batches"][str(N)] = r
        del x
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
