"""Time the learned-filter-bank encoder on an MI355X: model.LFBEnconder on its HIP path (csrc/lfb.hip) against the module's own
torch path (hip=False: the reference's computation on MIOpen / rocBLAS, what a user would otherwise run) on the same GPU.

    python tools/bench_lfb.py [--rounds 9] [--iters 5] [--out profiles/lfb_bench.json]

D = 256, L = 20480, N in {8, 64}; forward (no_grad) and forward + backward of each path.  Both paths run in ONE process and
alternate round by round after a warm-up; a round times ``iters`` calls between two device events.  Per measurement the JSON
holds the median over the rounds, the fastest and slowest round and the run-to-run spread (max - min) / median; per batch size
the algorithmic FLOPs from the shapes (conv 2 N 2D 400 (L - 399) forward; the backward recomputes it and adds the
weight-gradient product of the same size), the achieved rate against the exact-f32 MFMA roof (157 TF), the
ratio torch / HIP with ``won`` = the HIP path's slowest round is faster than the torch path's fastest, and the peak device
memory of each path above what was allocated before it ran."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc_audio_amd import model  # noqa: E402

D, L = 256, 20480
ROOF_TFLOPS = 157.0        # exact-f32 MFMA (v_mfma_f32_32x32x2_f32), the arithmetic of csrc/lfb.hip


def forward_only(enc, x):
    with torch.no_grad():
        return enc(x)


def forward_backward(enc, x):
    enc.zero_grad(set_to_none=True)
    y = enc(x)
    y.backward(torch.ones_like(y))        # (a fresh gradient tensor per call on both paths alike)
    return y


def time_round(fn, enc, x, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn(enc, x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def peak_memory(fn, enc, x):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(enc, x)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(ts):
    med = statistics.median(ts)
    return {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "spread": (max(ts) - min(ts)) / med, "rounds": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    hip = model.LFBEnconder(D).cuda()
    ref = model.LFBEnconder(D, hip=False).cuda()
    ref.load_state_dict(hip.state_dict())
    out = {"device": torch.cuda.get_device_name(0), "D": D, "L": L, "roof_tflops": ROOF_TFLOPS, "rounds": args.rounds,
           "iters": args.iters, "batches": {}}
    for N in args.batches:
        x = (0.1 * torch.randn(N, 1, L, device="cuda")).clamp_(-1, 1)
        conv_flops = 2.0 * N * 2 * D * 400 * (L - 399)
        flops = {"forward": conv_flops, "forward_backward": 3 * conv_flops}      # forward; recomputed conv + weight gradient
        res = {"flops": flops}
        runs = [("hip", hip), ("torch", ref)]
        for what, fn in (("forward", forward_only), ("forward_backward", forward_backward)):
            for _, enc in runs:                                                  # warm-up: allocator, MIOpen's choice of kernel
                for _ in range(2):
                    fn(enc, x)
            torch.cuda.synchronize()
            ts = {"hip": [], "torch": []}
            for _ in range(args.rounds):                                         # alternate between the two paths
                for name, enc in runs:
                    ts[name].append(time_round(fn, enc, x, args.iters))
            r = {name: summary(t) for name, t in ts.items()}
            r["hip"]["tflops"] = flops[what] / (r["hip"]["median_ms"] * 1e-3) / 1e12
            r["hip"]["share_of_roof"] = r["hip"]["tflops"] / ROOF_TFLOPS
            r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
            r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
            for name, enc in runs:
                r[name]["peak_bytes"] = peak_memory(fn, enc, x)
            res[what] = r
        out["batches"][str(N)] = res
        del x
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
