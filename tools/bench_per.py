"""PER decoding throughput on the GPU (csrc/ctc_decode.hip through cpc_audio_amd.seq_alignment): one JSON line per run.

Batches of B utterances of T = 250 frames over P = 41 classes (40 phones + blank), beams of n_keep, in float32 -- as perStep
decodes them -- from two kinds of input: peaked rows (softmax of 16 x N(0, 1) logits, a confident classifier: distinct
nonzero scores, the radix select stops after the score bytes) and flat rows (near-uniform: float32 scores underflow to exact
zeros within about 30 frames and every later step is decided by the key bytes).  Per configuration: kernel time of the decode alone and of decode +
alignment (device events, median of --reps), sequences/s, and the reference's measured wall time per beam_search call from
tests/golden/per_meta.json for orientation.  Kernel resources of the two kernels come from tools/kernel_resources.py.

    python tools/bench_per.py [--reps 5] [--out profiles/per_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpc_audio_amd import ops, seq_alignment as SA    # noqa: E402


def inputs(kind, B, T, P, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "peaked":
        x = torch.softmax(torch.randn(B, T, P, generator=g) * 16.0, -1)
    else:
        x = torch.rand(B, T, P, generator=g) + 0.5
        x = x / x.sum(-1, keepdim=True)
    return x.cuda()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                        os.path.join(ROOT, "cpc_audio_amd", "csrc", "ctc_decode.hip")], capture_output=True, text=True)
    return [re.sub(r"\s+", " ", line.strip()) for line in r.stdout.splitlines() if "kernel" in line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--P", type=int, default=41)
    ap.add_argument("--batches", type=str, default="8,1024")
    ap.add_argument("--keeps", type=str, default="20,100")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    T, P, blank = args.T, args.P, args.P - 1
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        lengths = torch.full((B,), T, dtype=torch.int32, device="cuda")
        ref = torch.randint(0, P - 1, (B, 60), dtype=torch.int32, device="cuda")
        ref_len = torch.full((B,), 60, dtype=torch.int32, device="cuda")
        for K in [int(x) for x in args.keeps.split(",")]:
            for kind in ("peaked", "flat"):
                probs = inputs(kind, B, T, P)
                out = {}

                def decode():
                    out["d"] = SA.beam_search_batch(probs, lengths, K, blank)

                def both():
                    lab, ll, _, _ = SA.beam_search_batch(probs, lengths, K, blank)
                    out["p"] = SA.seq_per_batch(ref, ref_len, lab[:, 0], ll[:, 0])
                t_dec = timed(decode, args.reps)
                t_both = timed(both, args.reps)
                ops.check_device_errors()
                zeros = float((out["d"][2][:, 0] == 0).float().mean().item())
                rows.append({"B": B, "T": T, "P": P, "n_keep": K, "input": kind, "decode_ms": round(t_dec, 3),
                             "decode_per_ms": round(t_both, 3), "seq_per_s": round(B / (t_both * 1e-3), 1),
                             "best_score_zero_fraction": zeros})
                print(json.dumps(rows[-1]), flush=True)
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "per_meta.json")))
    result = {"bench": "per_decode", "device": torch.cuda.get_device_name(0), "rows": rows,
              "reference_cpu_seconds_per_call": meta["timing"], "reference_host": meta["host"], "resources": resources()}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
