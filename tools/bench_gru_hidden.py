"""Time the GRU at a hidden width other than 256 on an MI355X: the HIP path (csrc/gru.hip: cpc_gru_*_h through
ops.GruHiddenFunction) against the same module on torch.nn.GRU (MIOpen), same GPU, same commit, same process.

    python tools/bench_gru_hidden.py [--rounds 9] [--iters 3] [--out profiles/bench_gru_hidden.json]

model.CPCAR(D, H, nl, mode GRU, hiddenKernel) forward + backward at B = 64, S = 128 with gradients to x and every parameter,
against the same CPCAR without hiddenKernel: (D, H) in {(256, 128), (256, 512), (512, 512), (40, 64)} at nl = 2 (this package's
default depth) and (256, 512) at nl = 1 (the reference's default).
Protocol of tools/bench_lstm_hidden.py / bench_ar_widths.py: the two paths alternate round by round after a warm-up, a round
times ``iters`` calls between two device events; per path the median, the fastest and the slowest of the rounds, beside the mean
shader clock and power sampled during the rounds.  ``verdict``: "won" only when the HIP path's slowest round beats torch's
fastest, "lost" when its fastest is slower than torch's slowest, else "undecided".  ``paths`` names the recurrence kernels the
HIP side launched (persistent / per_step).  Not timed here: the kernels on their own, the per-step fallback, nl > 2."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_ar_widths import alternate  # noqa: E402
from cpc_audio_amd import ops  # noqa: E402
from cpc_audio_amd.model import CPCAR  # noqa: E402

CASES = [(256, 128, 2), (256, 512, 2), (512, 512, 2), (40, 64, 2), (256, 512, 1)]


def pair(hip_fn, torch_fn, x, dy, rounds, iters):
    last = {}

    def run(fn, key):
        x.grad = None
        y = fn(x)
        y.backward(dy)
        last[key] = y.detach()

    ops.gru_hidden_paths(clear=True)
    r = alternate([("hip", lambda: run(hip_fn, "hip")), ("torch", lambda: run(torch_fn, "torch"))], rounds, iters)
    r["paths"] = sorted(ops.gru_hidden_paths(clear=True))
    r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
    r["verdict"] = "won" if r["hip"]["max_ms"] < r["torch"]["min_ms"] else \
        ("lost" if r["hip"]["min_ms"] > r["torch"]["max_ms"] else "undecided")
    r["y_max_abs_diff"] = (last["hip"] - last["torch"]).abs().max().item()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_hidden: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B, S = 64, 128
    out = {"bench": "gru_hidden_fwdbwd", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "B": B, "S": S, "cases": {}}
    g = torch.Generator().manual_seed(0)
    for D, H, nl in CASES:
        torch.manual_seed(1)
        hip_ar = CPCAR(D, H, False, nl, mode="GRU", hiddenKernel=True).to(dev)
        torch_ar = CPCAR(D, H, False, nl, mode="GRU").to(dev)
        torch_ar.load_state_dict(hip_ar.state_dict())
        assert hip_ar.hip_gru_hidden and not (torch_ar.hip_gru_hidden or torch_ar.hip or torch_ar.hip_in)
        x = torch.randn(B, S, D, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(B, S, H, generator=g).to(dev)

        def call(ar):
            def fn(t):
                ar.zero_grad(set_to_none=True)
                return ar(t)
            return fn

        out["cases"][f"D{D}_H{H}_nl{nl}"] = pair(call(hip_ar), call(torch_ar), x, dy, args.rounds, args.iters)
        del hip_ar, torch_ar, x, dy
        torch.cuda.empty_cache()
    ops.check_device_errors(clear=True)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
