"""Time the autoregressors behind an encoder of another width than 256 on an MI355X: model.CPCAR(D, 256, ...,
inputKernel=True) -- layer 0's input projection in csrc/in_proj.hip, the HIP recurrences behind it -- against the same CPCAR
without the keywords (torch.nn.GRU / nn.LSTM / nn.RNN, MIOpen) on the same GPU, same commit, same process.

    python tools/bench_ar_widths.py [--rounds 9] [--iters 3] [--out profiles/bench_ar_widths.json]

B = 64, S = 128, D in {13, 40, 64, 512}; GRU with 2 layers, LSTM and RNN with 1; one call = forward + backward with gradients to
x and every parameter.  Protocol of tools/bench_criterion_widths.py: the two paths alternate round by round after a warm-up, a
round times ``iters`` calls between two device events; per path the median, the fastest and the slowest of the rounds; ``won`` =
the HIP path's slowest round beats the other's fastest.
``projection``: the three in_proj.hip products alone at D = 40, N = 768 (the GRU's gate rows), 8192 rows, each against the
256-wide launch it stands in for -- cpc_gemm_nt at K = 256 (forward), cpc_gemm_nt at N = 256, K = 768 (dx) and cpc_gemm_tn
(dW): what the narrow input saves or costs.  The dx baseline is the plain launch; gru.hip's two-layer backward runs that product
with its K walk split over more workgroups (not reachable through the C ABI alone, not timed here)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import RsmiSampler  # noqa: E402
from cpc_audio_amd import _lib, ops  # noqa: E402
from cpc_audio_amd.model import CPCAR  # noqa: E402

B, S = 64, 128
WIDTHS = [13, 40, 64, 512]
CELLS = [("GRU", 2), ("LSTM", 1), ("RNN", 1)]


def summary(ts):
    med = statistics.median(ts)
    return {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "spread": (max(ts) - min(ts)) / med, "rounds": len(ts)}


def time_round(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(runs, rounds, iters):
    for _, fn in runs:                                           # warm-up: allocator, code objects, MIOpen's choice
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in runs}
    with RsmiSampler(0) as smi:
        for _ in range(rounds):
            for name, fn in runs:
                ts[name].append(time_round(fn, iters))
    r = {name: summary(t) for name, t in ts.items()}
    r["rounds_ms"] = ts
    r["sclk_mhz"], r["power_w"], r["smi_samples"] = smi.means()
    return r


def projection(dev, rounds, iters):
    """The three products at D = 40 against the 256-wide GEMM launches, through the C ABI on the current stream."""
    lib = _lib.get()
    M, N, D, H = B * S, 768, 40, 256
    g = torch.Generator().manual_seed(3)
    p = lambda t: t.data_ptr()
    x, x256 = torch.randn(M, D, generator=g).to(dev), torch.randn(M, H, generator=g).to(dev)
    w, w256 = (torch.randn(N, D, generator=g) / 16).to(dev), (torch.randn(N, H, generator=g) / 16).to(dev)
    w256t = w256.t().contiguous()
    bias, dg = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    out, dx, dx256 = torch.empty(M, N, device=dev), torch.empty(M, D, device=dev), torch.empty(M, H, device=dev)
    dw, dw256 = torch.empty(N, D, device=dev), torch.empty(N, H, device=dev)
    scratch = torch.empty(lib.cpc_in_proj_scratch_floats(M, N, D), device=dev)
    part = torch.empty(lib.cpc_gemm_tn_scratch_floats(M, N, H), device=dev)
    st = ops._stream
    runs = {
        "forward": [("in_proj", lambda: lib.check(lib.cpc_in_proj_forward(p(x), D, p(w), p(bias), p(scratch), p(out), M, N, D, st()), "in_proj")),
                    ("gemm_256", lambda: lib.check(lib.cpc_gemm_nt(p(x256), H, p(w256), H, p(bias), p(out), N, M, N, H, st()), "gemm_nt"))],
        "dx": [("in_proj", lambda: lib.check(lib.cpc_in_proj_backward(p(x), D, p(w), p(dg), p(scratch), p(dx), None, M, N, D, st()), "in_proj")),
               ("gemm_256", lambda: lib.check(lib.cpc_gemm_nt(p(dg), N, p(w256t), N, None, p(dx256), H, M, H, N, st()), "gemm_nt"))],
        "dw": [("in_proj", lambda: lib.check(lib.cpc_in_proj_backward(p(x), D, p(w), p(dg), p(scratch), None, p(dw), M, N, D, st()), "in_proj")),
               ("gemm_256", lambda: lib.check(lib.cpc_gemm_tn(p(dg), N, p(x256), H, p(part), p(dw256), M, N, H, 0, st()), "gemm_tn"))],
    }
    res = {"M": M, "N": N, "D": D}
    for name, pair in runs.items():
        r = alternate(pair, rounds, max(iters, 10))
        r["ratio_256_over_in_proj"] = r["gemm_256"]["median_ms"] / r["in_proj"]["median_ms"]
        res[name] = r
    res["forward_out_bytes"], res["dx_dg_bytes"] = 4 * M * N, 4 * M * N
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ar_widths: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    out = {"bench": "ar_widths_fwdbwd", "device": torch.cuda.get_device_name(0), "B": B, "S": S, "rounds": args.rounds,
           "iters": args.iters, "cells": {}}
    g = torch.Generator().manual_seed(0)
    for mode, nl in CELLS:
        for D in WIDTHS:
            torch.manual_seed(1)
            hip_ar = CPCAR(D, 256, False, nl, mode=mode, inputKernel=True, lstmKernel=True, rnnKernel=True).to(dev)
            torch_ar = CPCAR(D, 256, False, nl, mode=mode).to(dev)
            torch_ar.load_state_dict(hip_ar.state_dict())
            assert hip_ar.hip_in and not (torch_ar.hip_in or torch_ar.hip or torch_ar.hip_lstm or torch_ar.hip_rnn)
            x = torch.randn(B, S, D, generator=g).to(dev).requires_grad_(True)
            dy = torch.randn(B, S, 256, generator=g).to(dev)
            last = {}

            def run(ar, key):
                ar.zero_grad(set_to_none=True)
                x.grad = None
                y = ar(x)
                y.backward(dy)
                last[key] = y.detach()

            r = alternate([("hip", lambda: run(hip_ar, "hip")), ("torch", lambda: run(torch_ar, "torch"))], args.rounds, args.iters)
            r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
            r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
            r["y_max_abs_diff"] = (last["hip"] - last["torch"]).abs().max().item()
            out["cells"][f"{mode}_nl{nl}_D{D}"] = r
            del hip_ar, torch_ar, x, dy
            torch.cuda.empty_cache()
    out["projection"] = projection(dev, args.rounds, args.iters)
    ops.check_device_errors(clear=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
