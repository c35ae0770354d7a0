"""Time the CPC criterion at encoder / context widths other than 256 on an MI355X: CPCUnsupersivedCriterion on the
width-parametric score kernels (csrc/nce_wide.hip) against oracle.cpc_oracle.criterion_forward on the same CUDA tensors and
weights under autograd -- this package's torch statement of the reference formula (cpc/criterion/criterion.py:108-116, 245-257)
with the negatives gathered once -- on the same GPU, same commit, same process.

    python tools/bench_criterion_widths.py [--rounds 9] [--iters 3] [--out profiles/bench_criterion_widths.json]

B = 64, S = 128 (W = 116), K = 12, N = 128 for (H, C) = (256, 40), (256, 128), (512, 512), linear heads; one call = the criterion
forward on fixed draws plus losses.sum().backward() with gradients to c, z and every head.  Protocol of
tools/bench_predictors.py: the two paths alternate round by round after a warm-up, a round times ``iters`` calls between two
device events; per path the median, the fastest and the slowest of the rounds; ``won`` = the HIP path's slowest round beats the
other's fastest.  One more row at (256, 256): ops.InfoNCEWideScoresFunction against ops.InfoNCEScoresFunction under
cpc_set_nce_fused(0) on given predictions -- the same algorithm at four channel blocks (there ``won`` reads: the new kernels'
slowest round beats the plain kernels' fastest); ``--only-256`` runs that row alone (profiling)."""
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
from cpc_audio_amd.train import build_criterion  # noqa: E402
from oracle import cpc_oracle as O  # noqa: E402

B, S, K, N = 64, 128, 12, 128
WIDTHS = [(256, 40), (256, 128), (512, 512)]


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
    for _, fn in runs:                                           # warm-up: allocator, code objects, the BLAS library's choice
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=B)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-256", action="store_true", help="the (256, 256) row alone (profiling runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_criterion_widths: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    Bn, W = args.batch, S - K
    out = {"bench": "criterion_widths_step", "device": torch.cuda.get_device_name(0), "B": Bn, "S": S, "W": W, "K": K, "N": N,
           "rounds": args.rounds, "iters": args.iters, "widths": {}}
    g = torch.Generator().manual_seed(0)
    bi, si = O.draw_negative_indices(Bn, S, W, N, generator=g)
    neg = (bi.to(dev), si.to(dev))
    for H, C in ([] if args.only_256 else WIDTHS):
        torch.manual_seed(1)
        crit = build_criterion(nPredicts=K, hiddenGar=H, hiddenEncoder=C, negativeSamplingExt=N).to(dev)
        c = torch.tanh(torch.randn(Bn, S, H, generator=g)).to(dev).requires_grad_(True)
        z = torch.relu(torch.randn(Bn, S, C, generator=g)).to(dev).requires_grad_(True)
        heads = dict(crit.named_parameters())
        last = {}

        def hip():
            crit.zero_grad(set_to_none=True)
            c.grad = z.grad = None
            losses, _ = crit(c, z, None, negatives=neg)
            losses.sum().backward()
            last["hip"] = losses.detach()

        def torch_statement():
            crit.zero_grad(set_to_none=True)
            c.grad = z.grad = None
            rows = O.negative_rows(neg[0], neg[1], Bn, S, W, N)
            losses, _ = O.criterion_forward(heads, c, z, rows, K)
            losses.sum().backward()
            last["torch"] = losses.detach()

        r = alternate([("hip", hip), ("torch", torch_statement)], args.rounds, args.iters)
        r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
        r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
        r["loss_max_abs_diff"] = (last["hip"].float() - last["torch"].float()).abs().max().item()
        r["v_bytes"] = 4 * Bn * W * (N + K) * ops.nce_wide_padded_width(C)
        out["widths"][f"{H}x{C}"] = r
        del crit, c, z, heads
        torch.cuda.empty_cache()
    # (256, 256): the new kernels against the plain scores path (cpc_nce_scores_* with the two-pass kernels) on given predictions
    lib = _lib.get()
    pred = (2.0 * torch.randn(Bn, W, K * 256, generator=g)).to(dev).requires_grad_(True)
    z = torch.relu(torch.randn(Bn, S, 256, generator=g)).to(dev).requires_grad_(True)
    ext, perm, row_ptr = ops.prepare_negatives(neg[0], neg[1], Bn, S, K, N)
    last = {}

    def wide():
        pred.grad = z.grad = None
        losses, _ = ops.InfoNCEWideScoresFunction.apply(pred, z, ext, perm, row_ptr, 256, N)
        losses.sum().backward()
        last["wide"] = losses.detach()

    def plain():
        pred.grad = z.grad = None
        losses, _ = ops.InfoNCEScoresFunction.apply(pred, z, ext, perm, row_ptr, N)
        losses.sum().backward()
        last["plain"] = losses.detach()

    lib.check(lib.cpc_set_nce_fused(0), "set_nce_fused")
    try:
        r = alternate([("wide", wide), ("plain", plain)], args.rounds, args.iters)
    finally:
        lib.cpc_set_nce_fused(_lib.DEFAULT_NCE_FUSED)
    r["ratio_plain_over_wide"] = r["plain"]["median_ms"] / r["wide"]["median_ms"]
    r["won"] = r["wide"]["max_ms"] < r["plain"]["min_ms"]
    r["loss_max_abs_diff"] = (last["wide"] - last["plain"]).abs().max().item()
    out["scores_256x256"] = r
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
