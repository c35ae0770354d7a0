"""Time the prediction networks behind ``hipPredictors`` (--rnnMode ffd / conv4 / conv8 / conv12 / RNN / LSTM) on an MI355X: the
criterion's forward + backward with the flag on (csrc/pred_conv.hip; csrc/rnn.hip, csrc/lstm.hip) and off (the torch modules:
per head a transpose, a pad, one MIOpen Conv1d, a multiply, a transpose back -- or one nn.RNN / nn.LSTM call -- then one cat: the
parent's path) on the same GPU, same commit, same process.

    python tools/bench_predictors.py [--rounds 9] [--iters 5] [--out profiles/bench_predictors.json]

B = 64, S = 128 (W = 116), K = 12, N = 128: CPCUnsupersivedCriterion(rnnMode)(c, z) with seeded c, z of the model's output
ranges; one call = forward, losses.sum().backward() with gradients to c, z and every predictor parameter.  The two paths
alternate round by round after a warm-up; a round times ``iters`` calls between two device events.  Per mode and path the JSON
holds the median over the rounds, the fastest and slowest round and the spread (max - min) / median; per mode the predictors'
algorithmic FLOPs from the shapes (forward 2 K B W 256 256 ks, backward twice that; ks = 2 for RNN, 8 for LSTM: the input and
recurrent products of one and of four gates), the ratio torch / HIP with ``won`` = the
HIP path's slowest round is faster than the torch path's fastest; and the mean shader clock and socket power sampled in process
during each mode's timed rounds (bench.RsmiSampler; None where the library is missing).  The times are whole criterion steps
(predictors + score kernels), so ``predictor_tflops_if_all_time`` UNDERSTATES the predictor kernels' own rate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import RsmiSampler  # noqa: E402
from cpc_audio_amd.train import build_criterion  # noqa: E402

B, S, K, N = 64, 128, 12, 128
TAPS = {"ffd": 2, "conv4": 4, "conv8": 8, "conv12": 12, "RNN": 2, "LSTM": 8}          # 256 x 256 products per head and frame
ROOF_TFLOPS = 157.0        # exact-f32 MFMA (v_mfma_f32_32x32x2_f32), the arithmetic of csrc/pred_conv.hip


def step(crit, c, z):
    crit.zero_grad(set_to_none=True)
    c.grad = z.grad = None
    losses, _ = crit(c, z, None)
    losses.sum().backward()
    return losses


def time_round(crit, c, z, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step(crit, c, z)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts):
    med = statistics.median(ts)
    return {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "spread": (max(ts) - min(ts)) / med, "rounds": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=B)
    ap.add_argument("--modes", nargs="+", default=list(TAPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predictors: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    c = torch.tanh(torch.randn(args.batch, S, 256, generator=g)).to(dev).requires_grad_(True)        # a GRU's range
    z = torch.randn(args.batch, S, 256, generator=g).to(dev).requires_grad_(True)
    out = {"bench": "predictors_criterion_step", "device": torch.cuda.get_device_name(0), "B": args.batch, "S": S, "W": S - K,
           "K": K, "N": N, "roof_tflops": ROOF_TFLOPS, "rounds": args.rounds, "iters": args.iters, "modes": {}}
    for mode in args.modes:
        torch.manual_seed(1)
        hip = build_criterion(nPredicts=K, negativeSamplingExt=N, rnnMode=mode, hipPredictors=True).to(dev)
        ref = build_criterion(nPredicts=K, negativeSamplingExt=N, rnnMode=mode).to(dev)
        ref.load_state_dict(hip.state_dict())
        runs = [("hip", hip), ("torch", ref)]
        for _, crit in runs:                                     # warm-up: allocator, code objects, MIOpen's choice of kernel
            for _ in range(3):
                step(crit, c, z)
        torch.cuda.synchronize()
        assert hip.wPrediction.last_path == "hip" and ref.wPrediction.last_path == "torch"
        ts = {"hip": [], "torch": []}
        with RsmiSampler(0) as smi:
            for _ in range(args.rounds):                         # alternate between the two paths
                for name, crit in runs:
                    ts[name].append(time_round(crit, c, z, args.iters))
        sclk, power, nsamp = smi.means()
        r = {name: summary(t) for name, t in ts.items()}
        flops = 3 * 2.0 * K * args.batch * (S - K) * 256 * 256 * TAPS[mode]
        r["predictor_flops"] = flops
        r["hip"]["predictor_tflops_if_all_time"] = flops / (r["hip"]["median_ms"] * 1e-3) / 1e12
        r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
        r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
        r["sclk_mhz"], r["power_w"], r["smi_samples"] = sclk, power, nsamp
        with torch.no_grad():                                    # the two paths compute the same thing at the timed size
            lh, lt = step_losses(hip, c, z), step_losses(ref, c, z)
        r["loss_max_abs_diff"] = (lh - lt).abs().max().item()
        out["modes"][mode] = r
        del hip, ref
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def step_losses(crit, c, z):
    """Losses of one forward on fixed negatives (the draws are the criterion's own otherwise)."""
    W = S - K
    gen = torch.Generator().manual_seed(9)
    n = N * W * c.shape[0]
    bi = torch.randint(0, c.shape[0], (n,), generator=gen).to(c.device)
    si = torch.randint(1, S, (n,), generator=gen).to(c.device)
    return crit(c.detach(), z.detach(), None, negatives=(bi, si))[0].float().cpu()


if __name__ == "__main__":
    main()
