"""Time the linear probe on precomputed features at feature widths other than 256 -> profiles/bench_probe_widths.json.

D in {13, 40, 64, 512}; phone: 41 classes on B * 128 rows, speaker: 251 classes on the B last frames of (B, 128, D), B = 8 and 64.
Three variants alternate in one process, each timed by device events around --iters steps after warm-up, --rounds times:
  fused    ops.probe_train_step (cpc_probe_train_step_d): classifier, loss, accuracy, gradients and Adam in one C call
  unfused  the wideKernel criterion's autograd Function (cpc_classifier_*_d) + optim.Adam.step()
  torch    nn.Linear + F.cross_entropy + torch.optim.Adam
and, at D = 256, cpc_probe_train_step_d (probe_wide_kernel) against cpc_probe_train_step (probe_tile_kernel) through the C ABI
on the same shapes.  Per pair: median, minimum and maximum of the rounds; ``won`` only where the fused path's slowest round beats
the torch path's fastest; the mean shader clock and socket power sampled in process during the pair's rounds (bench.RsmiSampler;
None where the library is missing).  Before the timing every variant's loss on the same state is compared.  Not part of bench.py.
usage: python tools/bench_probe_widths.py [--iters N] [--rounds N] [--out PATH]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import RsmiSampler  # noqa: E402
from cpc_audio_amd import _lib, ops, optim  # noqa: E402
from cpc_audio_amd.criterion import PhoneCriterion, SpeakerCriterion  # noqa: E402

S = 128
WIDTHS = (13, 40, 64, 512)
KINDS = (("phone", 41), ("speaker", 251))
BATCHES = (8, 64)


def timeit(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}


def rounds_of(variants, iters, rounds):
    times = {name: [] for name, _ in variants}
    with RsmiSampler(0) as smi:
        for _ in range(rounds):                           # the variants alternate: drift of the machine hits them alike
            for name, fn in variants:
                times[name].append(timeit(fn, iters))
    sclk, power, nsamp = smi.means()
    out = {name: summary(ts) for name, ts in times.items()}
    out["sclk_mhz"], out["power_w"], out["smi_samples"] = sclk, power, nsamp
    return out


def widths_pair(kind, C, B, D, dev, iters, rounds):
    torch.manual_seed(D + B)
    feats = torch.randn(B, S, D, device=dev)
    label = torch.randint(0, C, (B, S) if kind == "phone" else (B,), device=dev)
    crits = [(PhoneCriterion(D, C, False, wideKernel=True) if kind == "phone" else SpeakerCriterion(D, C, wideKernel=True)).to(dev)
             for _ in range(2)]
    assert all(c.hip_wide for c in crits)
    lins = [c.PhoneCriterionClassifier if kind == "phone" else c.linearSpeakerClassifier for c in crits]
    ref = torch.nn.Linear(D, C).to(dev)
    with torch.no_grad():
        for lin in lins:
            lin.weight.copy_(ref.weight)
            lin.bias.copy_(ref.bias)
    opts = [optim.Adam(c.parameters(), lr=2e-4, eps=2e-8) for c in crits]
    ropt = torch.optim.Adam(ref.parameters(), lr=2e-4, eps=2e-8)
    accum = torch.zeros(2, dtype=torch.float64, device=dev)
    bufs = (torch.empty(1, 1, device=dev), torch.empty(1, 1, device=dev, dtype=torch.float64))
    x, y = (feats.reshape(-1, D), label.view(-1)) if kind == "phone" else (feats[:, -1, :], label)

    def fused():
        ops.probe_train_step(x, y, lins[0].weight, lins[0].bias, opts[0], accum=accum, out=bufs)

    def unfused():
        opts[1].zero_grad()
        loss, acc = crits[1](feats, feats, label)
        loss.sum().backward()
        opts[1].step()
        accum[0] += loss.detach().mean().double()
        accum[1] += acc.detach().mean().double()

    def torch_form():
        ropt.zero_grad()
        pred = ref(x)
        loss = F.cross_entropy(pred, y)
        acc = (pred.max(1)[1] == y).double().mean()
        loss.backward()
        ropt.step()
        accum[0] += loss.detach().double()
        accum[1] += acc

    # the three compute the same thing at the timed size: the loss of the shared initial state
    with torch.no_grad():
        l_f = ops.probe_eval(x, y, lins[0].weight, lins[0].bias)[0].item()
        l_u = crits[1](feats, feats, label)[0].item()
        l_t = F.cross_entropy(ref(x), y).item()
    r = rounds_of((("fused", fused), ("unfused", unfused), ("torch", torch_form)), iters, rounds)
    r["loss_max_rel_diff"] = max(abs(l_f - l_t), abs(l_u - l_t)) / abs(l_t)
    r["won"] = r["fused"]["max_ms"] < r["torch"]["min_ms"]
    r["unfused_won"] = r["unfused"]["max_ms"] < r["torch"]["min_ms"]
    r["ratio_torch_over_fused"] = round(r["torch"]["median_ms"] / r["fused"]["median_ms"], 3)
    return r


def d256_pair(kind, C, B, dev, iters, rounds):
    """cpc_probe_train_step_d at D = 256 against cpc_probe_train_step, through the C ABI on the same buffers' shapes."""
    lib = _lib.get()
    torch.manual_seed(256 + B)
    D = 256
    feats = torch.randn(B, S, D, device=dev)
    R = B * S if kind == "phone" else B
    x_ptr, ldx = (feats.data_ptr(), D) if kind == "phone" else (feats[:, -1, :].data_ptr(), S * D)
    y = torch.randint(0, C, (R,), device=dev)
    sizes = (ctypes.c_long * 3)()
    lib.check(lib.cpc_probe_layout_d(R, C, D, sizes), "probe_layout_d")
    state = {}
    for name in ("wide", "tile"):
        torch.manual_seed(1)
        state[name] = dict(W=0.05 * torch.randn(C, D, device=dev), b=torch.zeros(C, device=dev), mW=torch.zeros(C, D, device=dev),
                           vW=torch.zeros(C, D, device=dev), mb=torch.zeros(C, device=dev), vb=torch.zeros(C, device=dev),
                           ws=torch.empty(sizes[0], device=dev), loss=torch.empty(1, device=dev),
                           acc=torch.empty(1, device=dev, dtype=torch.float64))
    bc1, bc2s = 1.0 - 0.9 ** 3, math.sqrt(1.0 - 0.999 ** 3)
    stream = torch.cuda.current_stream().cuda_stream

    def call(name):
        s = state[name]
        tail = (s["W"].data_ptr(), s["b"].data_ptr(), s["mW"].data_ptr(), s["vW"].data_ptr(), s["mb"].data_ptr(), s["vb"].data_ptr(),
                2e-4, 0.9, 0.999, 2e-8, bc1, bc2s, s["ws"].data_ptr(), s["loss"].data_ptr(), s["acc"].data_ptr(), None, None, None, stream)
        if name == "wide":
            return lambda: lib.cpc_probe_train_step_d(x_ptr, ldx, y.data_ptr(), R, C, D, *tail)
        return lambda: lib.cpc_probe_train_step(x_ptr, ldx, y.data_ptr(), R, C, *tail)

    wide, tile = call("wide"), call("tile")
    assert wide() == 0 and tile() == 0
    torch.cuda.synchronize()
    same = all(torch.equal(state["wide"][k], state["tile"][k]) for k in ("W", "b", "loss", "acc"))
    r = rounds_of((("wide", wide), ("tile", tile)), iters, rounds)
    r["same_bits"] = same
    r["wide_faster"] = r["wide"]["max_ms"] < r["tile"]["min_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_probe_widths.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe_widths: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "S": S, "iters": args.iters, "rounds": args.rounds, "pairs": {}, "d256": {}}
    for kind, C in KINDS:
        for B in BATCHES:
            for D in WIDTHS:
                out["pairs"][f"{kind}_B{B}_D{D}"] = widths_pair(kind, C, B, D, dev, args.iters, args.rounds)
            out["d256"][f"{kind}_B{B}"] = d256_pair(kind, C, B, dev, args.iters, args.rounds)
    ops.check_device_errors(clear=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
