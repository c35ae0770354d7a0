"""Time the PER phone classifier and the phone posteriors at feature widths other than 256 -> profiles/bench_head_widths.json.

D in {13, 40, 64, 512}, on precomputed features, at the shapes of tools/bench_phone_head.py and tools/bench_posterior.py:
  per_step    one step of CTCphone_criterion(D, 40, reduction="mean", wideKernel=True) -- head, log-softmax and CTC, forward and
              backward -- on B = 8 utterances of S = 1000 frames with 60 labels each, frozen features: hipHead=True against the
              module's own torch path (hipHead=False, the same parameters)
  posterior   one ops.posterior(..., wide=True) call against torch.softmax(F.linear(...)) on R in {400, 6400, 102400} rows and
              C in {42, 251} classes
Both variants of a pair alternate in one process, each timed by device events around --iters calls after warm-up, --rounds
times.  Per pair: median, fastest and slowest round of either side; ``won`` only where the HIP path's slowest round beats the
torch path's fastest, ``lost`` only where its fastest is slower than torch's slowest.  Before the timing both sides' results on
the same state are compared.
And, at D = 256, the _d entry points against the 256 entry points through the C ABI (head forward + backward, seqNorm forward +
backward, posteriors): the same bits, and which is faster.  Not part of bench.py.
usage: python tools/bench_head_widths.py [--iters N] [--rounds N] [--out PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc_audio_amd import _lib, common_voices_eval as CV, ops  # noqa: E402

WIDTHS = (13, 40, 64, 512)
B, S, PHONES, LABELS = 8, 1000, 40, 60
POSTERIOR_SHAPES = [(R, C) for R in (400, 6400, 102400) for C in (42, 251)]


def timeit(fn, iters, warm=3):
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
    for _ in range(rounds):                               # the variants alternate: drift of the machine hits them alike
        for name, fn in variants:
            times[name].append(timeit(fn, iters))
    return {name: summary(ts) for name, ts in times.items()}


def verdict(r, ours, theirs):
    r["won"] = r[ours]["max_ms"] < r[theirs]["min_ms"]
    r["lost"] = r[ours]["min_ms"] > r[theirs]["max_ms"]
    r[f"ratio_{theirs}_over_{ours}"] = round(r[theirs]["median_ms"] / r[ours]["median_ms"], 3)
    return r


def per_step_pair(D, dev, iters, rounds):
    torch.manual_seed(D)
    crits = {"hip": CV.CTCphone_criterion(D, PHONES, reduction="mean", hipHead=True, wideKernel=True).to(dev),
             "torch": CV.CTCphone_criterion(D, PHONES, reduction="mean", hipHead=False).to(dev)}
    crits["torch"].load_state_dict(crits["hip"].state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, D, generator=g).to(dev)
    sizes = torch.full((B,), S, dtype=torch.long, device=dev)
    phones = torch.randint(0, PHONES, (B, LABELS), generator=g).to(dev)
    size_phones = torch.full((B,), LABELS, dtype=torch.long, device=dev)
    last = {}

    def step(name):
        crit = crits[name]

        def fn():
            for p in crit.parameters():
                p.grad = None
            loss = crit(x, sizes, phones, size_phones)
            loss.mean().backward()
            last[name] = loss.detach()
        return fn

    fns = {k: step(k) for k in crits}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert {k: c.last_path for k, c in crits.items()} == {"hip": "hip", "torch": "torch"}
    gh, gt = (crits[k].PhoneCriterionClassifier.weight.grad for k in ("hip", "torch"))
    r = rounds_of(tuple(fns.items()), iters, rounds)
    r["loss_rel_diff"] = abs(float(last["hip"]) - float(last["torch"])) / abs(float(last["torch"]))
    r["dW_rel_diff"] = float((gh - gt).norm() / gt.norm())
    return verdict(r, "hip", "torch")


def posterior_pair(D, R, C, dev, iters, rounds):
    g = torch.Generator().manual_seed(R + C + D)
    x = torch.randn(R, D, generator=g).to(dev)
    W = ((2 * torch.rand(C, D, generator=g) - 1) / D ** 0.5).to(dev)
    b = ((2 * torch.rand(C, generator=g) - 1) / 16).to(dev)
    fns = {"hip": lambda: ops.posterior(x, W, b, wide=True), "torch": lambda: torch.softmax(F.linear(x, W, b), dim=1)}
    with torch.no_grad():
        diff = (fns["hip"]() - fns["torch"]()).abs().max().item()
        n = max(10, min(iters * 10, (iters * 10 * 6400) // R))               # (the largest shape: fewer calls per window)
        r = rounds_of(tuple(fns.items()), n, rounds)
    r["iters"], r["softmax_max_abs_diff"] = n, diff
    return verdict(r, "hip", "torch")


def d256_pairs(dev, iters, rounds):
    """The _d entry points at D = 256 against the 256 entry points, through the C ABI on buffers of the same shapes."""
    lib, D, C = _lib.get(), 256, PHONES + 1
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(256)
    x = torch.randn(B, S, D, generator=g).to(dev)
    W, bias = (0.05 * torch.randn(C, D, 8, generator=g)).to(dev), torch.zeros(C, device=dev)
    sizes = (ctypes.c_long * 5)()
    lib.check(lib.cpc_phone_head_layout_d(B, S, C, 0, D, sizes), "phone_head_layout_d")
    T = sizes[0]
    dl = torch.randn(B, T, C, generator=g).to(dev)
    dy = torch.randn(B, S, D, generator=g).to(dev)
    lens = torch.full((B,), S - 7, dtype=torch.long, device=dev)
    R, Cp = 6400, 42
    xp, Wp, bp = torch.randn(R, D, generator=g).to(dev), ((2 * torch.rand(Cp, D, generator=g) - 1) / 16).to(dev), torch.zeros(Cp, device=dev)
    out = {}
    bufs = {n: dict(wr=torch.empty(sizes[1], device=dev), scr=torch.empty(sizes[2], device=dev), lg=torch.empty(sizes[3], device=dev),
                    dW=torch.empty(C, D, 8, device=dev), db=torch.empty(C, device=dev), dX=torch.empty(B, S, D, device=dev),
                    y=torch.empty(B, S, D, device=dev), st=torch.empty(B, 2, D, device=dev), dx=torch.empty(B, S, D, device=dev),
                    post=torch.empty(R, Cp, device=dev)) for n in ("wide", "fixed")}
    P = lambda t: t.data_ptr()    # noqa: E731

    def head(n):
        s, t = bufs[n], ((D,) if n == "wide" else ())
        fwd = lib.cpc_phone_head_forward_d if n == "wide" else lib.cpc_phone_head_forward
        bwd = lib.cpc_phone_head_backward_d if n == "wide" else lib.cpc_phone_head_backward

        def fn():
            assert fwd(P(x), P(W), P(bias), P(s["wr"]), P(s["scr"]), P(s["lg"]), B, S, C, *t, stream) == 0
            assert bwd(P(x), P(s["wr"]), P(dl), P(s["scr"]), P(s["dW"]), P(s["db"]), P(s["dX"]), B, S, C, *t, stream) == 0
        return fn

    def seqnorm(n):
        s, t = bufs[n], ((D,) if n == "wide" else ())
        fwd = lib.cpc_seqnorm_forward_d if n == "wide" else lib.cpc_seqnorm_forward
        bwd = lib.cpc_seqnorm_backward_d if n == "wide" else lib.cpc_seqnorm_backward

        def fn():
            assert fwd(P(x), P(lens), None, P(s["y"]), P(s["st"]), B, S, *t, 1, stream) == 0
            assert bwd(P(x), P(dy), P(lens), None, P(s["st"]), P(s["dx"]), B, S, *t, 1, stream) == 0
        return fn

    def posterior(n):
        s, t = bufs[n], ((D,) if n == "wide" else ())
        fwd = lib.cpc_posterior_forward_d if n == "wide" else lib.cpc_posterior_forward
        return lambda: fwd(P(xp), D, P(Wp), P(bp), R, Cp, *t, 0, P(s["post"]), None, stream)

    for what, make, keys, k in (("head", head, ("lg", "dW", "db", "dX"), 1), ("seqnorm", seqnorm, ("y", "st", "dx"), 5),
                                ("posterior", posterior, ("post",), 10)):
        fns = {n: make(n) for n in ("wide", "fixed")}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        r = rounds_of(tuple(fns.items()), iters * k, rounds)
        r["same_bits"] = all(torch.equal(bufs["wide"][key], bufs["fixed"][key]) for key in keys)
        r["wide_slower"] = r["wide"]["min_ms"] > r["fixed"]["max_ms"]
        r["wide_faster"] = r["wide"]["max_ms"] < r["fixed"]["min_ms"]
        out[what] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_head_widths.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_widths: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "B": B, "S": S, "classes": PHONES + 1, "labels": LABELS, "iters": args.iters,
           "rounds": args.rounds, "per_step": {}, "posterior": {}}
    for D in WIDTHS:
        out["per_step"][f"D{D}"] = per_step_pair(D, dev, args.iters, args.rounds)
        for R, C in POSTERIOR_SHAPES:
            out["posterior"][f"D{D}_R{R}_C{C}"] = posterior_pair(D, R, C, dev, args.iters, args.rounds)
    out["d256"] = d256_pairs(dev, args.iters, args.rounds)
    ops.check_device_errors(clear=True)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
