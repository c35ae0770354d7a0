"""Time the frozen linear-separability step (cpc_audio_amd.linear_separability.train_step's loop body) at B = 8 and B = 64, S = 128:
the CPC model's forward under no_grad, then the probe -- phone (41 classes, B * S rows) or speaker (251 classes, B rows) -- in
three variants that alternate in one process:
  fused   ops.probe_train_step (csrc/probe.hip): classifier, loss, accuracy, gradients and Adam in one C call
  unfused the criterion's autograd Function (csrc/supervised.hip) + optim.Adam.step(): the path without the fused step
  torch   nn.Linear + F.cross_entropy + torch.optim.Adam, the formulation of tools/bench_supervised.py
Each variant is timed --reps times (device events around --iters steps after warm-up); the JSON line gives the median, the
minimum and the maximum of those repeats per variant, for the whole step ("step") and for the probe alone on precomputed features
("probe"), and the feature forward alone.  Not part of bench.py.
usage: python tools/bench_linsep.py [--iters N] [--reps N]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cpc_audio_amd import ops, optim  # noqa: E402
from cpc_audio_amd.criterion import PhoneCriterion, SpeakerCriterion  # noqa: E402
from cpc_audio_amd.train import build_model  # noqa: E402
import supervised_util as U  # noqa: E402


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


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    iters, reps = arg("--iters", 100), arg("--reps", 5)
    dev = torch.device("cuda:0")
    S = 128
    out = {"S": S, "iters": iters, "reps": reps, "phones": U.N_PHONES, "speakers": 251}
    for B in (8, 64):
        torch.manual_seed(0)
        model = build_model().to(dev).eval()
        for p in model.parameters():
            p.requires_grad = False
        wave = (0.1 * torch.randn(B, 1, 20480, device=dev)).clamp_(-1, 1)
        with torch.no_grad():
            fixed, _, _ = model(wave, None)
        for kind, C in (("phone", U.N_PHONES), ("speaker", 251)):
            label = U.frame_labels(C, B, S).to(dev) if kind == "phone" else torch.randint(0, C, (B,), device=dev)
            crits = [(PhoneCriterion(256, C, False) if kind == "phone" else SpeakerCriterion(256, C)).to(dev) for _ in range(2)]
            lins = [c.PhoneCriterionClassifier if kind == "phone" else c.linearSpeakerClassifier for c in crits]
            ref = torch.nn.Linear(256, C).to(dev)
            opts = [optim.Adam(c.parameters(), lr=2e-4, eps=2e-8) for c in crits]
            ropt = torch.optim.Adam(ref.parameters(), lr=2e-4, eps=2e-8)
            accum = torch.zeros(2, dtype=torch.float64, device=dev)
            bufs = (torch.empty(1, 1, device=dev), torch.empty(1, 1, device=dev, dtype=torch.float64))

            def rows(cf):
                return (cf.reshape(-1, 256), label.view(-1)) if kind == "phone" else (cf[:, -1, :], label)

            def fused(cf):
                x, y = rows(cf)
                ops.probe_train_step(x, y, lins[0].weight, lins[0].bias, opts[0], accum=accum, out=bufs)

            def unfused(cf):
                opts[1].zero_grad()
                loss, acc = crits[1](cf, cf, label)
                loss.sum().backward()
                opts[1].step()
                accum[0] += loss.detach().mean().double()
                accum[1] += acc.detach().mean().double()

            def torch_form(cf):
                ropt.zero_grad()
                x, y = rows(cf)
                pred = ref(x)
                loss = F.cross_entropy(pred, y)
                acc = (pred.max(1)[1] == y).double().mean()
                loss.backward()
                ropt.step()
                accum[0] += loss.detach().double()
                accum[1] += acc

            def whole(probe):
                def step():
                    with torch.no_grad():
                        cf, _, _ = model(wave, None)
                    probe(cf.detach())
                return step

            variants = (("fused", fused), ("unfused", unfused), ("torch", torch_form))
            times = {f"{scope}_{name}": [] for scope in ("step", "probe") for name, _ in variants}
            feats = []
            for _ in range(reps):                       # the variants alternate: drift of the machine hits them alike
                with torch.no_grad():
                    feats.append(timeit(lambda: model(wave, None), iters))
                for name, fn in variants:
                    times[f"step_{name}"].append(timeit(whole(fn), iters))
                    times[f"probe_{name}"].append(timeit(lambda: fn(fixed), iters))
            key = f"B{B}_{kind}"
            out[f"{key}_features_ms"] = round(statistics.median(feats), 4)
            for k, v in times.items():
                out[f"{key}_{k}_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    ops.check_device_errors(clear=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
