"""Time ops.posterior (csrc/posterior.hip) against the torch ops it replaces, on the same device and shapes:
  softmax   F.linear + softmax                     vs  ops.posterior(x, W, b)
  one_hot   F.linear + argmax + harness.toOneHot   vs  ops.posterior(x, W, b, one_hot=True)
at R in {400, 6400, 102400} rows of 256 features (400 rows: one 64000-sample chunk) and C in {42, 251} classes.  The variants
alternate in one process; each is timed --reps times (device events around --iters calls after warm-up) and every JSON line
gives the median, the minimum and the maximum of those repeats, after the outputs of the two variants have been compared at that
shape.  Then one end-to-end export of a synthetic directory (build_zeroSpeech_features.main, --files files of 64000 + 12345
samples, a seeded two-layer GRU with a CTC phone classifier of 42 classes) per format and head, by the host clock around the
whole command.  Not part of bench.py.
usage: python tools/bench_posterior.py [--iters N] [--reps N] [--files N]"""
import json
import os
import statistics
import sys
import tempfile
import time
import wave

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc_audio_amd import build_zeroSpeech_features as Z, harness, ops  # noqa: E402
from cpc_audio_amd.criterion import CTCPhoneCriterion  # noqa: E402
from cpc_audio_amd.train import build_model  # noqa: E402


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


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def calls(iters, reps, dev):
    for R in (400, 6400, 102400):
        for C in (42, 251):
            g = torch.Generator().manual_seed(R + C)
            x = torch.randn(R, 256, generator=g).to(dev)
            W = ((2 * torch.rand(C, 256, generator=g) - 1) / 16).to(dev)
            b = ((2 * torch.rand(C, generator=g) - 1) / 16).to(dev)
            variants = {
                "softmax_hip": lambda: ops.posterior(x, W, b),
                "softmax_torch": lambda: torch.softmax(F.linear(x, W, b), dim=1),
                "one_hot_hip": lambda: ops.posterior(x, W, b, one_hot=True),
                "one_hot_torch": lambda: harness.toOneHot(F.linear(x, W, b).view(1, R, C).argmax(dim=2), C),
            }
            with torch.no_grad():
                diff = (variants["softmax_hip"]() - variants["softmax_torch"]()).abs().max().item()
                rows = int((variants["one_hot_hip"]() != variants["one_hot_torch"]().view(R, C)).any(dim=1).sum())
                n = max(10, min(iters, (iters * 6400) // R))          # (the largest shape: fewer calls per window)
                times = {k: [] for k in variants}
                for _ in range(reps):                                  # the variants alternate: drift hits them alike
                    for k, fn in variants.items():
                        times[k].append(timeit(fn, n))
            line = {"bench": "posterior_call", "R": R, "C": C, "iters": n, "reps": reps, "softmax_max_abs_diff": diff,
                    "one_hot_rows_that_differ": rows}
            line.update({f"{k}_ms": spread(v) for k, v in times.items()})
            print(json.dumps(line), flush=True)


def export(n_files, dev):
    with tempfile.TemporaryDirectory() as td:
        db, ckpt = os.path.join(td, "db"), os.path.join(td, "ckpt")
        os.makedirs(db)
        os.makedirs(ckpt)
        g = torch.Generator().manual_seed(1)
        for k in range(n_files):
            pcm = ((0.1 * torch.randn(64000 + 12345, generator=g)).clamp_(-1, 1) * 32767).round().to(torch.int16).numpy()
            with wave.open(os.path.join(db, f"utt{k:04d}.wav"), "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(16000)
                f.writeframes(pcm.astype("<i2").tobytes())
        torch.manual_seed(2)
        with open(os.path.join(ckpt, "checkpoint_args.json"), "w") as f:
            json.dump({"arMode": "GRU", "nLevelsGRU": 2, "CTC": True}, f)
        path = os.path.join(ckpt, "checkpoint_0.pt")
        harness.save_checkpoint(build_model(arMode="GRU", nLevelsGRU=2).state_dict(), CTCPhoneCriterion(256, 41, False).state_dict(),
                                None, None, path)
        runs = [("features", fmt, []) for fmt in ("npy", "fea")]
        runs += [(f"posteriors_{head}", fmt, ["--addCriterion", f"--{head}"]) for fmt in ("npy", "fea") for head in ("hipHead", "no-hipHead")]
        for rep in range(2):                                           # (the first pass also loads code objects and libraries)
            for what, fmt, options in runs:
                out = os.path.join(td, f"out_{what}_{fmt}_{rep}")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                Z.main([db, out, path, "--format", fmt, *options])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(json.dumps({"bench": "export", "pass": rep, "what": what, "format": fmt, "files": n_files,
                                  "frames": n_files * ((64000 + 12345) // 160), "seconds": round(dt, 4),
                                  "ms_per_file": round(1000 * dt / n_files, 3)}), flush=True)


def main():
    assert torch.cuda.is_available(), "bench_posterior.py times the GPU: no device, no numbers"
    dev = torch.device("cuda:0")
    calls(arg("--iters", 2000), arg("--reps", 5), dev)
    export(arg("--files", 50), dev)
    ops.check_device_errors(clear=True)


if __name__ == "__main__":
    main()
