"""Time the LSTM at a hidden width other than 256 on an MI355X: the HIP path (csrc/lstm.hip: cpc_lstm_*_h through
ops.LstmHiddenFunction) against the same module on torch.nn.LSTM (MIOpen), same GPU, same commit, same process.

    python tools/bench_lstm_hidden.py [--rounds 9] [--iters 3] [--out profiles/bench_lstm_hidden.json]

``cpcar``: model.CPCAR(D, H, 1 layer, mode LSTM, lstmKernel, hiddenKernel) forward + backward at B = 64, S = 128 with gradients
to x and every parameter, (D, H) in {(256, 128), (256, 512), (512, 512), (40, 64)}, against the same CPCAR without hiddenKernel.
``per_front``: the LSTM step of the PER classifier's front -- nn.LSTM(D, D) of common_voices_eval.CTCphone_criterion on
(8, 1000, D) features, forward + backward -- at D in {13, 40, 64, 512}: ops.LstmHiddenFunction on conv1's parameters (what
hipFront + wideKernel + hiddenKernel runs) against conv1 itself (what it runs without hiddenKernel).
Protocol of tools/bench_ar_widths.py: the two paths alternate round by round after a warm-up, a round times ``iters`` calls
between two device events; per path the median, the fastest and the slowest of the rounds; ``won`` = the HIP path's slowest
round beats the other's fastest.  ``paths`` names the recurrence kernels the HIP side launched (persistent / per_step)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_ar_widths import alternate  # noqa: E402
from cpc_audio_amd import common_voices_eval as CV  # noqa: E402
from cpc_audio_amd import ops  # noqa: E402
from cpc_audio_amd.model import CPCAR  # noqa: E402

CPCAR_CASES = [(256, 128), (256, 512), (512, 512), (40, 64)]
FRONT_WIDTHS = [13, 40, 64, 512]


def pair(hip_fn, torch_fn, x, dy, rounds, iters):
    last = {}

    def run(fn, key):
        x.grad = None
        y = fn(x)
        y.backward(dy)
        last[key] = y.detach()

    ops.lstm_hidden_paths(clear=True)
    r = alternate([("hip", lambda: run(hip_fn, "hip")), ("torch", lambda: run(torch_fn, "torch"))], rounds, iters)
    r["paths"] = sorted(ops.lstm_hidden_paths(clear=True))
    r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
    r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
    r["lost"] = r["hip"]["min_ms"] > r["torch"]["max_ms"]
    r["y_max_abs_diff"] = (last["hip"] - last["torch"]).abs().max().item()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm_hidden: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    out = {"bench": "lstm_hidden_fwdbwd", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "cpcar": {"B": 64, "S": 128}, "per_front": {"B": 8, "S": 1000}}
    g = torch.Generator().manual_seed(0)
    for D, H in CPCAR_CASES:
        B, S = 64, 128
        torch.manual_seed(1)
        hip_ar = CPCAR(D, H, False, 1, mode="LSTM", lstmKernel=True, hiddenKernel=True).to(dev)
        torch_ar = CPCAR(D, H, False, 1, mode="LSTM", lstmKernel=True).to(dev)
        torch_ar.load_state_dict(hip_ar.state_dict())
        assert hip_ar.hip_hidden and not (torch_ar.hip_hidden or torch_ar.hip_lstm or torch_ar.hip_in)
        x = torch.randn(B, S, D, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(B, S, H, generator=g).to(dev)

        def call(ar):
            def fn(t):
                ar.zero_grad(set_to_none=True)
                return ar(t)
            return fn

        out["cpcar"][f"D{D}_H{H}"] = pair(call(hip_ar), call(torch_ar), x, dy, args.rounds, args.iters)
        del hip_ar, torch_ar, x, dy
        torch.cuda.empty_cache()
    for D in FRONT_WIDTHS:
        B, S = 8, 1000
        torch.manual_seed(2)
        crit = CV.CTCphone_criterion(D, 41, LSTM=True, hipFront=True, wideKernel=True, hiddenKernel=True).to(dev)
        lstm = crit.conv1
        x = torch.randn(B, S, D, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(B, S, D, generator=g).to(dev)

        def hip_fn(t):
            lstm.zero_grad(set_to_none=True)
            return ops.LstmHiddenFunction.apply(t, None, False, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0,
                                                lstm.bias_hh_l0)[0]

        def torch_fn(t):
            lstm.zero_grad(set_to_none=True)
            return lstm(t)[0]

        out["per_front"][f"D{D}"] = pair(hip_fn, torch_fn, x, dy, args.rounds, args.iters)
        del crit, lstm, x, dy
        torch.cuda.empty_cache()
    ops.check_device_errors(clear=True)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
