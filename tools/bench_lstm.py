"""Time the HIP LSTM (cpc_lstm_forward / _backward through ops.LstmFunction: persistent recurrence and one launch per step)
against torch.nn.LSTM (MIOpen) in the same process, at B = 64 / 256, S = 128, nl = 1 / 2.  Prints one JSON line (ms per call;
"fwd" = forward alone, "fwdbwd" = forward + backward).  Not part of bench.py.
--cell RNN times the Elman kernels instead (cpc_rnn_forward / _backward through ops.RnnFunction, batch-first, as
CPCAR(mode="RNN", rnnKernel=True) calls them) against torch.nn.RNN.
usage: python tools/bench_lstm.py [--iters N] [--cell LSTM|RNN]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpc_audio_amd.ops import LstmFunction, RnnFunction, check_device_errors  # noqa: E402


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


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    cell = sys.argv[sys.argv.index("--cell") + 1] if "--cell" in sys.argv else "LSTM"
    if cell not in ("LSTM", "RNN"):
        raise SystemExit("bench_lstm: --cell LSTM or RNN")
    name = "nn_lstm" if cell == "LSTM" else "nn_rnn"
    dev = torch.device("cuda:0")
    S = 128
    out = {"cell": cell, "S": S, "iters": iters}
    for B in (64, 256):
        for nl in (1, 2):
            torch.manual_seed(0)
            net = (torch.nn.LSTM if cell == "LSTM" else torch.nn.RNN)(256, 256, num_layers=nl, batch_first=True).to(dev)
            params = [p for p in net.parameters()]          # weight_ih, weight_hh, bias_ih, bias_hh per layer
            x = torch.randn(B, S, 256, device=dev, requires_grad=True)
            dy = torch.randn(B, S, 256, device=dev)

            def call(per_step):
                if cell == "LSTM":
                    return LstmFunction.apply(x, None, per_step, *params)[0]
                return RnnFunction.apply(x, None, False, per_step, *params)[0]

            def hip(per_step, backward):
                y = call(per_step)
                if backward:
                    y.backward(dy)

            def miopen(backward):
                y = net(x)[0]
                if backward:
                    y.backward(dy)

            key = f"B{B}_nl{nl}"
            with torch.no_grad():
                out[f"{key}_fwd_ms_hip"] = round(timeit(lambda: hip(False, False), iters), 4)
                out[f"{key}_fwd_ms_hip_per_step"] = round(timeit(lambda: hip(True, False), iters), 4)
                out[f"{key}_fwd_ms_{name}"] = round(timeit(lambda: miopen(False), iters), 4)
            out[f"{key}_fwdbwd_ms_hip"] = round(timeit(lambda: hip(False, True), iters), 4)
            out[f"{key}_fwdbwd_ms_hip_per_step"] = round(timeit(lambda: hip(True, True), iters), 4)
            out[f"{key}_fwdbwd_ms_{name}"] = round(timeit(lambda: miopen(True), iters), 4)
            with torch.no_grad():
                a = call(False)
                b = net(x)[0]
            out[f"{key}_max_abs_diff"] = float((a - b).abs().max().item())
    check_device_errors(clear=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
