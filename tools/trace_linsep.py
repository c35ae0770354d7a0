"""Launch counts of the fused probe step for a kernel trace: N calls of ops.probe_train_step and N of ops.probe_eval on random
features (phone: B = 8, S = 128, 41 classes; speaker: 8 rows read through their stride, 251 classes), nothing else on the device.
usage: rocprofv3 --kernel-trace --stats -- python tools/trace_linsep.py [N]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc_audio_amd import ops, optim  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    c = torch.randn(8, 128, 256, device=dev)
    accum = torch.zeros(2, dtype=torch.float64, device=dev)
    for rows, C in ((c.reshape(-1, 256), 41), (c[:, -1, :], 251)):
        lin = torch.nn.Linear(256, C).to(dev)
        opt = optim.Adam(lin.parameters(), lr=2e-4, eps=2e-8)
        label = torch.randint(0, C, (rows.shape[0],), device=dev)
        out = (torch.empty(1, 1, device=dev), torch.empty(1, 1, device=dev, dtype=torch.float64))
        torch.cuda.synchronize()
        for _ in range(n):
            ops.probe_train_step(rows, label, lin.weight, lin.bias, opt, accum=accum, out=out)
        for _ in range(n):
            ops.probe_eval(rows, label, lin.weight, lin.bias, accum=accum, out=out)
        torch.cuda.synchronize()
    ops.check_device_errors()
    print(f"{2 * n} probe_train_step calls, {2 * n} probe_eval calls; running sums {accum.tolist()}")


if __name__ == "__main__":
    main()
