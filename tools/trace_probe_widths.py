"""20 fused probe steps (phone, B = 64: 8192 rows of D features, 41 classes) at one feature width, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/trace_probe_widths.py D

profiles/probe_widths_kernel_stats.csv holds the probe kernels' rows of such runs at D = 13, 40, 64 and 512."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc_audio_amd import ops, optim  # noqa: E402
from cpc_audio_amd.criterion import PhoneCriterion  # noqa: E402


def main():
    D = int(sys.argv[1])
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(64 * 128, D, device=dev)
    y = torch.randint(0, 41, (64 * 128,), device=dev)
    crit = PhoneCriterion(D, 41, False, wideKernel=True).to(dev)
    lin = crit.PhoneCriterionClassifier
    opt = optim.Adam(crit.parameters(), lr=2e-4, eps=2e-8)
    for _ in range(20):
        ops.probe_train_step(x, y, lin.weight, lin.bias, opt)
    torch.cuda.synchronize()
    ops.check_device_errors()


if __name__ == "__main__":
    main()
