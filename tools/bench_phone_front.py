"""One training step of the PER phone classifier on the GPU, HIP front against torch front: one JSON line per run.

CTCphone_criterion(256, 40, hipHead=True) on B = 8 utterances of S = 1000 frames with ragged sizes, 41 classes, targets of 60
labels: forward + backward of `criterion(c_feature, sizes, phones, sizePhones).mean()`, as common_voices_eval.train_step runs
it.  hipFront=True runs seqNorm and the dropout on csrc/seqnorm.hip and the LSTM on csrc/lstm.hip; hipFront=False is the
module's torch front (the per-utterance seqNorm loop with its int() round trips, nn.LSTM, nn.Dropout2d) -- the code path of
the commit before the HIP front, unchanged.  Both modules hold the same weights and are timed in one process, alternating,
after a warm-up of every shape: device events around each step, median of --reps (>= 5).  Variants: --seqNorm alone, --LSTM
alone, all three flags, each with frozen features and with features that require a gradient.  Kernel resources come from
tools/kernel_resources.py.

    python tools/bench_phone_front.py [--reps 9] [--out profiles/phone_front_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_phone_head import timed_pair                     # noqa: E402
from cpc_audio_amd import common_voices_eval as CV, ops    # noqa: E402

VARIANTS = {"seqNorm": dict(LSTM=False, seqNorm=True, dropout=False),
            "LSTM": dict(LSTM=True, seqNorm=False, dropout=False),
            "LSTM+seqNorm+dropout": dict(LSTM=True, seqNorm=True, dropout=True)}


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                        os.path.join(ROOT, "cpc_audio_amd", "csrc", "seqnorm.hip")], capture_output=True, text=True)
    return [re.sub(r"\s+", " ", line.strip()) for line in r.stdout.splitlines() if "kernel" in line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--S", type=int, default=1000)
    ap.add_argument("--phones", type=int, default=40)
    ap.add_argument("--labels", type=int, default=60)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    B, S, n_phones, L = args.B, args.S, args.phones, args.labels
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B, S, 256, generator=g) + 2.0 * torch.randn(256, generator=g)).cuda()
    x_grad = x.clone().requires_grad_(True)
    sizes = torch.linspace(S, (3 * S) // 5, B).long().cuda()           # ragged: the longest fills the batch, the shortest 60 %
    phones = torch.randint(0, n_phones, (B, L), generator=g).cuda()
    size_phones = torch.full((B,), L, dtype=torch.long, device="cuda")
    result = {"bench": "phone_front_step", "device": torch.cuda.get_device_name(0), "B": B, "S": S, "sizes": sizes.tolist(),
              "classes": n_phones + 1, "labels": L, "reps": args.reps, "head": "hip", "variants": {}}
    for name, flags in VARIANTS.items():
        torch.manual_seed(0)
        crits = {"hip": CV.CTCphone_criterion(256, n_phones, reduction="mean", hipHead=True, hipFront=True, **flags).cuda(),
                 "torch": CV.CTCphone_criterion(256, n_phones, reduction="mean", hipHead=True, hipFront=False, **flags).cuda()}
        crits["torch"].load_state_dict(crits["hip"].state_dict())
        last = {}

        def step(key, feats):
            crit = crits[key]

            def fn():
                for p in crit.parameters():
                    p.grad = None
                feats.grad = None
                loss = crit(feats, sizes, phones, size_phones)
                loss.mean().backward()
                last[key] = loss.detach()
            return fn

        frozen, frozen_all = timed_pair({k: step(k, x) for k in crits}, args.reps)
        fronts = {k: c.last_front for k, c in crits.items()}
        assert fronts == {"hip": "hip", "torch": "torch"}, fronts
        with_dx, with_dx_all = timed_pair({k: step(k, x_grad) for k in crits}, args.reps)
        ops.check_device_errors()
        entry = {"step_frozen_ms": frozen, "step_with_dx_ms": with_dx, "step_frozen_all_ms": frozen_all,
                 "step_with_dx_all_ms": with_dx_all, "torch_over_hip_frozen": round(frozen["torch"] / frozen["hip"], 3),
                 "torch_over_hip_with_dx": round(with_dx["torch"] / with_dx["hip"], 3)}
        if not flags["dropout"]:                  # the two fronts compute the same step (with dropout their masks differ)
            crits["hip"].zero_grad(), crits["torch"].zero_grad()
            step("hip", x)(), step("torch", x)()
            wh, wt = (crits[k].PhoneCriterionClassifier.weight.grad for k in ("hip", "torch"))
            entry["agreement"] = {"loss_hip": float(last["hip"]), "loss_torch": float(last["torch"]),
                                  "dW_rel_diff": float((wh - wt).norm() / wt.norm())}
        result["variants"][name] = entry
    result["resources"] = resources()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
