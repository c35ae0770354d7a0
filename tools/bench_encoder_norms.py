"""Time the conv encoder under normMode batchNorm / instanceNorm / ID on an MI355X: the HIP path (csrc/enc_wide.hip:
cpc_encoder_*_n through ops.EncoderNormFunction) against the same module's torch path (five nn.Conv1d on MIOpen + nn.BatchNorm1d /
nn.InstanceNorm1d / nothing + ReLU), same GPU, same commit, same process.

    python tools/bench_encoder_norms.py [--rounds 9] [--iters 3] [--out profiles/bench_encoder_norms.json]

model.CPCEncoder(C, mode, encoderKernel=True) forward + backward in training mode at B = 64, L = 20480 with gradients to every
parameter, the three modes at C = 256 and C = 512, and batchNorm's eval-mode forward (no_grad) at C = 256, each against a copy of
the module without the keyword carrying the same weights and buffers.
Protocol of tools/bench_encoder_widths.py: the two paths alternate round by round after a warm-up, a round times ``iters`` calls
between two device events; per path the median, the fastest and the slowest of the rounds; ``won`` = the HIP path's slowest round
beats the other's fastest, ``lost`` = its fastest is slower than the other's slowest, otherwise undecided."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_ar_widths import alternate  # noqa: E402
from cpc_audio_amd import ops  # noqa: E402
from cpc_audio_amd.model import CPCEncoder  # noqa: E402

PAIRS = [(mode, C, "fwdbwd") for C in (256, 512) for mode in ("batchNorm", "instanceNorm", "ID")] + [("batchNorm", 256, "eval_fwd")]
B, L = 64, 20480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_norms: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    out = {"bench": "encoder_norms", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "B": B, "L": L}
    g = torch.Generator().manual_seed(0)
    wave = (0.1 * torch.randn(B, 1, L, generator=g)).clamp_(-1, 1).to(dev)
    for mode, C, what in PAIRS:
        torch.manual_seed(1)
        hip_enc = CPCEncoder(C, mode, encoderKernel=True).to(dev)
        torch_enc = copy.deepcopy(hip_enc)
        torch_enc.hip_norm = False
        assert hip_enc.hip_norm and not (hip_enc.hip or hip_enc.hip_wide or torch_enc.hip)
        dz = torch.randn(B, C, L // 160, generator=g).to(dev)
        last = {}
        if what == "eval_fwd":
            hip_enc.eval()
            torch_enc.eval()

            def run(enc, key):
                with torch.no_grad():
                    last[key] = enc(wave)
        else:
            def run(enc, key):
                enc.zero_grad(set_to_none=True)
                z = enc(wave)
                z.backward(dz)
                last[key] = z.detach()

        r = alternate([("hip", lambda: run(hip_enc, "hip")), ("torch", lambda: run(torch_enc, "torch"))], args.rounds, args.iters)
        r["ratio_torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
        r["won"] = r["hip"]["max_ms"] < r["torch"]["min_ms"]
        r["lost"] = r["hip"]["min_ms"] > r["torch"]["max_ms"]
        r["z_max_abs_diff"] = (last["hip"] - last["torch"]).abs().max().item()
        if what == "fwdbwd":
            # (conv biases before a mean-removing norm have an analytically zero gradient: noise on both sides, left out)
            pairs = [(p, q) for (n, p), (_, q) in zip(hip_enc.named_parameters(), torch_enc.named_parameters())
                     if mode == "ID" or not (n.startswith("conv") and n.endswith("bias"))]
            r["grad_max_rel_diff"] = max(((p.grad - q.grad).norm() / q.grad.norm()).item() for p, q in pairs)
        out[f"{mode}_C{C}_{what}"] = r
        del hip_enc, torch_enc, dz, last
        torch.cuda.empty_cache()
    ops.check_device_errors(clear=True)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
