"""Time the supervised criteria (csrc/supervised.hip through SpeakerCriterion / PhoneCriterion / CTCPhoneCriterion) against
the reference's torch formulation (nn.Linear + nn.CrossEntropyLoss, and for CTC log_softmax + nn.CTCLoss on labels collapsed by
the reference's per-sequence loop, cpc/criterion/seq_alignment.py:64-86) on the same GPU, at B = 8 and B = 64, S = 128: forward +
backward ms per call (device events around --iters calls after warm-up).  Also the frozen linear-separability step end to end
(the CPC model's forward under no_grad, the phone criterion, Adam on the classifier).  Prints one JSON line.  Not part of bench.py.
usage: python tools/bench_supervised.py [--iters N]"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cpc_audio_amd.criterion import CTCPhoneCriterion, PhoneCriterion, SpeakerCriterion  # noqa: E402
from cpc_audio_amd.ops import check_device_errors  # noqa: E402
import supervised_util as U  # noqa: E402


def timeit(fn, iters, warm=20):
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


def collapse_reference(labels):
    """The reference's collapseLabelChain: a loop over the batch and a host read of the longest chain."""
    N, T = labels.size()
    sizes = torch.zeros(N, device=labels.device, dtype=torch.int64)
    out = []
    for i in range(N):
        status = torch.cat([torch.ones(1, device=labels.device, dtype=labels.dtype), labels[i, :-1] - labels[i, 1:]])
        sizes[i] = (status != 0).sum()
        out.append(labels[i][status != 0])
    padded = torch.zeros(N, int(sizes.max().item()), device=labels.device, dtype=torch.int64)
    for i in range(N):
        padded[i, :int(sizes[i])] = out[i]
    return padded, sizes


def torch_step(kind, lin, c, label):
    """The reference's forward (criterion.py:194-203, 218-231, 265-283) and backward on torch ops."""
    B, S, _ = c.shape
    if kind == "speaker":
        loss = F.cross_entropy(lin(c[:, -1, :]), label)
    elif kind == "phone":
        pred = lin(c.reshape(B * S, -1))
        loss = F.cross_entropy(pred, label.view(-1))
        (pred.max(1)[1] == label.view(-1)).double().mean()
    else:
        lp = F.log_softmax(lin(c.reshape(B * S, -1)).view(B, S, -1), dim=2).permute(1, 0, 2)
        tgt, sizes = collapse_reference(label)
        loss = F.ctc_loss(lp, tgt, torch.full((B,), S, dtype=torch.int64, device=c.device), sizes, blank=lin.out_features - 1,
                          zero_infinity=True)
    loss.backward()


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 200
    dev = torch.device("cuda:0")
    S = 128
    out = {"S": S, "iters": iters, "phones": U.N_PHONES, "speakers": 251}
    for B in (8, 64):
        torch.manual_seed(0)
        c = torch.randn(B, S, 256, device=dev, requires_grad=True)
        ph = U.frame_labels(U.N_PHONES, B, S).to(dev)
        spk = torch.randint(0, 251, (B,), device=dev)
        for kind, crit in (("speaker", SpeakerCriterion(256, 251)), ("phone", PhoneCriterion(256, U.N_PHONES, False)),
                           ("ctc", CTCPhoneCriterion(256, U.N_PHONES, False))):
            crit = crit.to(dev)
            lin = crit.linearSpeakerClassifier if kind == "speaker" else crit.PhoneCriterionClassifier
            label = spk if kind == "speaker" else ph

            def hip():
                loss, _ = crit(c, c, label)
                torch.autograd.backward([loss], [torch.ones_like(loss)])

            out[f"B{B}_{kind}_fwdbwd_ms_hip"] = round(timeit(hip, iters), 4)
            out[f"B{B}_{kind}_fwdbwd_ms_torch"] = round(timeit(lambda: torch_step(kind, lin, c, label), iters), 4)

    # frozen linear separability, one step: features under no_grad, the phone criterion, Adam on the classifier
    from cpc_audio_amd.train import build_model
    for B in (8, 64):
        torch.manual_seed(0)
        model = build_model().to(dev)
        for p in model.parameters():
            p.requires_grad = False
        wave = (0.1 * torch.randn(B, 1, 20480, device=dev)).clamp_(-1, 1)
        label = U.frame_labels(U.N_PHONES, B, S).to(dev)
        crit = PhoneCriterion(256, U.N_PHONES, False).to(dev)
        ref = torch.nn.Linear(256, U.N_PHONES).to(dev)
        opt, ropt = torch.optim.Adam(crit.parameters(), lr=2e-4), torch.optim.Adam(ref.parameters(), lr=2e-4)

        def step_hip():
            with torch.no_grad():
                cf, enc, _ = model(wave, label)
            loss, _ = crit(cf, enc, label)
            torch.autograd.backward([loss], [torch.ones_like(loss)])
            opt.step()
            opt.zero_grad()

        def step_torch():
            with torch.no_grad():
                cf, _, _ = model(wave, label)
            F.cross_entropy(ref(cf.reshape(-1, 256)), label.view(-1)).backward()
            ropt.step()
            ropt.zero_grad()

        with torch.no_grad():
            out[f"B{B}_features_ms"] = round(timeit(lambda: model(wave, label), iters // 4), 4)
        out[f"B{B}_separability_step_ms_hip"] = round(timeit(step_hip, iters // 4), 4)
        out[f"B{B}_separability_step_ms_torch"] = round(timeit(step_torch, iters // 4), 4)
    check_device_errors(clear=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
