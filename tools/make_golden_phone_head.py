"""Fixture of the PER phone classifier's head and loss (the reference's cpc/eval/common_voices_eval.py, CTCphone_criterion) --
tests/golden/phone_head.npz + phone_head_meta.json.  Runs only where the reference is importable:

    python tools/make_golden_phone_head.py

One case at the width the HIP head is built for: dimEncoder 256, 6 phones, B = 3 utterances of S = 28 frames with ragged
feature and label sizes, seeded head weights, reduction 'sum', no LSTM / seqNorm / dropout.  Stored: the input, the head's
weight and bias, the reference's getPrediction, its loss (forward() with // 4 and the clamp to the prediction's length, as
tools/make_golden_per.py follows it) and the loss's gradients with respect to weight, bias and input.
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np          # noqa: E402
import torch                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_per import import_reference_cv_eval  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    cve = import_reference_cv_eval()
    torch.manual_seed(300)
    crit = cve.CTCphone_criterion(256, 6, False, reduction="sum").eval()
    g = torch.Generator().manual_seed(301)
    x = torch.randn(3, 28, 256, generator=g).requires_grad_(True)
    feature_size = torch.tensor([28, 22, 13])
    label = torch.randint(0, 6, (3, 5), generator=g)
    label_size = torch.tensor([5, 3, 2])
    pred = crit.getPrediction(x, feature_size)
    fs = feature_size // 4
    cut = pred[:, :int(fs.max())]
    fs = torch.clamp(fs, max=cut.size(1))
    loss = crit.lossCriterion(torch.nn.functional.log_softmax(cut, dim=2).permute(1, 0, 2),
                              label[:, :int(label_size.max())], fs, label_size)
    loss.backward()
    head = crit.PhoneCriterionClassifier
    arrays = {"x": x.detach().numpy(), "weight": head.weight.detach().numpy(), "bias": head.bias.detach().numpy(),
              "label": label.numpy(), "pred": pred.detach().numpy(), "dweight": head.weight.grad.numpy(),
              "dbias": head.bias.grad.numpy(), "dx": x.grad.numpy()}
    meta = {"dimEncoder": 256, "nPhones": 6, "reduction": "sum", "feature_size": feature_size.tolist(),
            "label_size": label_size.tolist(), "loss": float(loss.detach()), "torch": torch.__version__,
            "keys": list(crit.state_dict().keys())}
    np.savez_compressed(os.path.join(GOLDEN, "phone_head.npz"), **arrays)
    with open(os.path.join(GOLDEN, "phone_head_meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(f"loss {float(loss.detach())}, prediction {tuple(pred.shape)}, "
          f"{os.path.getsize(os.path.join(GOLDEN, 'phone_head.npz'))} bytes")


if __name__ == "__main__":
    main()
