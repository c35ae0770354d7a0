"""Fixture of the PER phone classifier with its front (the reference's cpc/eval/common_voices_eval.py, CTCphone_criterion with
seqNorm, without and with the LSTM) -- tests/golden/phone_front.npz + phone_front_meta.json.  Runs only where the reference is
importable:

    python tools/make_golden_phone_front.py

CTCphone_criterion(256, 6, LSTM, seqNorm=True, reduction='sum') in eval(), LSTM off and on, B = 3 utterances of S = 28 frames
with ragged sizes [28, 22, 13].  The parameters are oracle.make_golden_predictors.seeded_state(shapes, seed) over the state
dict's keys, the seed stored in the meta file.  Stored: the input, both predictions, the losses (formed as
tools/make_golden_phone_head.py forms them: the reference's forward divides an integer tensor in place), the head's gradients,
and of the LSTM's four gradients the [::16, ::16] sub-grid with each tensor's norm and sum (the full tensors are 2 MB).

The reference's getPrediction writes its seqNorm into its input, so it gets a clone of features that do not require a
gradient; it cannot backpropagate through that in-place write, so the fixture holds no gradient of the input.
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
from oracle.make_golden_predictors import seeded_state  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 410
LSTM_KEYS = ("conv1.weight_ih_l0", "conv1.weight_hh_l0", "conv1.bias_ih_l0", "conv1.bias_hh_l0")


def subgrid(t):
    return t[::16, ::16] if t.dim() == 2 else t[::16]


def main():
    cve = import_reference_cv_eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(3, 28, 256, generator=g) + 0.5 * torch.randn(256, generator=g)
    feature_size = torch.tensor([28, 22, 13])
    label = torch.randint(0, 6, (3, 5), generator=g)
    label_size = torch.tensor([5, 3, 2])
    arrays = {"x": x.numpy().copy(), "label": label.numpy()}
    meta = {"dimEncoder": 256, "nPhones": 6, "reduction": "sum", "seqNorm": True, "seed": SEED,
            "feature_size": feature_size.tolist(), "label_size": label_size.tolist(), "torch": torch.__version__, "loss": {},
            "lstm_grad_norm": {}, "lstm_grad_sum": {}}
    for lstm in (False, True):
        tag = "lstm" if lstm else "plain"
        crit = cve.CTCphone_criterion(256, 6, lstm, seqNorm=True, reduction="sum").eval()
        crit.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in crit.state_dict().items()}, SEED))
        meta["keys"] = list(crit.state_dict().keys())
        pred = crit.getPrediction(x.clone(), feature_size)
        fs = feature_size // 4
        cut = pred[:, :int(fs.max())]
        fs = torch.clamp(fs, max=cut.size(1))
        loss = crit.lossCriterion(torch.nn.functional.log_softmax(cut, dim=2).permute(1, 0, 2),
                                  label[:, :int(label_size.max())], fs, label_size)
        loss.backward()
        head = crit.PhoneCriterionClassifier
        arrays.update({f"pred_{tag}": pred.detach().numpy(), f"dweight_{tag}": head.weight.grad.numpy(),
                       f"dbias_{tag}": head.bias.grad.numpy()})
        meta["loss"][tag] = float(loss.detach())
        if lstm:
            for k in LSTM_KEYS:
                grad = dict(crit.named_parameters())[k].grad
                arrays["d" + k] = subgrid(grad).contiguous().numpy()
                meta["lstm_grad_norm"][k] = float(grad.double().norm())
                meta["lstm_grad_sum"][k] = float(grad.double().sum())
    path = os.path.join(GOLDEN, "phone_front.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(GOLDEN, "phone_front_meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(f"losses {meta['loss']}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
