"""Linear-separability evaluation (cpc/eval/linear_separability.py): a linear phone or speaker classifier trained on the
features of a CPC checkpoint -- the accuracy the CPC paper reports.

    python -m cpc_audio_amd.linear_separability pathDB pathTrain pathVal checkpoint.pt [--pathPhone labels.txt] [--CTC] ...

Functions, arguments, defaults and the files written (``<pathCheckpoint>/checkpoint_args.json``, ``checkpoint_<epoch>.pt`` with
``{"gEncoder", "cpcCriterion", "optimizer", "best"}``, ``checkpoint_logs.json``) are the reference's.  One process, one GPU, one
checkpoint: ``--nGPU n`` only scales the batch to ``batchSizeGPU * n`` (the reference's global batch); several checkpoints
(concatenated models) raise.

In the default frozen mode the step behind the feature forward -- classifier, cross-entropy, accuracy, both gradients and the
Adam update -- is ONE C call (``ops.probe_train_step``, csrc/probe.hip) when ``FUSED_PROBE`` is set, the criterion is a
SpeakerCriterion or PhoneCriterion on the HIP path (one layer; 256 features, or with ``--wideKernel`` any width from 1 to 512:
an MFCC, filter-bank, ``no_ar`` or ``hiddenGar 512`` checkpoint) and the features are CUDA fp32.  Everything else (``--CTC``,
``--unfrozen``, the flag off) runs the criterion's autograd Function and ``optim.Adam.step()`` in the same loop -- on the library's
kernels at 256 features and, with ``--wideKernel``, at the other widths, on torch ops otherwise; all write the same files.

Two deliberate differences from the reference:

1. Log averages.  The reference divides the summed logs by the LAST STEP INDEX (utils.update_logs(logs, step)), so an epoch of
   N batches is scaled by N / (N - 1) and an epoch of one batch divides by zero.  Here the averages divide by the number of
   batches; ``"iter"`` keeps the reference's value, the last step index.
2. No per-step host reads.  The reference calls ``.item()`` twice per step; here loss and accuracy accumulate on the device
   in float64 and are read once at the end of the epoch, where ``ops.check_device_errors()`` is also called.
"""
import argparse
import json
import sys
import time
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch

from . import criterion as cr
from .dataset import AudioBatchData, filterSeqs, findAllSeqs, parseSeqLabels

FUSED_PROBE = True             # frozen SpeakerCriterion / PhoneCriterion steps through ops.probe_train_step / probe_eval (False: always autograd)


def get_module(module):
    """cpc/feature_loader.py:193-198."""
    if isinstance(module, torch.nn.DataParallel):
        return get_module(module.module)
    return module


def _probe_of(feature_maker, criterion):
    """The (classifier layer, kind) the fused probe step applies to, or None."""
    crit = get_module(criterion)
    if not FUSED_PROBE or getattr(feature_maker, "optimize", True):
        return None
    if not (getattr(crit, "hip_path", False) or getattr(crit, "hip_wide", False)):
        return None
    if isinstance(crit, cr.SpeakerCriterion):
        return crit.linearSpeakerClassifier, "speaker"
    if isinstance(crit, cr.PhoneCriterion):
        return crit.PhoneCriterionClassifier, "phone"
    return None


def _probe_rows(criterion, kind, c_feature, encoded_data, label):
    """What the criterion's forward would classify: (rows (R, D), labels (R,)), or None when the features are not CUDA fp32."""
    if kind == "speaker":
        features = c_feature[:, -1, :]                   # read in place through its row stride
    else:
        features = encoded_data if get_module(criterion).onEncoder else c_feature
        B, S = features.size(0), features.size(1)
        if label.dim() != 2 or tuple(label.shape) != (B, S):
            raise ValueError(f"PhoneCriterion: per-frame labels of shape ({B}, {S}) expected, got {tuple(label.shape)}")
        features = features.reshape(B * S, -1)
    if not (features.is_cuda and features.dtype == torch.float32):
        return None
    return features, label.reshape(-1)


class _EpochSums:
    """Loss and accuracy summed on the device in float64, read once."""

    def __init__(self):
        self.accum = None
        self.out = None

    def on(self, device):
        if self.accum is None:
            self.accum = torch.zeros(2, dtype=torch.float64, device=device)
            self.out = (torch.empty(1, 1, dtype=torch.float32, device=device), torch.empty(1, 1, dtype=torch.float64, device=device))
        return self.accum

    def add(self, all_losses, all_acc):
        accum = self.on(all_losses.device)
        accum[0] += all_losses.detach().mean().double()
        accum[1] += all_acc.detach().mean().double().to(accum.device)

    def means(self, n_batches):
        if n_batches == 0:
            raise ValueError("the data loader gave no batch")
        if self.accum.is_cuda:
            from . import ops
            with torch.cuda.device(self.accum.device):
                ops.check_device_errors()
        loss, acc = (self.accum / n_batches).tolist()
        return np.asarray([loss]), np.asarray([acc])


def train_step(feature_maker, criterion, data_loader, optimizer):
    """cpc/eval/linear_separability.py:21-47 -> {"locLoss_train", "locAcc_train", "iter"}."""
    if feature_maker.optimize:
        feature_maker.train()
    criterion.train()
    probe = _probe_of(feature_maker, criterion)
    if probe is not None:
        from . import ops, optim
        if not isinstance(optimizer, optim.Adam):
            probe = None
    sums, n, step = _EpochSums(), 0, -1
    for step, (batch_data, label) in enumerate(data_loader):
        n += 1
        with torch.enable_grad() if feature_maker.optimize else torch.no_grad():
            c_feature, encoded_data, _ = feature_maker(batch_data, None)
        if not feature_maker.optimize:
            c_feature, encoded_data = c_feature.detach(), encoded_data.detach()
        rows = None if probe is None else _probe_rows(criterion, probe[1], c_feature, encoded_data, label)
        if rows is not None:
            lin = probe[0]
            accum = sums.on(rows[0].device)
            ops.probe_train_step(rows[0], rows[1], lin.weight, lin.bias, optimizer, accum=accum, out=sums.out)
            continue
        optimizer.zero_grad()
        all_losses, all_acc = criterion(c_feature, encoded_data, label)
        all_losses.sum().backward()
        optimizer.step()
        sums.add(all_losses, all_acc)
    loss, acc = sums.means(n)
    return {"locLoss_train": loss, "locAcc_train": acc, "iter": step}


def val_step(feature_maker, criterion, data_loader):
    """cpc/eval/linear_separability.py:50-68 -> {"locLoss_val", "locAcc_val"}."""
    feature_maker.eval()
    criterion.eval()
    probe = _probe_of(feature_maker, criterion)
    if probe is not None:
        from . import ops
    sums, n = _EpochSums(), 0
    for batch_data, label in data_loader:
        n += 1
        with torch.no_grad():
            c_feature, encoded_data, _ = feature_maker(batch_data, None)
            rows = None if probe is None else _probe_rows(criterion, probe[1], c_feature, encoded_data, label)
            if rows is not None:
                lin = probe[0]
                accum = sums.on(rows[0].device)
                ops.probe_eval(rows[0], rows[1], lin.weight, lin.bias, accum=accum, out=sums.out)
                continue
            all_losses, all_acc = criterion(c_feature, encoded_data, label)
            sums.add(all_losses, all_acc)
    loss, acc = sums.means(n)
    return {"locLoss_val": loss, "locAcc_val": acc}


def show_logs(text, logs):
    print("")
    print("-" * 50)
    print(text)
    for key, value in logs.items():
        if key != "iter":
            print(f"{key:>16} " + " ".join(f"{v:10.6f}" for v in value))
    print("-" * 50)


def run(feature_maker, criterion, train_loader, val_loader, optimizer, logs, n_epochs, path_checkpoint):
    """cpc/eval/linear_separability.py:71-118: the epoch loop, the best-state rule and the save rule."""
    from .harness import save_checkpoint, save_logs
    start_epoch = len(logs["epoch"])
    best_acc, best_state = -1, None
    start_time = time.time()
    for epoch in range(start_epoch, n_epochs):
        logs_train = train_step(feature_maker, criterion, train_loader, optimizer)
        logs_val = val_step(feature_maker, criterion, val_loader)
        print("")
        print("_" * 50)
        print(f"Ran {epoch + 1} epochs in {time.time() - start_time:.2f} seconds")
        show_logs("Training loss", logs_train)
        show_logs("Validation loss", logs_val)
        print("_" * 50)
        print("")
        if logs_val["locAcc_val"] > best_acc:
            best_state = deepcopy(get_module(feature_maker).state_dict())
            best_acc = logs_val["locAcc_val"]
        logs["epoch"].append(epoch)
        for key, value in dict(logs_train, **logs_val).items():
            if key not in logs:
                logs[key] = [None for _ in range(epoch)]
            if isinstance(value, np.ndarray):
                value = value.tolist()
            logs[key].append(value)
        if (epoch % logs["saveStep"] == 0 and epoch > 0) or epoch == n_epochs - 1:
            save_checkpoint(get_module(feature_maker).state_dict(), get_module(criterion).state_dict(), optimizer.state_dict(),
                            best_state, f"{path_checkpoint}_{epoch}.pt")
            save_logs(logs, f"{path_checkpoint}_logs.json")


def parse_args(argv):
    parser = argparse.ArgumentParser(description='Linear separability trainer (default test in speaker separability)')
    parser.add_argument('pathDB', type=str, help="Path to the directory containing the audio data.")
    parser.add_argument('pathTrain', type=str, help="Path to the list of the training sequences.")
    parser.add_argument('pathVal', type=str, help="Path to the list of the test sequences.")
    parser.add_argument('load', type=str, nargs='*', help="Path to the checkpoint to evaluate.")
    parser.add_argument('--pathPhone', type=str, default=None,
                        help="Path to the phone labels. If given, will compute the phone separability.")
    parser.add_argument('--CTC', action='store_true', help="Use the CTC loss (for phone separability only)")
    parser.add_argument('--pathCheckpoint', type=str, default='out',
                        help="Path of the output directory where the checkpoints should be dumped.")
    parser.add_argument('--nGPU', type=int, default=-1,
                        help='Scales the batch to batchSizeGPU * nGPU (the work runs on one GPU). Default=-1: 1')
    parser.add_argument('--batchSizeGPU', type=int, default=8, help='Batch size per GPU.')
    parser.add_argument('--n_epoch', type=int, default=10)
    parser.add_argument('--debug', action='store_true', help='If activated, will load only a small number of audio data.')
    parser.add_argument('--unfrozen', action='store_true',
                        help="If activated, update the feature network as well as the linear classifier")
    parser.add_argument('--no_pretraining', action='store_true', help="If activated, work from an untrained model.")
    parser.add_argument('--file_extension', type=str, default=".flac", help="Extension of the audio files in pathDB.")
    parser.add_argument('--save_step', type=int, default=-1,
                        help="Frequency at which a checkpoint should be saved, set to -1 (default) to save only the last one.")
    parser.add_argument('--get_encoded', action='store_true',
                        help="If activated, will work with the output of the convolutional encoder (see CPC's architecture).")
    parser.add_argument('--lr', type=float, default=2e-4, help='Learning rate.')
    parser.add_argument('--beta1', type=float, default=0.9, help='Value of beta1 for the Adam optimizer.')
    parser.add_argument('--beta2', type=float, default=0.999, help='Value of beta2 for the Adam optimizer.')
    parser.add_argument('--epsilon', type=float, default=2e-8, help='Value of epsilon for the Adam optimizer.')
    parser.add_argument('--ignore_cache', action='store_true', help="Activate if the sequences in pathDB have changed.")
    parser.add_argument('--size_window', type=int, default=20480, help="Number of frames to consider in each batch.")
    # (an addition.  Off by default, and then absent from the namespace: the reference's argument lists keep parsing to the
    # reference's namespace, which is also what checkpoint_args.json records)
    parser.add_argument('--wideKernel', action='store_true', default=argparse.SUPPRESS,
                        help="Run the classifier on the HIP kernels at feature widths other than 256 as well (1 to 512).")
    parser.add_argument('--encoderKernel', action='store_true', default=argparse.SUPPRESS,
                        help="The convolutional encoder on the HIP kernels at every width from 2 to 512 and under every normMode the checkpoint "
                             "was trained with (off by default: 256 channels under layerNorm only, everything else on torch ops).")
    args = parser.parse_args(argv)
    if args.nGPU < 0:
        args.nGPU = 1
    if args.save_step <= 0:
        args.save_step = args.n_epoch
    args.load = [str(Path(x).resolve()) for x in args.load]
    args.pathCheckpoint = str(Path(args.pathCheckpoint).resolve())
    return args


def main(argv):
    from . import optim
    from .common_voices_eval import load_feature_maker
    args = parse_args(argv)
    wide = getattr(args, "wideKernel", False)
    logs = {"epoch": [], "iter": [], "saveStep": args.save_step}
    if len(args.load) > 1:
        raise ValueError("concatenated models (more than one checkpoint) are not supported")
    if len(args.load) == 0:
        raise ValueError("a checkpoint to evaluate is required")
    seqNames, speakers = findAllSeqs(args.pathDB, extension=args.file_extension, loadCache=not args.ignore_cache)
    model, hidden_gar, _ = load_feature_maker(args.load[0], no_pretraining=args.no_pretraining,
                                             encoderKernel=getattr(args, "encoderKernel", False))
    hidden_encoder = model.gEncoder.getDimOutput()
    model.cuda()
    dim_features = hidden_encoder if args.get_encoded else hidden_gar

    phone_labels = None
    if args.pathPhone is not None:
        phone_labels, n_phones = parseSeqLabels(args.pathPhone)
        if not args.CTC:
            print("Running phone separability with aligned phones")
            criterion = cr.PhoneCriterion(dim_features, n_phones, args.get_encoded, wideKernel=wide)
        else:
            print("Running phone separability with CTC loss")
            criterion = cr.CTCPhoneCriterion(dim_features, n_phones, args.get_encoded, wideKernel=wide)
    else:
        print("Running speaker separability")
        criterion = cr.SpeakerCriterion(dim_features, len(speakers), wideKernel=wide)
    criterion.cuda()

    seq_train = filterSeqs(args.pathTrain, seqNames)
    seq_val = filterSeqs(args.pathVal, seqNames)
    if args.debug:
        seq_train = seq_train[:1000]
        seq_val = seq_val[:100]
    db_train = AudioBatchData(args.pathDB, args.size_window, seq_train, phone_labels, len(speakers)).to("cuda")
    db_val = AudioBatchData(args.pathDB, args.size_window, seq_val, phone_labels, len(speakers)).to("cuda")
    batch_size = args.batchSizeGPU * max(args.nGPU, 1)
    train_loader = db_train.getDataLoader(batch_size, "uniform", True, numWorkers=0)
    val_loader = db_val.getDataLoader(batch_size, "sequential", False, numWorkers=0)

    g_params = list(criterion.parameters())
    model.optimize = False
    model.eval()
    if args.unfrozen:
        print("Working in full fine-tune mode")
        g_params += list(model.parameters())
        model.optimize = True
    else:
        print("Working with frozen features")
        for g in model.parameters():
            g.requires_grad = False
    optimizer = optim.Adam(g_params, lr=args.lr, betas=(args.beta1, args.beta2), eps=args.epsilon)

    args.pathCheckpoint = Path(args.pathCheckpoint)
    args.pathCheckpoint.mkdir(exist_ok=True)
    args.pathCheckpoint = str(args.pathCheckpoint / "checkpoint")
    with open(f"{args.pathCheckpoint}_args.json", 'w') as file:
        json.dump(vars(args), file, indent=2)
    run(model, criterion, train_loader, val_loader, optimizer, logs, args.n_epoch, args.pathCheckpoint)


if __name__ == "__main__":
    main(sys.argv[1:])
