"""Phone recognition and PER on the CommonVoice pipeline (cpc/eval/common_voices_eval.py of the reference).

    python -m cpc_audio_amd.common_voices_eval train pathDB pathPhone pathCheckpoint [-o out] [...]
    python -m cpc_audio_amd.common_voices_eval per out [--pathDB ...] [--name 0]

The same commands, arguments and files as the reference: args_training.json, args_validation_<name>.json, logs_train.txt /
logs_per_<name>.txt, and out/checkpoint.pt = {'classifier', 'model', 'bestLoss'} with the reference's DataParallel key layout
('module.' prefix); either layout loads.  One process per GPU, no DataParallel at run time.

The reference was written for torch 1.4, where integer tensor division floors; here every length is floor-divided:
  CTC input lengths   (sizeSeq // downsampling) // 4, clamped to the classifier's output length after cutting the batch to its
                      longest sequence (the reference's clamp against the batch maximum)
  beam search length  T_b = min(sizeSeq_b // downsampling // 4, S'), S' the classifier's output length
PER: perStep decodes a whole batch with seq_alignment.beam_search_batch (beams of 20, csrc/ctc_decode.hip) and aligns it with
seq_alignment.seq_per_batch on the device -- no host round trip in between, no process pool -- and accumulates the mean and
sqrt(E[x^2] - mean^2) in float64 in loader order.

The classifier's head and loss -- Conv1d (k 8, stride 4) on 256 features, log_softmax and nn.CTCLoss with the utterances'
lengths -- run on csrc/phone_head.hip (ops.PhoneHeadCtcFunction, ops.phone_head_logits; `--hipHead` / `--no-hipHead`, see
CTCphone_criterion).  What stands in front of the head -- seqNorm, the optional LSTM and the dropout -- runs on
csrc/seqnorm.hip and csrc/lstm.hip with `--hipFront` (ops.SeqNormFunction, ops.LstmFunction: no host synchronisation, no
per-utterance launches) and as torch GPU ops without it (the default); the whole classifier is torch ops for another feature
width or kernel size -- unless `--wideKernel` is given, with which head and front run on the same kernels at any width from 1
to 512 (only the `--LSTM` recurrence, whose hidden width follows the features, stays on nn.LSTM away from 256).  CPC checkpoints load as abx.py loads them (checkpoint_args.json next to the checkpoint,
harness.load_checkpoint); their encoder and autoregressor run on the package's HIP kernels.
"""
import argparse
import json
import math
import os
import random
import sys
import time
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import ops
from . import seq_alignment as SA
from .dataset import filterSeqs, findAllSeqs, loadFile, parseSeqLabels

N_KEEP = 20           # perStep's beams
HIP_HEAD_DEFAULT = True   # what CTCphone_criterion(hipHead=None) means where the HIP head applies
HIP_FRONT_DEFAULT = False  # what CTCphone_criterion(hipFront=None) means: the torch front


def load(path_item):
    """-> (sequence name, (channels, samples) float tensor).  Audio goes through dataset.py's readers (mono); a .npy / .pt
    file of pre-computed features keeps its (channels, frames) rows."""
    path_item = Path(path_item)
    if path_item.suffix.lower() in (".npy", ".pt"):
        x = torch.from_numpy(np.load(str(path_item))) if path_item.suffix.lower() == ".npy" else torch.load(str(path_item))
        x = x.float()
        return path_item.stem, x.view(1, -1) if x.dim() == 1 else x
    _, name, wav = loadFile((0, str(path_item)))
    return name, wav.view(1, -1)


class SingleSequenceDataset(Dataset):
    """Whole utterances padded to the longest one: (sequence (inDim, maxSize), [size], phones (maxSizePhone,), [sizePhone])."""

    def __init__(self, pathDB, seqNames, phoneLabelsDict, inDim=1, transpose=True):
        self.seqNames = deepcopy(seqNames)
        self.pathDB = pathDB
        self.phoneLabelsDict = deepcopy(phoneLabelsDict)
        self.inDim = inDim
        self.transpose = transpose
        self.loadSeqs()

    def loadSeqs(self):
        self.seqOffset = [0]
        self.phoneLabels = []
        self.phoneOffsets = [0]
        self.maxSize = 0
        self.maxSizePhone = 0
        start_time = time.time()
        loaded = sorted((load(Path(self.pathDB) / x) for _, x in self.seqNames), key=lambda item: item[0])
        tmp, tot, min_phone = [], 0, float("inf")
        for name, seq in loaded:
            labels = self.phoneLabelsDict[name]
            self.phoneLabels += labels
            self.phoneOffsets.append(len(self.phoneLabels))
            self.maxSizePhone = max(self.maxSizePhone, len(labels))
            min_phone = min(min_phone, len(labels))
            n = seq.size(1)
            self.maxSize = max(self.maxSize, n)
            tot += n
            tmp.append(seq)
            self.seqOffset.append(self.seqOffset[-1] + n)
        self.data = torch.cat(tmp, dim=1)
        self.phoneLabels = torch.tensor(self.phoneLabels, dtype=torch.long)
        print(f'Loaded {len(self.phoneOffsets)} sequences in {time.time() - start_time:.2f} seconds')
        print(f'maxSizeSeq : {self.maxSize}')
        print(f'maxSizePhone : {self.maxSizePhone}')
        print(f"minSizePhone : {min_phone}")
        print(f'Total size dataset {tot / (16000 * 3600)} hours')

    def __getitem__(self, idx):
        o0, o1 = self.seqOffset[idx], self.seqOffset[idx + 1]
        p0, p1 = self.phoneOffsets[idx], self.phoneOffsets[idx + 1]
        size_seq, size_phone = int(o1 - o0), int(p1 - p0)
        out_seq = torch.zeros((self.inDim, self.maxSize))
        out_phone = torch.zeros((self.maxSizePhone))
        out_seq[:, :size_seq] = self.data[:, o0:o1]
        out_phone[:size_phone] = self.phoneLabels[p0:p1]
        return out_seq, torch.tensor([size_seq], dtype=torch.long), out_phone.long(), torch.tensor([size_phone], dtype=torch.long)

    def __len__(self):
        return len(self.seqOffset) - 1


def ctc_input_lengths(size_seq, downsampling_factor):
    """Frames of the classifier's output per utterance: (sizeSeq // downsampling) // 4."""
    return (size_seq // downsampling_factor) // 4


class CTCphone_criterion(torch.nn.Module):
    """The reference's phone classifier: optional 1-layer LSTM (conv1), Conv1d(dim, nPhones + 1, sizeKernel, stride
    sizeKernel // 2), nn.CTCLoss(blank=nPhones, zero_infinity=True).  Same state-dict keys.  getPrediction takes the
    per-utterance feature lengths (sizeSeq // downsampling) and does not write into its input.

    hipHead: the Conv1d, log_softmax and the CTC loss on csrc/phone_head.hip.  That path takes dimEncoder 256, sizeKernel 8,
    CUDA fp32 features and what cpc_phone_head_layout accepts.  None: use it where it applies (HIP_HEAD_DEFAULT), torch
    elsewhere; False: torch; True: the HIP path or NotImplementedError.  On it getPrediction is not differentiable
    (evaluation); forward is.  last_path names the path of the last call.

    hipFront: what stands in front of the head on HIP kernels, whichever head reads it -- seqNorm and the dropout on
    csrc/seqnorm.hip (ops.SeqNormFunction: the utterances' lengths are read on the device, the dropout is a per-(utterance,
    channel) factor of 0 or 2 folded into the normalisation's scale), the LSTM on csrc/lstm.hip (ops.LstmFunction on conv1's
    parameters).  It takes dimEncoder 256 and CUDA fp32 features.  None: HIP_FRONT_DEFAULT (off); False: the torch ops; True:
    the HIP front or NotImplementedError.  The dropout's factors come from torch's generator (bernoulli_(0.5) * 2: the
    distribution of nn.Dropout2d on (B, 256, S), not its bits) and stay in last_channel_scale; last_front names the front of
    the last call ("hip", "torch", None when no front op was active).

    wideKernel (off by default): the HIP head and the HIP front at any dimEncoder from 1 to 512 (cpc_phone_head_*_d,
    cpc_seqnorm_*_d); sizeKernel is still 8, and hipHead and hipFront keep their three meanings.  The LSTM is nn.LSTM(dimEncoder,
    dimEncoder): its hidden width follows dimEncoder, and csrc/lstm.hip's recurrence is 256 wide.  So away from 256 the HIP
    front is the HIP seqNorm, then nn.LSTM (MIOpen), then the HIP dropout scale; last_front stays "hip" and last_lstm names the
    recurrence's path of the last call ("hip", "torch", None without --LSTM or when no front op was active).

    hiddenKernel (off by default; with wideKernel): away from 256 the front's LSTM runs on the LSTM kernels of any hidden width
    too (ops.LstmHiddenFunction, cpc_lstm_forward_h at D = H = dimEncoder) and last_lstm is "hip" there."""

    def __init__(self, dimEncoder, nPhones, LSTM=False, sizeKernel=8, seqNorm=False, dropout=False, reduction='sum',
                 hipHead=None, hipFront=None, wideKernel=False, hiddenKernel=False):
        super().__init__()
        self.hipHead = hipHead
        self.hipFront = hipFront
        self.wideKernel = bool(wideKernel)
        widths = f"1 <= dimEncoder <= {ops.PHONE_HEAD_MAX_DIM}" if self.wideKernel else "dimEncoder 256"
        width_ok = 1 <= dimEncoder <= ops.PHONE_HEAD_MAX_DIM if self.wideKernel else dimEncoder == 256
        self._hipConfig = width_ok and sizeKernel == ops.PHONE_HEAD_KERNEL
        if hipHead and not self._hipConfig:
            raise NotImplementedError(f"CTCphone_criterion(hipHead=True): the HIP phone head is built for {widths} and "
                                      f"sizeKernel 8 (got {dimEncoder}, {sizeKernel})")
        self._hipFrontConfig = width_ok
        if hipFront and not self._hipFrontConfig:
            raise NotImplementedError("CTCphone_criterion(hipFront=True): the HIP seqNorm, LSTM and dropout are built for "
                                      f"{widths} (got {dimEncoder})")
        self._hipLstmConfig = dimEncoder == 256            # csrc/lstm.hip: a recurrence 256 wide
        self.hiddenKernel = bool(hiddenKernel)
        # ... or, asked for, the recurrence of any hidden width (cpc_lstm_*_h)
        self._hipLstmHidden = (self.hiddenKernel and self.wideKernel and dimEncoder != 256
                               and 1 <= dimEncoder <= ops.LSTM_HIDDEN_MAX)
        self.last_path = None
        self.last_front = None
        self.last_lstm = None
        self.last_channel_scale = None
        self.seqNorm = seqNorm
        self.epsilon = 1e-8
        self.dropout = torch.nn.Dropout2d(p=0.5, inplace=False) if dropout else None
        self.conv1 = torch.nn.LSTM(dimEncoder, dimEncoder, num_layers=1, batch_first=True)
        self.PhoneCriterionClassifier = torch.nn.Conv1d(dimEncoder, nPhones + 1, sizeKernel, stride=sizeKernel // 2)
        self.lossCriterion = torch.nn.CTCLoss(blank=nPhones, reduction=reduction, zero_infinity=True)
        self.relu = torch.nn.ReLU()
        self.BLANK_LABEL = nPhones
        self.useLSTM = LSTM

    def _hipPath(self, cFeature, Lmax=0):
        """Does this call run on the HIP head?"""
        if self.hipHead is False or (self.hipHead is None and not HIP_HEAD_DEFAULT) or not self._hipConfig:
            return False
        B, S, D = cFeature.size()
        ok = cFeature.is_cuda and cFeature.dtype == torch.float32 and \
            ops.phone_head_supported(B, S, self.BLANK_LABEL + 1, Lmax, D)
        if self.hipHead and not ok:
            raise NotImplementedError("CTCphone_criterion(hipHead=True): the HIP phone head takes CUDA fp32 features of a shape "
                                      f"cpc_phone_head_layout accepts (got {tuple(cFeature.size())}, {cFeature.dtype}, "
                                      f"{cFeature.device}, {Lmax} target columns)")
        return ok

    def _hipFrontPath(self, cFeature):
        """Does this call run its seqNorm, LSTM and dropout on the HIP kernels?"""
        if self.hipFront is False or (self.hipFront is None and not HIP_FRONT_DEFAULT) or not self._hipFrontConfig:
            return False
        B, S, D = cFeature.size()
        ok = cFeature.is_cuda and cFeature.dtype == torch.float32 and ops.seqnorm_supported(B, S, D) and \
            (not self.useLSTM or not self._hipLstmConfig or ops.lstm_supported(B, S)) and \
            (not self.useLSTM or not self._hipLstmHidden or ops.lstm_hidden_supported(B, S, 1, D, D))
        if self.hipFront and not ok:
            raise NotImplementedError("CTCphone_criterion(hipFront=True): the HIP front takes CUDA fp32 features of a shape "
                                      f"cpc_seqnorm_forward and cpc_lstm_layout accept (got {tuple(cFeature.size())}, "
                                      f"{cFeature.dtype}, {cFeature.device})")
        return ok

    def _front(self, cFeature, featureSize):
        """What the head reads, channels-last (B, S, H): seqNorm, the LSTM and the dropout.  Never writes into cFeature."""
        B, S, H = cFeature.size()
        drop = self.dropout is not None and self.training
        self.last_channel_scale = None
        self.last_lstm = None
        if not (self.seqNorm or self.useLSTM or drop):
            self.last_front = None
            return cFeature
        if self._hipFrontPath(cFeature):
            self.last_front = "hip"
            scale = cFeature.new_empty(B, H).bernoulli_(0.5).mul_(2) if drop else None
            self.last_channel_scale = scale
            if self.seqNorm:                       # the dropout rides on the normalisation unless the LSTM stands between
                cFeature = ops.SeqNormFunction.apply(cFeature, featureSize, None if self.useLSTM else scale, True)
            if self.useLSTM and self._hipLstmConfig:
                self.last_lstm = "hip"
                cFeature = ops.LstmFunction.apply(cFeature, None, False, self.conv1.weight_ih_l0, self.conv1.weight_hh_l0,
                                                  self.conv1.bias_ih_l0, self.conv1.bias_hh_l0)[0]
            elif self.useLSTM and self._hipLstmHidden:
                self.last_lstm = "hip"
                cFeature = ops.LstmHiddenFunction.apply(cFeature, None, False, self.conv1.weight_ih_l0, self.conv1.weight_hh_l0,
                                                        self.conv1.bias_ih_l0, self.conv1.bias_hh_l0)[0]
            elif self.useLSTM:                     # a hidden width other than 256 without hiddenKernel: stays on MIOpen
                self.last_lstm = "torch"
                cFeature = self.conv1(cFeature)[0]
            if drop and (self.useLSTM or not self.seqNorm):
                cFeature = ops.SeqNormFunction.apply(cFeature, None, scale, False)
            return cFeature
        self.last_front = "torch"
        if self.seqNorm:
            rows = []
            for b in range(B):
                size = int(featureSize[b])
                m = cFeature[b, :size].mean(dim=0, keepdim=True)
                v = cFeature[b, :size].var(dim=0, keepdim=True)
                rows.append((cFeature[b] - m) / torch.sqrt(v + self.epsilon))
            cFeature = torch.stack(rows)
        if self.useLSTM:
            self.last_lstm = "torch"
            cFeature = self.conv1(cFeature)[0]
        if self.dropout is not None:
            cFeature = self.dropout(cFeature.permute(0, 2, 1)).permute(0, 2, 1)
        return cFeature

    def getPrediction(self, cFeature, featureSize):
        head = self.PhoneCriterionClassifier
        if self._hipPath(cFeature):
            self.last_path = "hip"
            return ops.phone_head_logits(self._front(cFeature, featureSize), head.weight, head.bias)
        self.last_path = "torch"
        return head(self._front(cFeature, featureSize).permute(0, 2, 1)).permute(0, 2, 1)

    def forward(self, cFeature, featureSize, label, labelSize):
        """featureSize: sizeSeq // downsampling per utterance (integer tensor)."""
        if self._hipPath(cFeature, label.size(1)):
            # the lengths do cut_data's work on the device: no .max() round trip, no copies
            self.last_path = "hip"
            head = self.PhoneCriterionClassifier
            nWindows = (cFeature.size(1) - ops.PHONE_HEAD_KERNEL) // ops.PHONE_HEAD_STRIDE + 1
            loss = ops.PhoneHeadCtcFunction.apply(self._front(cFeature, featureSize), head.weight, head.bias,
                                                  torch.clamp(featureSize // 4, max=nWindows), label, labelSize,
                                                  self.BLANK_LABEL, self.lossCriterion.reduction).view(1, -1)
            if torch.isinf(loss).sum() > 0 or torch.isnan(loss).sum() > 0:
                loss = loss.new_zeros(1, 1).requires_grad_()
            return loss
        predictions = self.getPrediction(cFeature, featureSize)
        featureSize = featureSize // 4
        predictions = cut_data(predictions, featureSize)
        featureSize = torch.clamp(featureSize, max=predictions.size(1))
        label = cut_data(label, labelSize)
        if labelSize.min() <= 0:
            print(label, labelSize)
        predictions = torch.nn.functional.log_softmax(predictions, dim=2).permute(1, 0, 2)
        loss = self.lossCriterion(predictions, label, featureSize, labelSize).view(1, -1)
        if torch.isinf(loss).sum() > 0 or torch.isnan(loss).sum() > 0:
            loss = loss.new_zeros(1, 1).requires_grad_()
        return loss


class IDModule(torch.nn.Module):
    """Pre-computed features: (B, C, S) -> ((B, S, C), None, None)."""

    def forward(self, feature, *args):
        return feature.permute(0, 2, 1), None, None


def cut_data(seq, sizeSeq):
    return seq[:, :int(sizeSeq.max())]


def prepare_data(data):
    seq, sizeSeq, phone, sizePhone = data
    seq = seq.cuda(non_blocking=True)
    phone = phone.cuda(non_blocking=True)
    sizeSeq = sizeSeq.cuda(non_blocking=True).view(-1)
    sizePhone = sizePhone.cuda(non_blocking=True).view(-1)
    seq = cut_data(seq.permute(0, 2, 1), sizeSeq).permute(0, 2, 1)
    return seq, sizeSeq, phone, sizePhone


def _module(m):
    return getattr(m, "module", m)


def train_step(train_loader, model, criterion, optimizer, downsampling_factor):
    if getattr(model, "optimize", True):
        model.train()
    criterion.train()
    avg_loss, n_items = 0, 0
    for data in train_loader:
        optimizer.zero_grad()
        seq, sizeSeq, phone, sizePhone = prepare_data(data)
        c_feature, _, _ = model(seq, None)
        if not getattr(model, "optimize", True):
            c_feature = c_feature.detach()
        loss = criterion(c_feature, sizeSeq // downsampling_factor, phone, sizePhone)
        loss.mean().backward()
        avg_loss += loss.mean().item()
        n_items += 1
        optimizer.step()
    return avg_loss / n_items


def val_step(val_loader, model, criterion, downsampling_factor):
    model.eval()
    criterion.eval()
    avg_loss, n_items = 0, 0
    for data in val_loader:
        with torch.no_grad():
            seq, sizeSeq, phone, sizePhone = prepare_data(data)
            c_feature, _, _ = model(seq, None)
            loss = criterion(c_feature, sizeSeq // downsampling_factor, phone, sizePhone)
            avg_loss += loss.mean().item()
            n_items += 1
    return avg_loss / n_items


def get_per(data):
    """One utterance, as the reference's pool worker: (pred (S', P), size_pred, gt, size_gt, blank_label) -> PER, beams of 20."""
    pred, size_pred, gt, size_gt, blank_label = data
    l_ = min(int(size_pred) // 4, pred.size(0))
    p_ = pred[:l_].reshape(l_, -1).cpu().numpy()
    gt_seq = gt[:int(size_gt)].view(-1).tolist()
    pred_seq = SA.beam_search(p_, N_KEEP, blank_label)[0][1]
    return SA.get_seq_PER(gt_seq, pred_seq)


def batch_per(predictions, sizeSeq, phone, sizePhone, blank_label):
    """PER of every utterance of a batch on the device: softmax outputs (B, S', P), sizeSeq // downsampling (B,) ->
    (B,) float64 device tensor."""
    lengths = torch.clamp(sizeSeq // 4, max=predictions.size(1)).to(torch.int32)
    lab, lab_len, _, _ = SA.beam_search_batch(predictions, lengths, N_KEEP, blank_label)
    return SA.seq_per_batch(phone, sizePhone, lab[:, 0], lab_len[:, 0])


def perStep(val_loader, model, criterion, downsampling_factor):
    """-> (mean PER, standard deviation), printed as the reference prints them."""
    model.eval()
    criterion.eval()
    crit = _module(criterion)
    avg, var, n_items = 0.0, 0.0, 0
    print("Starting the PER computation through beam search")
    for data in val_loader:
        with torch.no_grad():
            seq, sizeSeq, phone, sizePhone = prepare_data(data)
            c_feature, _, _ = model(seq, None)
            sizeSeq = sizeSeq // downsampling_factor
            predictions = torch.nn.functional.softmax(crit.getPrediction(c_feature, sizeSeq), dim=2)
            values = batch_per(predictions.contiguous(), sizeSeq, phone, sizePhone, crit.BLANK_LABEL).cpu().tolist()
        avg += sum(values)
        var += sum(x * x for x in values)
        n_items += len(values)
    avg /= n_items
    var /= n_items
    var -= avg ** 2
    std = math.sqrt(max(var, 0.0))
    print(f"Average PER {avg}")
    print(f"Standard deviation PER {std}")
    return avg, std


def with_module_prefix(state_dict):
    """The reference's checkpoint layout (both modules inside DataParallel)."""
    return {("module." + k if not k.startswith("module.") else k): v for k, v in state_dict.items()}


def without_module_prefix(state_dict):
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def run(train_loader, val_loader, model, criterion, optimizer, downsampling_factor, nEpochs, pathCheckpoint):
    print(f"Starting the training for {nEpochs} epochs")
    best = float('inf')
    for epoch in range(nEpochs):
        loss_train = train_step(train_loader, model, criterion, optimizer, downsampling_factor)
        print(f"Epoch {epoch} loss train : {loss_train}")
        loss_val = val_step(val_loader, model, criterion, downsampling_factor)
        print(f"Epoch {epoch} loss val : {loss_val}")
        if loss_val < best:
            best = loss_val
            torch.save({'classifier': with_module_prefix(criterion.state_dict()),
                        'model': with_module_prefix(model.state_dict()), 'bestLoss': best}, pathCheckpoint)


def get_PER_args(args):
    with open(os.path.join(args.output, "args_training.json"), 'rb') as file:
        data = json.load(file)
    if args.pathDB is None:
        args.pathDB = data["pathDB"]
        args.file_extension = data["file_extension"]
    if args.pathVal is None and args.pathPhone is None:
        args.pathPhone = data["pathPhone"]
        args.pathVal = data["pathVal"]
    args.pathCheckpoint = data["pathCheckpoint"]
    args.no_pretraining = data["no_pretraining"]
    args.LSTM = data.get("LSTM", False)
    args.seqNorm = data.get("seqNorm", False)
    args.dropout = data.get("dropout", False)
    args.in_dim = data.get("in_dim", 1)
    args.loss_reduction = data.get("loss_reduction", "mean")
    args.hipHead = data.get("hipHead", None)
    args.hipFront = data.get("hipFront", None)
    if data.get("wideKernel", False):                      # (absent where the training run did not ask for it)
        args.wideKernel = True
    if data.get("hiddenKernel", False):
        args.hiddenKernel = True
    if data.get("encoderKernel", False):
        args.encoderKernel = True
    return args


def parse_args(argv):
    parser = argparse.ArgumentParser(description='Simple phone recognition pipeline for the common voices datasets')
    sub = parser.add_subparsers(dest='command')
    t = sub.add_parser('train')
    t.add_argument('pathDB', type=str, help='Path to the directory containing the audio data / pre-computed features.')
    t.add_argument('pathPhone', type=str, help='Path to the .txt file containing the phone transcription.')
    t.add_argument('pathCheckpoint', type=str, help='Path to the CPC checkpoint to load. Set to ID to work with pre-computed '
                   'features.')
    t.add_argument('--freeze', action='store_true', help="Freeze the CPC features layers")
    t.add_argument('--pathTrain', default=None, type=str, help='List of the training sequences.')
    t.add_argument('--pathVal', default=None, type=str, help='List of the validation sequences.')
    t.add_argument('--file_extension', type=str, default=".mp3", help='Extension of the files in the dataset')
    t.add_argument('--batchSize', type=int, default=8)
    t.add_argument('--nEpochs', type=int, default=30)
    t.add_argument('--beta1', type=float, default=0.9)
    t.add_argument('--beta2', type=float, default=0.999)
    t.add_argument('--epsilon', type=float, default=1e-08)
    t.add_argument('--lr', type=float, default=2e-04)
    t.add_argument('-o', '--output', type=str, default='out', help="Output directory")
    t.add_argument('--debug', action='store_true')
    t.add_argument('--no_pretraining', action='store_true')
    t.add_argument('--LSTM', action='store_true', help='Add a LSTM to the phone classifier')
    t.add_argument('--seqNorm', action='store_true', help='Normalize each sequence of features through time')
    t.add_argument('--kernelSize', type=int, default=8)
    t.add_argument('--dropout', action='store_true')
    t.add_argument('--in_dim', type=int, default=1, help='Dimension of the input data')
    t.add_argument('--loss_reduction', type=str, default='mean', choices=['mean', 'sum'])
    t.add_argument('--hipHead', dest='hipHead', action='store_true', default=None,
                   help="The classifier's head and CTC loss on the HIP kernels (an error where they do not apply)")
    t.add_argument('--no-hipHead', dest='hipHead', action='store_false', help="The classifier's head and CTC loss as torch ops")
    t.add_argument('--hipFront', dest='hipFront', action='store_true', default=None,
                   help="The classifier's seqNorm, LSTM and dropout on the HIP kernels (an error where they do not apply)")
    t.add_argument('--no-hipFront', dest='hipFront', action='store_false',
                   help="The classifier's seqNorm, LSTM and dropout as torch ops (the default)")
    t.add_argument('--wideKernel', action='store_true', default=argparse.SUPPRESS,
                   help="The HIP head and the HIP front at any feature width from 1 to 512 (off by default: 256 only); per reads "
                   "it back from the training run's arguments")
    t.add_argument('--hiddenKernel', action='store_true', default=argparse.SUPPRESS,
                   help="With --hipFront --wideKernel --LSTM: the LSTM at a feature width other than 256 on the HIP kernels too "
                   "(off by default: nn.LSTM there); per reads it back from the training run's arguments")
    t.add_argument('--encoderKernel', action='store_true', default=argparse.SUPPRESS,
                   help="The convolutional encoder on the HIP kernels at every width from 2 to 512 and under every normMode the checkpoint "
                   "was trained with (off by default: 256 channels under layerNorm only, everything else on torch ops); per reads "
                   "it back from the training run's arguments")
    p = sub.add_parser('per')
    p.add_argument('output', type=str)
    p.add_argument('--batchSize', type=int, default=8)
    p.add_argument('--debug', action='store_true')
    p.add_argument('--pathDB', type=str, default=None, help="For computing the PER on another dataset")
    p.add_argument('--pathVal', type=str, default=None, help="For computing the PER on specific sequences")
    p.add_argument('--pathPhone', type=str, default=None, help="For computing the PER on specific sequences")
    p.add_argument('--file_extension', type=str, default=".mp3")
    p.add_argument('--name', type=str, default="0")
    args = parser.parse_args(argv)
    if args.command is None:
        parser.error("choose train or per")
    return args


def load_feature_maker(path_checkpoint, no_pretraining=False, in_dim=1, encoderKernel=False):
    """-> (module, feature width, downsampling factor).  'ID': pre-computed features.  encoderKernel is build_model's; the
    checkpoint's normMode is read from its saved arguments."""
    if path_checkpoint == 'ID':
        return IDModule(), in_dim, 1
    from . import harness, train
    ckpt = Path(path_checkpoint)
    with open(ckpt.parent / "checkpoint_args.json") as f:
        saved = json.load(f)
    model = train.build_model(hiddenEncoder=saved.get("hiddenEncoder", 256), hiddenGar=saved.get("hiddenGar", 256),
                              nLevelsGRU=saved.get("nLevelsGRU", 1), arMode=saved.get("arMode", "LSTM"),
                              reverse=saved.get("cpc_mode") == "reverse", sizeWindow=saved.get("sizeWindow", 20480),
                              abspos=saved.get("abspos", False), encoder_type=saved.get("encoder_type", "cpc"),
                              mfccKernel=True, normMode=saved.get("normMode", "layerNorm"),
                              encoderKernel=encoderKernel)
    if not no_pretraining:
        harness.load_checkpoint(str(ckpt), model)
    width = saved.get("hiddenEncoder", 256) if saved.get("arMode", "LSTM") == "no_ar" else saved.get("hiddenGar", 256)
    return model, width, 160


class _Tee:
    def __init__(self, path, stream):
        self.file, self.stream = open(path, "w"), stream

    def write(self, s):
        self.stream.write(s)
        self.file.write(s)

    def flush(self):
        self.stream.flush()
        self.file.flush()


def main(argv):
    args = parse_args(argv)
    if args.command == 'per':
        args = get_PER_args(args)
    os.makedirs(args.output, exist_ok=True)
    name = f"_{args.name}" if args.command == "per" else ""
    stdout, tee = sys.stdout, _Tee(os.path.join(args.output, f'logs_{args.command}{name}.txt'), sys.stdout)
    sys.stdout = tee
    try:
        return _main(args)
    finally:
        sys.stdout = stdout
        tee.file.close()


def _main(args):
    phone_labels, n_phones = parseSeqLabels(args.pathPhone)
    in_seqs, _ = findAllSeqs(args.pathDB, extension=args.file_extension)
    if args.command == 'train' and args.pathTrain is not None:
        seq_train = filterSeqs(args.pathTrain, in_seqs)
    else:
        seq_train = in_seqs
    if args.pathVal is None and args.command == 'train':
        random.shuffle(seq_train)
        size_train = int(0.9 * len(seq_train))
        seq_train, seq_val = seq_train[:size_train], seq_train[size_train:]
    elif args.pathVal is not None:
        seq_val = filterSeqs(args.pathVal, in_seqs)
    else:
        raise RuntimeError("No validation dataset found for PER computation")
    if args.debug:
        seq_val = seq_val[:100]

    feature_maker, hidden_gar, downsampling_factor = load_feature_maker(args.pathCheckpoint, args.no_pretraining, args.in_dim,
                                                                           encoderKernel=getattr(args, "encoderKernel", False))
    feature_maker.cuda()
    phone_criterion = CTCphone_criterion(hidden_gar, n_phones, args.LSTM, seqNorm=args.seqNorm, dropout=args.dropout,
                                         reduction=args.loss_reduction, hipHead=args.hipHead, hipFront=args.hipFront,
                                         wideKernel=getattr(args, "wideKernel", False),
                                         hiddenKernel=getattr(args, "hiddenKernel", False)).cuda()
    print(f"Loading the validation dataset at {args.pathDB}")
    dataset_val = SingleSequenceDataset(args.pathDB, seq_val, phone_labels, inDim=args.in_dim)
    val_loader = DataLoader(dataset_val, batch_size=args.batchSize, shuffle=True)
    path_checkpoint = os.path.join(args.output, 'checkpoint.pt')

    if args.command == 'train':
        feature_maker.optimize = True
        if args.freeze:
            feature_maker.eval()
            feature_maker.optimize = False
            for g in feature_maker.parameters():
                g.requires_grad = False
        if args.debug:
            random.shuffle(seq_train)
            seq_train = seq_train[:1000]
        print(f"Loading the training dataset at {args.pathDB}")
        dataset_train = SingleSequenceDataset(args.pathDB, seq_train, phone_labels, inDim=args.in_dim)
        train_loader = DataLoader(dataset_train, batch_size=args.batchSize, shuffle=True)
        g_params = list(phone_criterion.parameters())
        if not args.freeze:
            print("Optimizing model")
            g_params += list(feature_maker.parameters())
        optimizer = torch.optim.Adam(g_params, lr=args.lr, betas=(args.beta1, args.beta2), eps=args.epsilon)
        with open(os.path.join(args.output, "args_training.json"), 'w') as file:
            json.dump(vars(args), file, indent=2)
        run(train_loader, val_loader, feature_maker, phone_criterion, optimizer, downsampling_factor, args.nEpochs,
            path_checkpoint)
        return None

    print(f"Loading data at {path_checkpoint}")
    state_dict = torch.load(path_checkpoint, map_location=lambda storage, loc: storage)
    if 'bestLoss' in state_dict:
        print(f"Best loss : {state_dict['bestLoss']}")
    phone_criterion.load_state_dict(without_module_prefix(state_dict['classifier']))
    feature_maker.load_state_dict(without_module_prefix(state_dict['model']))
    with open(os.path.join(args.output, f"args_validation_{args.name}.json"), 'w') as file:
        json.dump(vars(args), file, indent=2)
    return perStep(val_loader, feature_maker, phone_criterion, downsampling_factor)


if __name__ == "__main__":
    main(sys.argv[1:])
