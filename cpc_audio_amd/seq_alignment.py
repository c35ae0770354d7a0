"""PER decoding and alignment (cpc/criterion/seq_alignment.py of the reference) on csrc/ctc_decode.hip.

The reference's names and signatures -- beam_search, collapseLabelChain, NeedlemanWunschAlignScore, get_seq_PER, getPER -- take
what it takes (numpy arrays, lists, tensors) and compute on the GPU kernels; there is no CPU path.  The batched entry points
beam_search_batch and seq_per_batch take device tensors and return device tensors, so a caller (common_voices_eval.perStep)
decodes and scores a whole batch with no host round trip in between.

beam_search computes in the input's dtype (float32 stays float32, everything else is taken as float64) and gives the
reference's bits, ties included: the reference ranks candidates by (score, key) with key the string ",a,b,c", which orders
label sequences lexicographically with labels ranked by their decimal strings (decimal_rank) and a proper prefix first.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_KEEP = 128          # cpc_ctc_decode_layout sizes[4]
MAX_CLASSES = 128       # sizes[5]
MAX_HYP_LEN = 4096      # sizes[6]: longest hypothesis of cpc_nw_align_score
PAD = -1                # label padding of beam_search_batch


def decimal_rank(P):
    """rank[c] = position of str(c) among the decimal strings of 0 .. P-1 (the order the reference's string keys give labels)."""
    order = sorted(range(P), key=str)
    rank = np.empty(P, dtype=np.int64)
    rank[order] = np.arange(P)
    return rank


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("cpc_audio_amd.seq_alignment: needs an AMD GPU; this package has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None


def check_limits(P, n_keep, n_out=1):
    if not 1 <= n_keep <= MAX_KEEP:
        raise ValueError(f"beam_search: nKeep must be in [1, {MAX_KEEP}], got {n_keep}")
    if not 2 <= P <= MAX_CLASSES:
        raise ValueError(f"beam_search: the number of classes must be in [2, {MAX_CLASSES}], got {P}")
    if not 1 <= n_out <= n_keep:
        raise ValueError(f"beam_search: n_out must be in [1, nKeep], got {n_out}")


def launch_beam_search(lib, probs, lengths, n_keep, blank, n_out, stream=None):
    """cpc_ctc_beam_search on tensors that ``lib`` can address (device tensors for the product library) -> (labels (B, n_out,
    T) int32 padded with PAD, label_len (B, n_out) int32, scores (B, n_out) in probs' dtype, n_beams (B) int32)."""
    if probs.dim() != 3 or probs.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"beam_search_batch: probabilities (B, T, P) in float32 or float64 expected, got "
                         f"{tuple(probs.shape)} {probs.dtype}")
    B, T, P = probs.shape
    check_limits(P, n_keep, n_out)
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous():
        raise ValueError("beam_search_batch: lengths must be a contiguous (B,) int32 tensor")
    sizes = (ctypes.c_long * 7)()
    lib.check(lib.cpc_ctc_decode_layout(B, max(T, 1), P, n_keep, sizes), "ctc_decode_layout")
    dev = probs.device
    scratch = torch.empty(int(sizes[0]), dtype=torch.uint8, device=dev)
    labels = torch.empty(B, n_out, max(T, 1), dtype=torch.int32, device=dev)
    label_len = torch.empty(B, n_out, dtype=torch.int32, device=dev)
    scores = torch.empty(B, n_out, dtype=probs.dtype, device=dev)
    n_beams = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return labels, label_len, scores, n_beams
    sb, st, sp = probs.stride()
    lib.check(lib.cpc_ctc_beam_search(probs.data_ptr(), 0 if probs.dtype == torch.float32 else 1, sb, st, sp,
                                      lengths.data_ptr(), B, max(T, 1), P, int(blank), int(n_keep), int(n_out),
                                      scratch.data_ptr(), scratch.numel(), labels.data_ptr(), label_len.data_ptr(),
                                      scores.data_ptr(), n_beams.data_ptr(), stream), "ctc_beam_search")
    return labels, label_len, scores, n_beams


def launch_nw(lib, ref, ref_len, hyp, hyp_len, d, m, r, normalize, stream=None):
    """cpc_nw_align_score on (B, L1) / (B, L2) int32 label rows (any row stride, unit element stride) -> (B,) float64."""
    for name, t in (("ref", ref), ("hyp", hyp)):
        if t.dim() != 2 or t.dtype != torch.int32 or t.stride(1) != 1:
            raise ValueError(f"seq_per_batch: {name} must be (B, L) int32 rows with unit element stride")
    for name, t in (("ref_len", ref_len), ("hyp_len", hyp_len)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.size(0) != ref.size(0) or not t.is_contiguous():
            raise ValueError(f"seq_per_batch: {name} must be a contiguous (B,) int32 tensor")
    B, L1 = ref.shape
    L2 = hyp.size(1)
    if hyp.size(0) != B:
        raise ValueError("seq_per_batch: ref and hyp batches differ")
    if L2 > MAX_HYP_LEN:
        raise ValueError(f"seq_per_batch: hypotheses longer than {MAX_HYP_LEN} labels are not supported")
    out = torch.empty(B, dtype=torch.float64, device=ref.device)
    if B == 0:
        return out
    if L1 == 0:                 # an empty row still needs an address
        ref = torch.zeros(B, 1, dtype=torch.int32, device=ref.device)
    if L2 == 0:
        hyp = torch.zeros(B, 1, dtype=torch.int32, device=hyp.device)
    lib.check(lib.cpc_nw_align_score(ref.data_ptr(), max(ref.stride(0), L1), ref_len.data_ptr(), L1, hyp.data_ptr(),
                                     max(hyp.stride(0), L2), hyp_len.data_ptr(), L2, B, float(d), float(m), float(r),
                                     int(bool(normalize)), out.data_ptr(), stream), "nw_align_score")
    return out


# --------------------------------------------------------------------------- batched device API
def beam_search_batch(probs, lengths, n_keep, blank, n_out=1):
    """beam_search on every sequence of a batch in one launch.  probs: (B, T, P) float32 / float64 probabilities on the GPU
    (any strides); lengths: (B,) frames per sequence, each in [1, T].  -> device tensors (labels (B, n_out, T) int32 padded
    with -1, label_len (B, n_out) int32, scores (B, n_out), n_beams (B) int32), beams in the reference's ranked order."""
    if not probs.is_cuda:
        raise RuntimeError("beam_search_batch: expected probabilities on an AMD GPU; this package has no CPU path")
    lengths = torch.as_tensor(lengths).to(probs.device, torch.int32).contiguous()
    return launch_beam_search(_lib.get(), probs, lengths, n_keep, blank, n_out, _stream(probs))


def seq_per_batch(ref, ref_len, hyp, hyp_len, d=-1, m=-1, r=0, normalize=True):
    """NeedlemanWunschAlignScore(ref[b, :ref_len[b]], hyp[b, :hyp_len[b]], d, m, r, normalize) for every b, on the GPU ->
    (B,) float64 device tensor (get_seq_PER with the defaults).  An empty reference gives NaN when normalised.  hyp may be
    beam_search_batch's labels[:, 0] and label_len[:, 0] directly."""
    if not ref.is_cuda:
        raise RuntimeError("seq_per_batch: expected labels on an AMD GPU; this package has no CPU path")
    dev = ref.device
    ref = ref.to(dev, torch.int32)
    hyp = hyp.to(dev, torch.int32)
    ref = ref if ref.stride(-1) == 1 else ref.contiguous()
    hyp = hyp if hyp.stride(-1) == 1 else hyp.contiguous()
    ref_len = torch.as_tensor(ref_len).to(dev, torch.int32).contiguous()
    hyp_len = torch.as_tensor(hyp_len).to(dev, torch.int32).contiguous()
    return launch_nw(_lib.get(), ref, ref_len, hyp, hyp_len, d, m, r, normalize, _stream(ref))


# --------------------------------------------------------------------------- the reference's API
def _as_table(score_preds):
    if isinstance(score_preds, torch.Tensor):
        t = score_preds.detach()
        dtype = torch.float32 if t.dtype == torch.float32 else torch.float64
        return t.to(dtype), (np.float32 if dtype == torch.float32 else np.float64)
    a = np.asarray(score_preds)
    dtype = np.float32 if a.dtype == np.float32 else np.float64
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)), dtype


def beam_search(score_preds, nKeep, blankLabel):
    """seq_alignment.py:11-61: the CTC prefix beam search of one (T, P) table of probabilities -> the last step's kept list
    [(score, labels)], best first, min(nKeep, candidates) entries; scores are numpy scalars of the input's dtype."""
    table, np_dtype = _as_table(score_preds)
    if table.dim() != 2:
        raise ValueError(f"beam_search: a (T, P) table expected, got shape {tuple(table.shape)}")
    T, P = table.shape
    if T == 0:
        raise ValueError("beam_search: the table has no frames")
    check_limits(P, nKeep)
    if not 0 <= blankLabel < P:
        raise ValueError(f"beam_search: blankLabel {blankLabel} outside [0, {P})")
    dev = _device()
    labels, label_len, scores, n_beams = beam_search_batch(table.to(dev).unsqueeze(0), torch.tensor([T], dtype=torch.int32),
                                                           nKeep, blankLabel, n_out=nKeep)
    n = int(n_beams[0].item())
    labels, label_len, scores = labels[0, :n].cpu().numpy(), label_len[0, :n].cpu().numpy(), scores[0, :n].cpu().numpy()
    return [(np_dtype(scores[k]), [int(x) for x in labels[k, :label_len[k]]]) for k in range(n)]


def collapseLabelChain(inputLabels):
    """seq_alignment.py:64-86: (N, T) frame labels -> ((N, maxSize) int64 collapsed labels padded with 0, (N,) int64 sizes)."""
    from .criterion import collapse_label_chain
    labels = torch.as_tensor(inputLabels)
    N = labels.size(0)
    flat, sizes = collapse_label_chain(labels)
    sizes = sizes.to(torch.int64)
    max_size = int(sizes.max().item()) if N else 0
    out = torch.zeros(N, max_size, device=labels.device, dtype=torch.int64)
    mask = torch.arange(max_size, device=labels.device).unsqueeze(0) < sizes.unsqueeze(1)
    out[mask] = flat.to(torch.int64)
    return out, sizes


def _labels(seq):
    if isinstance(seq, torch.Tensor):
        seq = seq.detach().cpu().numpy()
    return np.asarray(seq, dtype=np.int64).reshape(-1)


def NeedlemanWunschAlignScore(seq1, seq2, d, m, r, normalize=True):
    """seq_alignment.py:89-113 on the GPU: -(the max-plus alignment score of seq1 against seq2), divided by len(seq1) when
    normalize.  Integer d, m, r without normalisation give an int, as the reference's arithmetic does."""
    a, b = _labels(seq1), _labels(seq2)
    if normalize and a.size == 0:
        raise ZeroDivisionError("float division by zero")
    dev = _device()
    ref = torch.from_numpy(a.astype(np.int32)).view(1, -1).to(dev)
    hyp = torch.from_numpy(b.astype(np.int32)).view(1, -1).to(dev)
    out = seq_per_batch(ref, [a.size], hyp, [b.size], d, m, r, normalize)
    v = float(out[0].item())
    if not normalize and all(isinstance(x, (int, np.integer)) for x in (d, m, r)):
        return int(v)
    return v


def get_seq_PER(seqLabels, detectedLabels):
    return NeedlemanWunschAlignScore(seqLabels, detectedLabels, -1, -1, 0, normalize=True)


def getPER(dataLoader, featureMaker, blankLabel):
    """seq_alignment.py:116-158: the mean PER over a loader of (data, frame labels) batches; featureMaker(data) gives
    (N, S, P) probabilities.  Beams of 100, decoded and aligned per batch on the GPU; the sum is taken in float64 in order."""
    n_keep = 100
    out, n_items = 0.0, 0
    for data in dataLoader:
        with torch.no_grad():
            output = featureMaker(data)
        dev = output.device if output.is_cuda else _device()
        output = output.detach().to(dev)
        if output.dtype != torch.float32:
            output = output.to(torch.float64)
        labels, target_size = collapseLabelChain(data[1])
        N, S, _ = output.shape
        lab, lab_len, _, _ = beam_search_batch(output, torch.full((N,), S, dtype=torch.int32), n_keep, blankLabel)
        per = seq_per_batch(labels.to(dev), target_size, lab[:, 0], lab_len[:, 0])
        out += float(per.sum().item())
        n_items += N
    return out / n_items
