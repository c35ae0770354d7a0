"""ABX discrimination error within and across speakers -- the reference's cpc/eval/ABX.py and cpc/eval/ABX/{abx_iterators,
abx_group_computation}.py, scored on the HIP kernels of csrc/abx.hip.

The host side keeps the reference's API: item files, the (context, speaker, phone) grouping, ABXFeatureLoader and its two
iterators.  Scoring does not go through the iterators: a planner walks the same loops, draws the same random samples in the
same order, and emits a flat plan (member segment ids of A, B and X per group and the group's board coordinates).  One launch
pair per chunk of groups then computes every DTW distance and every group's 1 - theta on the GPU, straight from the loader's
packed frames, and the sparse means of ABX.py are taken in float64 in a fixed order.  There is no CPU path.

    python -m cpc_audio_amd.abx from_checkpoint CHECKPOINT ITEM_FILE DATASET_DIR [--seq_norm ...]
    python -m cpc_audio_amd.abx from_pre_computed FEATURE_DIR ITEM_FILE [--file_extension .pt|.npy ...]
"""
import argparse
import ctypes
import json
import math
import random
import sys
from pathlib import Path

import numpy as np
import torch

from . import _lib, ops

MAX_SEGMENT_FRAMES = 1024      # cpc_abx_layout sizes[1]
MAX_DIM = 1024
_CHUNK_PAIRS = 1 << 25         # pair distances (floats) of one scoring launch


# --------------------------------------------------------------------------- features and items (abx_iterators.py)
def normalize_with_singularity(x):
    """(N, S, H) -> (N, S, H + 1): unit frames with a trailing 1e-12; a null frame becomes 1/sqrt(H) everywhere with a
    trailing -2e12, which puts it at cosine distance 1 from every non-null frame and 0 from another null frame.
    (The reference also normalises ``x`` in place; this returns a new tensor and leaves ``x`` alone.)"""
    N, S, H = x.size()
    norm_x = (x ** 2).sum(dim=2, keepdim=True)
    y = x / torch.sqrt(norm_x)
    zero = (norm_x == 0).view(N, S)
    y[zero] = 1 / math.sqrt(H)
    border = torch.zeros((N, S, 1), dtype=x.dtype, device=x.device) + 1e-12
    border[zero] = -2 * 1e12
    return torch.cat([y, border], dim=2)


def load_item_file(path_item_file):
    """-> (files_data, context_match, phone_match, speaker_match).  files_data[file] = [[onset, offset, context, phone,
    speaker], ...]; ids in first-seen order; the context is 'prev+next'; the header line is skipped."""
    with open(path_item_file, "r") as f:
        lines = f.read().splitlines()[1:]
    out, context_match, phone_match, speaker_match = {}, {}, {}, {}
    for line in lines:
        items = line.split()
        if len(items) != 7:
            raise ValueError(f"{path_item_file}: item line needs 7 fields: {line!r}")
        file_id, onset, offset, phone, prev, nxt, speaker = items
        ctx = f"{prev}+{nxt}"
        pid = phone_match.setdefault(phone, len(phone_match))
        cid = context_match.setdefault(ctx, len(context_match))
        sid = speaker_match.setdefault(speaker, len(speaker_match))
        out.setdefault(file_id, []).append([float(onset), float(offset), cid, pid, sid])
    return out, context_match, phone_match, speaker_match


def get_features_group(in_data, index_order):
    """Sort the rows of ``in_data`` by the columns ``index_order`` (stable) and nest the runs: -> (sorted row indices,
    groups), where groups has len(index_order) - 1 levels of lists around (start, end) ranges of the sorted order."""
    order = sorted(range(len(in_data)), key=lambda i: [in_data[i][k] for k in index_order])
    keys = [[in_data[i][k] for k in index_order] for i in order]

    def split(lo, hi, level):
        runs, s = [], lo
        for i in range(lo + 1, hi + 1):
            if i == hi or keys[i][level] != keys[s][level]:
                runs.append((s, i))
                s = i
        if level == len(index_order) - 1:
            return runs
        return [split(a, b, level + 1) for a, b in runs]

    return order, split(0, len(order), 0)


class ABXFeatureLoader:
    """Segments of an item file cut out of per-file features.  ``features[i] = [first row in data, frames, context, phone,
    speaker]``; ``data`` holds every segment's frames packed (rows, feature_dim) -- the device layout of the scorer."""
    INDEX_CONTEXT, INDEX_PHONE, INDEX_SPEAKER = 2, 3, 4

    def __init__(self, path_item_file, seqList, featureMaker, stepFeature, normalize):
        files_data, self.context_match, self.phone_match, self.speaker_match = load_item_file(path_item_file)
        self.seqNorm = True
        self.stepFeature = stepFeature
        self.loadFromFileData(files_data, seqList, featureMaker, normalize)

    def loadFromFileData(self, files_data, seqList, feature_maker, normalize):
        self.features, data, total = [], [], 0
        for file_id, file_path in seqList:
            if file_id not in files_data:
                continue
            feats = feature_maker(file_path)
            if normalize:
                feats = normalize_with_singularity(feats)
            feats = feats.detach().cpu()
            feats = feats.view(feats.size(1), feats.size(2))
            T = feats.size(0)
            for onset, offset, cid, pid, sid in files_data[file_id]:
                i0 = max(0, int(math.ceil(self.stepFeature * onset - 0.5)))
                i1 = min(T, int(math.floor(self.stepFeature * offset - 0.5)))
                if i0 >= T or i1 <= i0:
                    continue
                self.features.append([total, i1 - i0, cid, pid, sid])
                data.append(feats[i0:i1])
                total += i1 - i0
        self.data = torch.cat(data, dim=0)
        self.feature_dim = self.data.size(1)

    def get_data_device(self):
        return self.data.device

    def cuda(self):
        self.data = self.data.cuda()

    def cpu(self):
        self.data = self.data.cpu()

    def get_ids(self, index):
        return tuple(self.features[index][2:])

    def __getitem__(self, index):
        start, size, cid, pid, sid = self.features[index]
        return self.data[start:start + size], size, (cid, pid, sid)

    def __len__(self):
        return len(self.features)

    def get_n_speakers(self):
        return len(self.speaker_match)

    def get_n_context(self):
        return len(self.context_match)

    def get_n_phone(self):
        return len(self.phone_match)

    def get_iterator(self, mode, max_size_group):
        if mode == "within":
            return ABXWithinGroupIterator(self, max_size_group)
        if mode == "across":
            return ABXAcrossGroupIterator(self, max_size_group)
        raise ValueError(f"Invalid mode: {mode}")


# --------------------------------------------------------------------------- the reference's iterators (API and tests)
class ABXIterator:
    """Groups of (context, speaker, phone); yields padded (data, sizes) batches as the reference does.  The scorer uses
    plan_within / plan_across instead, which draw the same samples."""

    def __init__(self, abxDataset, max_size_group, rng=None):
        self.max_size_group = max_size_group
        self.dataset = abxDataset
        self.len = 0
        self.rng = random if rng is None else rng
        self.index_csp, self.groups_csp = get_features_group(
            abxDataset.features, [abxDataset.INDEX_CONTEXT, abxDataset.INDEX_SPEAKER, abxDataset.INDEX_PHONE])

    def sample(self, i_start, i_end):
        """Dataset indices of one group, sampled down to max_size_group exactly as the reference's get_group draws."""
        take = list(range(i_start, i_end))
        if i_end - i_start > self.max_size_group:
            take = self.rng.sample(take, k=self.max_size_group)
        return [self.index_csp[i] for i in take]

    def get_group(self, i_start, i_end):
        ids = self.sample(i_start, i_end)
        items = [self.dataset[i] for i in ids]
        dev = self.dataset.get_data_device()
        max_size = max(s for _, s, _ in items)
        out = torch.zeros(len(ids), max_size, self.dataset.feature_dim, device=dev)
        sizes = torch.zeros(len(ids), dtype=torch.long, device=dev)
        for k, (d, s, _) in enumerate(items):
            out[k, :s] = d
            sizes[k] = s
        return out, sizes, items[-1][2]

    def __len__(self):
        return self.len


class ABXWithinGroupIterator(ABXIterator):
    def __init__(self, abxDataset, max_size_group, rng=None):
        super().__init__(abxDataset, max_size_group, rng)
        self.symmetric = True
        for context_group in self.groups_csp:
            for speaker_group in context_group:
                if len(speaker_group) > 1:
                    self.len += sum(len(speaker_group) - 1 for a, b in speaker_group if b - a > 1)

    def triplets(self):
        """(coords, A range, B range) in the reference's order (X is A)."""
        for context_group in self.groups_csp:
            for speaker_group in context_group:
                if len(speaker_group) == 1:
                    continue
                for i_a, ra in enumerate(speaker_group):
                    if ra[1] - ra[0] == 1:
                        continue
                    for i_b, rb in enumerate(speaker_group):
                        if i_b != i_a:
                            yield ra, rb

    def __iter__(self):
        for ra, rb in self.triplets():
            data_b, size_b, id_b = self.get_group(*rb)
            data_a, size_a, id_a = self.get_group(*ra)
            yield (id_a[2], id_a[1], id_b[1], id_a[0]), (data_a, size_a), (data_b, size_b), (data_a, size_a)

    def get_board_size(self):
        d = self.dataset
        return (d.get_n_speakers(), d.get_n_phone(), d.get_n_phone(), d.get_n_context())


class ABXAcrossGroupIterator(ABXIterator):
    def __init__(self, abxDataset, max_size_group, rng=None):
        super().__init__(abxDataset, max_size_group, rng)
        self.symmetric = False
        self.max_x = 5
        self.get_speakers_from_cp = {}
        for context_group in self.groups_csp:
            for speaker_group in context_group:
                for rng_ in speaker_group:
                    c, p, s = self.dataset.get_ids(self.index_csp[rng_[0]])
                    self.get_speakers_from_cp.setdefault(c, {}).setdefault(p, {})[s] = rng_
        for context_group in self.groups_csp:
            for speaker_group in context_group:
                if len(speaker_group) > 1:
                    for rng_ in speaker_group:
                        c, p, _ = self.dataset.get_ids(self.index_csp[rng_[0]])
                        self.len += (len(speaker_group) - 1) * min(self.max_x, len(self.get_speakers_from_cp[c][p]) - 1)

    def get_other_speakers_in_group(self, i_start_group):
        c, p, s = self.dataset.get_ids(self.index_csp[i_start_group])
        return [v for k, v in self.get_speakers_from_cp[c][p].items() if k != s]

    def triplets(self):
        """(A range, B range, X range) in the reference's order, drawing the X speakers as it does."""
        for context_group in self.groups_csp:
            for speaker_group in context_group:
                if len(speaker_group) == 1:
                    continue
                for i_a, ra in enumerate(speaker_group):
                    ref = self.get_other_speakers_in_group(ra[0])
                    xs = self.rng.sample(ref, k=self.max_x) if len(ref) > self.max_x else ref
                    for rx in xs:
                        for i_b, rb in enumerate(speaker_group):
                            if i_b != i_a:
                                yield ra, rb, rx

    def get_abx_triplet(self, i_a, i_b, i_x):
        data_a, size_a, id_a = self.get_group(*i_a)
        data_b, size_b, id_b = self.get_group(*i_b)
        data_x, size_x, id_x = self.get_group(*i_x)
        return (id_a[2], id_a[1], id_b[1], id_a[0], id_x[2]), (data_a, size_a), (data_b, size_b), (data_x, size_x)

    def __iter__(self):
        for ra, rb, rx in self.triplets():
            yield self.get_abx_triplet(ra, rb, rx)

    def get_board_size(self):
        d = self.dataset
        return (d.get_n_speakers(), d.get_n_phone(), d.get_n_phone(), d.get_n_context(), d.get_n_speakers())


# --------------------------------------------------------------------------- planner
class Plan:
    """A pass as the device sees it: per group the member dataset indices of A, B and X (after sampling) and the group's
    board coordinates -- (speaker, phone_a, phone_b, context) within, + speaker_x across."""

    def __init__(self, mode, symmetric, board, coords, a, b, x):
        self.mode, self.symmetric, self.board = mode, symmetric, tuple(board)
        self.coords = np.asarray(coords, dtype=np.int64).reshape(-1, len(board))
        self.a, self.b, self.x = a, b, x            # lists of lists of dataset indices

    def __len__(self):
        return len(self.a)


def _rng(seed):
    """None: the global random module (the reference's draws); an int: a private random.Random(seed); a Random: itself."""
    if seed is None or isinstance(seed, random.Random):
        return seed
    return random.Random(seed)


def plan_within(dataset, max_size_group, seed=None):
    """The within pass: for each (A, B), B is drawn first and then A (A again for every B), as the reference iterates."""
    it = ABXWithinGroupIterator(dataset, max_size_group, _rng(seed))
    coords, A, B = [], [], []
    for ra, rb in it.triplets():
        b = it.sample(*rb)
        a = it.sample(*ra)
        ca, pa, s = dataset.get_ids(a[-1])
        coords.append((s, pa, dataset.get_ids(b[-1])[1], ca))
        A.append(a)
        B.append(b)
    return Plan("within", True, it.get_board_size(), coords, A, B, A)


def plan_across(dataset, max_size_group, max_x=5, seed=None):
    """The across pass: per A the X speakers are drawn, then per triplet A, B and X in that order."""
    it = ABXAcrossGroupIterator(dataset, max_size_group, _rng(seed))
    it.max_x = max_x
    coords, A, B, X = [], [], [], []
    for ra, rb, rx in it.triplets():
        a = it.sample(*ra)
        b = it.sample(*rb)
        x = it.sample(*rx)
        ca, pa, sa = dataset.get_ids(a[-1])
        coords.append((sa, pa, dataset.get_ids(b[-1])[1], ca, dataset.get_ids(x[-1])[2]))
        A.append(a)
        B.append(b)
        X.append(x)
    return Plan("across", False, it.get_board_size(), coords, A, B, X)


# --------------------------------------------------------------------------- reduction (ABX.py)
def reduce_scores(plan, scores):
    """Group scores (1 - theta) -> the pass's ABX error: per (speaker, phone_a, phone_b) the mean over the remaining board
    axes (context; context and speaker_x across), then the mean over speakers with data, then over phone pairs with data.
    float64, in plan order: the same bits for the same inputs."""
    scores = np.asarray(scores, dtype=np.float64)
    S, P = plan.board[0], plan.board[1]
    c = plan.coords
    lin = (c[:, 0] * P + c[:, 1]) * P + c[:, 2]
    total = np.bincount(lin, weights=scores, minlength=S * P * P)
    count = np.bincount(lin, minlength=S * P * P).astype(np.float64)
    group = (total / (1e-08 * (count == 0) + count)).reshape(S, P, P)
    spk = (count > 0).reshape(S, P, P).sum(axis=0).astype(np.float64)
    phone = group.sum(axis=0) / (1e-08 * (spk == 0) + spk)
    return float(phone.sum() / (spk > 0).sum())


# --------------------------------------------------------------------------- distances (abx_group_computation.py)
def get_cosine_distance_batch(a1, a2, epsilon=1e-8):
    """(N1, S1, D) x (N2, S2, D) -> (N1, N2, S1, S2) acos(<x, y>) / pi; a1 and a2 must be normalised."""
    N1, S1, D = a1.size()
    N2, S2, _ = a2.size()
    prod = (a1.view(N1, 1, S1, 1, D) * a2.view(1, N2, 1, S2, D)).sum(dim=4)
    return torch.clamp(prod, -1, 1).acos() / math.pi


def get_euclidian_distance_batch(a1, a2):
    N1, S1, D = a1.size()
    N2, S2, _ = a2.size()
    diff = a1.view(N1, 1, S1, 1, D) - a2.view(1, N2, 1, S2, D)
    return torch.sqrt((diff ** 2).sum(dim=4))


def get_distance_function_from_name(name_str):
    if name_str == "euclidian":
        return get_euclidian_distance_batch
    if name_str == "cosine":
        return get_cosine_distance_batch
    raise ValueError("Invalid distance mode")


def _metric(distance_function):
    if distance_function is get_cosine_distance_batch:
        return 0
    if distance_function is get_euclidian_distance_batch:
        return 1
    return None


def _require_gpu(what):
    if not torch.cuda.is_available():
        ops._require_cuda(torch.empty(0), what)      # raises: no CPU path


# --------------------------------------------------------------------------- device scoring
class _Segments:
    """Packed frames (rows, D) on the device with per-segment (offset, length) int32."""

    def __init__(self, data, starts, sizes):
        data = data.detach()
        if data.dim() != 2 or data.size(1) > MAX_DIM or data.size(1) < 1:
            raise ValueError(f"ABX: features must be (frames, D) with 1 <= D <= {MAX_DIM}, got {tuple(data.shape)}")
        sizes = np.asarray(sizes, dtype=np.int64)
        starts = np.asarray(starts, dtype=np.int64)
        if sizes.size == 0 or sizes.min() < 1 or sizes.max() > MAX_SEGMENT_FRAMES:
            raise ValueError(f"ABX: every segment needs 1 .. {MAX_SEGMENT_FRAMES} frames")
        if starts.min() < 0 or (starts + sizes).max() > data.size(0):
            raise ValueError("ABX: a segment lies outside the frames")
        dev = torch.device("cuda", torch.cuda.current_device())
        self.feat = data.to(dev, torch.float32).contiguous()
        self.off = torch.from_numpy(starts.astype(np.int32)).to(dev)
        self.len = torch.from_numpy(sizes.astype(np.int32)).to(dev)
        self.n, self.D, self.max_len = int(sizes.size), int(data.size(1)), int(sizes.max())

    def args(self, metric):
        return (_lib.ptr(self.feat), _lib.ptr(self.off), _lib.ptr(self.len), self.n, self.feat.size(0), self.D,
                self.max_len, metric)


def _plan_arrays(A, B, X):
    na = np.fromiter((len(v) for v in A), np.int64, len(A))
    nb = np.fromiter((len(v) for v in B), np.int64, len(B))
    nx = np.fromiter((len(v) for v in X), np.int64, len(X))
    members = np.fromiter((m for a, b, x in zip(A, B, X) for m in (*a, *b, *x)), np.int64)
    return na, nb, nx, members


def score_groups(segs, A, B, X, symmetric, metric, with_dist=False, events=None):
    """Per group 1 - theta on the device (cpc_abx_group_scores), in chunks of at most _CHUNK_PAIRS pair distances.  A, B, X:
    lists of segment-id lists.  -> float32 CPU scores (and, with_dist, each group's (dxa, dxb) as CPU tensors).  ``events``:
    a list that receives a (start, end) pair of timing events around each launch."""
    lib = _lib.get()
    na, nb, nx, members = _plan_arrays(A, B, X)
    G = len(na)
    if members.size and (members.min() < 0 or members.max() >= segs.n):
        raise ValueError(f"ABX plan: a member id lies outside [0, {segs.n})")
    if G and (na.min() < 1 or nb.min() < 1 or nx.min() < 1):
        raise ValueError("ABX plan: every group needs at least one A, B and X member")
    if symmetric and np.any(na != nx):
        raise ValueError("ABX plan: the symmetric (within) pass needs X = A")
    if G and (nx * na * nb).max() >= 2 ** 31:
        raise ValueError("ABX plan: a group is too large")
    pairs = nx * (na + nb)
    first = np.concatenate([[0], np.cumsum(na + nb + nx)[:-1]]).astype(np.int64)
    dev = segs.feat.device
    stream = ops._stream()
    scores = torch.empty(G, dtype=torch.float32, device=dev)
    mem_d = torch.from_numpy(members.astype(np.int32)).to(dev)
    dists = []
    g0 = 0
    while g0 < G:
        cum = np.cumsum(pairs[g0:])
        g1 = g0 + max(1, int(np.searchsorted(cum, _CHUNK_PAIRS, side="right")))
        base = np.concatenate([[0], cum[:g1 - g0 - 1]]).astype(np.int64)
        n_pairs = int(cum[g1 - g0 - 1])
        groups = np.stack([first[g0:g1], na[g0:g1], nb[g0:g1], nx[g0:g1]], axis=1).astype(np.int32)
        gid = np.repeat(np.arange(g1 - g0), nx[g0:g1])
        xid = np.arange(gid.size) - np.repeat(np.cumsum(nx[g0:g1]) - nx[g0:g1], nx[g0:g1])
        work = np.stack([gid, xid], axis=1).astype(np.int32)
        sizes = (ctypes.c_long * 4)()
        lib.check(lib.cpc_abx_layout(segs.D, segs.max_len, g1 - g0, n_pairs, sizes), "abx_layout")
        dist = torch.empty(int(sizes[0]), dtype=torch.float32, device=dev)
        groups_d = torch.from_numpy(groups).to(dev)
        base_d = torch.from_numpy(base).to(dev)
        work_d = torch.from_numpy(work).to(dev)
        if events is not None:
            events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            events[-1][0].record()
        lib.check(lib.cpc_abx_group_scores(*segs.args(metric), _lib.ptr(mem_d), _lib.ptr(groups_d), _lib.ptr(base_d), g1 - g0,
                                           _lib.ptr(work_d), work.shape[0], int(symmetric), _lib.ptr(dist),
                                           _lib.ptr(scores[g0:g1]), stream), "abx_group_scores")
        if events is not None:
            events[-1][1].record()
        if with_dist:
            host = dist.cpu()
            for k in range(g1 - g0):
                o, x, a, b = int(base[k]), int(nx[g0 + k]), int(na[g0 + k]), int(nb[g0 + k])
                dists.append((host[o:o + x * a].view(x, a).clone(), host[o + x * a:o + x * (a + b)].view(x, b).clone()))
        g0 = g1
    return (scores.cpu(), dists) if with_dist else scores.cpu()


def score_plan(dataset, plan, metric):
    """Device group scores of a plan over an ABXFeatureLoader."""
    feats = np.asarray(dataset.features, dtype=np.int64).reshape(-1, 5)
    segs = _Segments(dataset.data, feats[:, 0], feats[:, 1])
    return score_groups(segs, plan.a, plan.b, plan.x, plan.symmetric, metric)


def ABX(feature_function, path_item_file, seq_list, distance_mode, step_feature, modes, seq_norm=True, cuda=False,
        max_x_across=5, max_size_group=30, seed=None):
    """-> {'within': error, 'across': error} for the requested modes.  Scores on the current GPU whatever ``cuda`` says
    (kept for the reference's signature).  seed=None draws from the global ``random`` module as the reference does; an int
    uses a private random.Random(seed) (the within pass first, then the across pass, from one generator)."""
    _require_gpu("abx.ABX")
    dataset = ABXFeatureLoader(path_item_file, seq_list, feature_function, step_feature, True)
    metric = _metric(get_distance_function_from_name(distance_mode))
    rng = _rng(seed)                           # one generator for both passes, as the global one is
    scores = {}
    if "within" in modes:
        plan = plan_within(dataset, max_size_group, rng)
        scores["within"] = reduce_scores(plan, score_plan(dataset, plan, metric).numpy())
    if "across" in modes:
        plan = plan_across(dataset, max_size_group, max_x_across, rng)
        scores["across"] = reduce_scores(plan, score_plan(dataset, plan, metric).numpy())
    return scores


# --------------------------------------------------------------------------- the reference's pair API
def _pack(*batches):
    """Padded (N, S, D) batches with sizes -> one _Segments holding every batch's valid frames, and each batch's first id."""
    rows, starts, lens, firsts, total = [], [], [], [], 0
    for data, sizes in batches:
        sizes = [int(v) for v in torch.as_tensor(sizes).reshape(-1).tolist()]
        if len(sizes) != data.size(0) or any(v < 1 or v > data.size(1) for v in sizes):
            raise ValueError("ABX: sizes must be 1 .. S for each of the N sequences")
        firsts.append(len(lens))
        for k, v in enumerate(sizes):
            rows.append(data[k, :v])
            starts.append(total)
            lens.append(v)
            total += v
    return _Segments(torch.cat(rows, dim=0), starts, lens), firsts


def _dtw_batch_pairs(N1, N2, ignore_diag, symmetric):
    return [(i, j) for i in range(N1) for j in range(i if symmetric else 0, N2) if not (ignore_diag and i == j)]


def get_distance_group_dtw(a1, a2, size1, size2, ignore_diag=False, symmetric=False,
                           distance_function=get_cosine_distance_batch):
    """(N1, N2) normalised DTW distances between the sequences of a1 (rows) and a2 (columns), as dtw_batch: with
    ``symmetric`` only j >= i is computed and mirrored, with ``ignore_diag`` the diagonal stays 0.  Built-in metrics run
    cpc_abx_pair_dtw on the frames; any other ``distance_function`` is evaluated with torch and only the DTW runs on the
    device (cpc_abx_dtw).  Returns a float32 CPU tensor."""
    _require_gpu("abx.get_distance_group_dtw")
    N1, N2 = a1.size(0), a2.size(0)
    if size1.size(0) != N1 or size2.size(0) != N2:
        raise ValueError("ABX: one size per sequence expected")
    lib, stream = _lib.get(), ops._stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    metric = _metric(distance_function)
    if metric is None:
        dist = distance_function(a1.to(dev), a2.to(dev)).detach().to(torch.float32).contiguous()
        s1 = torch.as_tensor(size1).to(dev, torch.int32)
        s2 = torch.as_tensor(size2).to(dev, torch.int32)
        out = torch.empty(N1, N2, dtype=torch.float32, device=dev)
        lib.check(lib.cpc_abx_dtw(_lib.ptr(dist), _lib.ptr(s1), _lib.ptr(s2), N1, N2, dist.size(2), dist.size(3),
                                  int(ignore_diag), int(symmetric), _lib.ptr(out), stream), "abx_dtw")
        return out.cpu()
    segs, (f1, f2) = _pack((a1, size1), (a2, size2))
    pairs = _dtw_batch_pairs(N1, N2, ignore_diag, symmetric)
    out = torch.zeros(N1, N2, dtype=torch.float32)
    if not pairs:
        return out
    ids = torch.tensor([(f1 + i, f2 + j) for i, j in pairs], dtype=torch.int32, device=dev)
    res = torch.empty(len(pairs), dtype=torch.float32, device=dev)
    lib.check(lib.cpc_abx_pair_dtw(*segs.args(metric), _lib.ptr(ids), len(pairs), _lib.ptr(res), stream), "abx_pair_dtw")
    res = res.cpu()
    for (i, j), v in zip(pairs, res.tolist()):
        out[i, j] = v
        if symmetric and i != j:
            out[j, i] = v
    return out


def theta_from_distances(dxa, dxb, symmetric):
    """theta of get_theta_group_dtw from (Nx, Na) / (Nx, Nb) DTW distances, with the reference's float32 rounding."""
    dxa = dxa.clone()
    Nx, Na = dxa.size()
    Nb = dxb.size(1)
    if symmetric:
        n_pos = Na * (Na - 1)
        max_val = dxb.max().item()
        for i in range(Na):
            dxa[i, i] = max_val + 1
    else:
        n_pos = Na * Nx
    dxb = dxb.view(Nx, 1, Nb).expand(Nx, Na, Nb)
    dxa = dxa.view(Nx, Na, 1).expand(Nx, Na, Nb)
    sc = (dxa < dxb).sum() + 0.5 * (dxa == dxb).sum()
    sc /= (n_pos * Nb)
    return sc.item()


def get_theta_group_dtw(a, b, x, sa, sb, sx, distance_function, symmetric):
    """theta of one (A, B, X) group.  Built-in metrics: one group through cpc_abx_group_scores (its dxa / dxb); otherwise
    get_distance_group_dtw with the torch distance."""
    if not (a.dim() == b.dim() == x.dim() == 3 and a.size(2) == b.size(2) == x.size(2)):
        raise ValueError("ABX: a, b and x must be (N, S, D) with one D")
    metric = _metric(distance_function)
    if metric is None:
        dxb = get_distance_group_dtw(x, b, sx, sb, distance_function=distance_function)
        dxa = get_distance_group_dtw(x, a, sx, sa, ignore_diag=symmetric, symmetric=symmetric,
                                     distance_function=distance_function)
        return theta_from_distances(dxa, dxb, symmetric)
    _require_gpu("abx.get_theta_group_dtw")
    segs, (fa, fb, fx) = _pack((a, sa), (b, sb), (x, sx))
    A = [list(range(fa, fa + a.size(0)))]
    B = [list(range(fb, fb + b.size(0)))]
    X = [list(range(fx, fx + x.size(0)))]
    _, dists = score_groups(segs, A, B, X, symmetric, metric, with_dist=True)
    return theta_from_distances(dists[0][0], dists[0][1], symmetric)


# --------------------------------------------------------------------------- command line (ABX.py)
def _base_args(parser):
    parser.add_argument("--debug", action="store_true")
    parser.add_argument("--feature_size", type=float, default=0.01, help="Size (in s) of one feature")
    parser.add_argument("--cuda", action="store_true", help="Accepted for compatibility: scoring always runs on the GPU")
    parser.add_argument("--mode", type=str, default="all", choices=["all", "within", "across"])
    parser.add_argument("--max_size_group", type=int, default=10)
    parser.add_argument("--max_x_across", type=int, default=5)
    parser.add_argument("--out", type=str, default=None, help="Directory of ABX_scores.json / ABX_args.json")
    parser.add_argument("--distance_mode", type=str, default="cosine", choices=["cosine", "euclidian"])
    parser.add_argument("--seed", type=int, default=None, help="Private random seed of the group sampling")


def parse_args(argv):
    parser = argparse.ArgumentParser(description="ABX metric")
    sub = parser.add_subparsers(dest="load")
    p = sub.add_parser("from_checkpoint")
    _base_args(p)
    p.add_argument("path_checkpoint", type=str)
    p.add_argument("path_item_file", type=str)
    p.add_argument("path_dataset", type=str)
    p.add_argument("--seq_norm", action="store_true")
    p.add_argument("--max_size_seq", default=64000, type=int)
    p.add_argument("--strict", action="store_true")
    p.add_argument("--file_extension", type=str, default=".wav")
    p.add_argument("--get_encoded", action="store_true")
    p.add_argument("--encoderKernel", action="store_true", default=argparse.SUPPRESS,
                   help="The convolutional encoder on the HIP kernels at every width from 2 to 512 and under every normMode the checkpoint "
                        "was trained with (off by default: 256 channels under layerNorm only, everything else on torch ops).")
    p = sub.add_parser("from_pre_computed")
    _base_args(p)
    p.add_argument("path_features", type=str, help="Directory of pre-computed (1, frames, D) features (.pt or .npy)")
    p.add_argument("path_item_file", type=str)
    p.add_argument("--file_extension", type=str, default=".pt")
    return parser.parse_args(argv)


def _load_features(path):
    if str(path).endswith(".npy"):
        return torch.from_numpy(np.load(path))
    return torch.load(path, map_location="cpu")


def _checkpoint_feature_function(args):
    from . import dataset, harness, train
    ckpt = Path(args.path_checkpoint)
    with open(ckpt.parent / "checkpoint_args.json") as f:
        saved = json.load(f)
    model = train.build_model(hiddenEncoder=saved.get("hiddenEncoder", 256), hiddenGar=saved.get("hiddenGar", 256),
                              nLevelsGRU=saved.get("nLevelsGRU", 1), arMode=saved.get("arMode", "LSTM"),
                              reverse=saved.get("cpc_mode") == "reverse", sizeWindow=saved.get("sizeWindow", 20480),
                              abspos=saved.get("abspos", False), encoder_type=saved.get("encoder_type", "cpc"),
                              mfccKernel=True, normMode=saved.get("normMode", "layerNorm"),
                              encoderKernel=getattr(args, "encoderKernel", False))
    harness.load_checkpoint(str(ckpt), model)
    model.gAR.keepHidden = True
    maker = harness.FeatureModule(model, args.get_encoded).cuda().eval()

    def feature_function(path):
        wave = dataset.loadFile((0, path))[2].view(1, -1)
        return harness.build_feature(maker, wave, strict=args.strict, max_size_seq=args.max_size_seq, seq_norm=args.seq_norm)
    return feature_function


def main(argv):
    args = parse_args(argv)
    from .dataset import findAllSeqs
    if args.load == "from_checkpoint":
        feature_function, root = _checkpoint_feature_function(args), args.path_dataset
        out_dir = Path(args.path_checkpoint).parent if args.out is None else Path(args.out)
    elif args.load == "from_pre_computed":
        feature_function, root = _load_features, args.path_features
        out_dir = Path(args.path_features) if args.out is None else Path(args.out)
    else:
        raise SystemExit("choose from_checkpoint or from_pre_computed")
    modes = ["within", "across"] if args.mode == "all" else [args.mode]
    seqs, _ = findAllSeqs(root, extension=args.file_extension)
    seq_list = [(str(Path(x).stem), str(Path(root) / x)) for _, x in seqs]
    if args.debug:
        seq_list = seq_list[:1000]
    scores = ABX(feature_function, args.path_item_file, seq_list, args.distance_mode, 1 / args.feature_size, modes,
                 seq_norm=getattr(args, "seq_norm", False), cuda=True, max_x_across=args.max_x_across,
                 max_size_group=args.max_size_group, seed=args.seed)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "ABX_scores.json", "w") as f:
        json.dump(scores, f, indent=2)
    with open(out_dir / "ABX_args.json", "w") as f:
        json.dump(vars(args), f, indent=2)
    return scores


if __name__ == "__main__":
    main(sys.argv[1:])
