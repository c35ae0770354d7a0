"""Drop-in replacements for the hot-path classes of the reference's cpc/criterion/criterion.py.

Same class names (including the reference's spelling ``CPCUnsupersivedCriterion``,
exported at cpc/criterion/__init__.py:5-6), constructor signatures and state-dict keys
(``wPrediction.predictors.{k}.weight``).  forward/backward of the criterion run in the
fused InfoNCE kernels of libcpc_hip.so; negatives are never materialised.
"""
import math

import torch
import torch.nn as nn

import torch.nn.functional as F

from .ops import (NCE_WIDE_MAX, ClassifierXentFunction, CtcXentFunction, InfoNCEFunction, InfoNCEScoresFunction,
                  nce_wide_scores, prepare_negatives)

_HEAD_TILE = 16          # prediction heads per call of the score kernels (a wavefront's MFMA tile; ops.head_group walks more)


class _Stacked(torch.autograd.Function):
    """The buffer K equally shaped parameters are views of (one behind the other), as a differentiable function of them:
    its gradient is handed to them block by block."""

    @staticmethod
    def forward(ctx, flat, *parts):
        ctx.shape = tuple(parts[0].shape)
        ctx.set_materialize_grads(False)
        return flat.view_as(flat)

    @staticmethod
    def backward(ctx, g):
        n = len(ctx.needs_input_grad) - 1
        if g is None:
            return (None,) * (n + 1)
        g = g.reshape(n, *ctx.shape)
        return (None,) + tuple(g[k] if ctx.needs_input_grad[k + 1] else None for k in range(n))


def stacked_parameters(owner, key, params, shape=None):
    """``params``: K equally shaped parameters.  -> one tensor of shape ``shape`` (default (K, *p.shape)) holding them one
    behind the other, tied to them for autograd, WITHOUT a per-step ``torch.cat``: the parameters are kept as views of one
    buffer (cached on ``owner`` under ``key``; re-established whenever somebody gave them new storage, e.g. ``.to(device)``;
    in-place updates -- the optimiser, ``load_state_dict`` -- keep it)."""
    cache = owner.__dict__.setdefault("_stacked_cache", {})
    flat = cache.get(key)
    p0 = params[0]
    step = p0.numel() * p0.element_size()
    if (flat is None or flat.device != p0.device or flat.dtype != p0.dtype
            or any(p.data_ptr() != flat.data_ptr() + k * step for k, p in enumerate(params))):
        with torch.no_grad():
            flat = torch.stack([p.detach() for p in params]).contiguous()
            for k, p in enumerate(params):
                p.data = flat[k]
        cache[key] = flat
    out = flat if shape is None else flat.view(shape)
    return _Stacked.apply(out, *params)


# the 13 parameters of a TransformerLayer in the order of the C ABI (cpc_transformer_layer_forward)
_LAYER_PARAMS = (lambda l: l.multihead.Wo.weight, lambda l: l.multihead.Wk.weight, lambda l: l.multihead.Wq.weight,
                 lambda l: l.multihead.Wv.weight, lambda l: l.multihead.Att.Krelpos if l.multihead.Att.relpos else None,
                 lambda l: l.ln_multihead.weight, lambda l: l.ln_multihead.bias, lambda l: l.ffnetwork.lin1.weight,
                 lambda l: l.ffnetwork.lin1.bias, lambda l: l.ffnetwork.lin2.weight, lambda l: l.ffnetwork.lin2.bias,
                 lambda l: l.ln_ffnetwork.weight, lambda l: l.ln_ffnetwork.bias)


class _Equalized(nn.Module):
    """cpc/criterion/custom_layers.py:45-78 as the criterion uses it (``equalized=True``): the wrapped layer (parameter keys
    ``module.weight`` / ``module.bias``) starts from N(0, 1) weights and a zero bias, and its output is multiplied at run time by
    He's constant sqrt(2 / fan_in) (custom_layers.py:33-42), kept in the plain attribute ``weight`` as in the reference."""

    def __init__(self, module):
        super().__init__()
        self.module = module
        with torch.no_grad():
            module.weight.normal_(0, 1)
            if module.bias is not None:
                module.bias.zero_()
        self.equalized = True
        self.weight = math.sqrt(2.0 / module.weight[0].numel())

    def forward(self, x):
        return self.module(x) * self.weight


class FFNetwork(nn.Module):
    """cpc/criterion/criterion.py:11-20 (``--rnnMode ffd``): lin2(drop(relu(lin1 x))) on equalized linear layers."""

    def __init__(self, din, dout, dff, dropout):
        super().__init__()
        self.lin1 = _Equalized(nn.Linear(din, dff, bias=True))
        self.lin2 = _Equalized(nn.Linear(dff, dout, bias=True))
        self.relu = nn.ReLU()
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        return self.lin2(self.drop(self.relu(self.lin1(x))))


class ShiftedConv(nn.Module):
    """cpc/criterion/criterion.py:23-41 (``--rnnMode conv4 / conv8 / conv12``): a causal convolution over the time axis of a
    (N, S, C) sequence -- kernelSize - 1 zero frames in front, an equalized Conv1d, back to (N, S, C)."""

    def __init__(self, dimOutputAR, dimOutputEncoder, kernelSize):
        super().__init__()
        self.module = _Equalized(nn.Conv1d(dimOutputAR, dimOutputEncoder, kernelSize, padding=0))
        self.kernelSize = kernelSize

    def forward(self, x):
        y = nn.functional.pad(x.transpose(1, 2), (self.kernelSize - 1, 0))
        return self.module(y).transpose(1, 2)


_TORCH_PREDICTORS = {
    # criterion.py:63-81.  nn.RNN is built WITHOUT batch_first there (:64-65) and so walks the batch axis of the (B, W, C)
    # context as its time axis; kept, since a checkpoint trained that way means exactly that
    "RNN": lambda a, e: nn.RNN(a, e),
    "LSTM": lambda a, e: nn.LSTM(a, e, batch_first=True),
    "ffd": lambda a, e: FFNetwork(a, e, e, 0),
    "conv4": lambda a, e: ShiftedConv(a, e, 4),
    "conv8": lambda a, e: ShiftedConv(a, e, 8),
    "conv12": lambda a, e: ShiftedConv(a, e, 12),
}
# ... which run, with ``hipPredictors``, on HIP kernels where every predictor is of the class named here: the feed-forward ones as
# grouped causal convolutions on csrc/pred_conv.hip (ops.PredConvFunction), the recurrent ones as K recurrences side by side on
# csrc/lstm.hip (ops.LstmGroupFunction) and csrc/rnn.hip (ops.RnnFunction)
_HIP_PREDICTORS = {"ffd": FFNetwork, "conv4": ShiftedConv, "conv8": ShiftedConv, "conv12": ShiftedConv,
                   "LSTM": nn.LSTM, "RNN": nn.RNN}
_CELL_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


class PredictionNetwork(nn.Module):
    """cpc/criterion/criterion.py:44-118: K prediction networks.  ``--rnnMode linear`` (the ``else`` branch at
    :89-95, north-star configuration): K bias-free nn.Linear(dimOutputAR, dimOutputEncoder) fused into the
    criterion kernels; ``--rnnMode transformer`` (:82-88, BASELINE.json config 4): K one-layer transformers
    ``buildTransformerAR(dimOutputEncoder, 1, sizeInputSeq, False)`` on the HIP transformer layer
    (``transformerDropout`` is an addition -- the reference's layers always use 0.1, which has no parity).  The reference's
    other choices (:63-81: ``RNN``, ``LSTM``, ``ffd``, ``conv4/8/12``; none in a BASELINE config) are torch modules with the
    reference's parameter names whose predictions the HIP score kernels take as a tensor (``scores_apart``); with
    ``hipPredictors`` those predictions come from HIP kernels on the modules' parameters (``_hip_predictions``)."""

    def __init__(self, nPredicts, dimOutputAR, dimOutputEncoder, rnnMode=None, dropout=False,
                 sizeInputSeq=116, transformerDropout=0.1, hipPredictors=False):
        super().__init__()
        # hipPredictors (an addition; off by default): ``ffd`` and ``conv4/8/12`` predictors run on csrc/pred_conv.hip, ``LSTM`` and
        # ``RNN`` predictors on csrc/lstm.hip / csrc/rnn.hip where _hip_predictors_apply allows, on the torch modules otherwise;
        # last_path names what the last call took
        self.hipPredictors = bool(hipPredictors)
        self.last_path = None
        if dimOutputAR < 1 or dimOutputEncoder < 1:
            raise ValueError("PredictionNetwork: dimOutputAR and dimOutputEncoder must be positive")
        if dimOutputEncoder > NCE_WIDE_MAX:
            raise NotImplementedError(f"the HIP score kernels take hiddenEncoder up to {NCE_WIDE_MAX} (eight 64-channel blocks per "
                                      f"wavefront), got {dimOutputEncoder}")
        # 256 / 256 (north-star configuration): the linear heads fused into the criterion kernels of csrc/nce.hip.  Any other pair
        # of widths: the predictions are formed as a tensor (scores_apart) and scored by the width-parametric kernels of
        # csrc/nce_wide.hip (ops.nce_wide_scores)
        self.wide = dimOutputAR != 256 or dimOutputEncoder != 256
        self.dimOutputEncoder = dimOutputEncoder
        # (any number of prediction steps: the score tiles hold 16 heads per wavefront, a larger criterion is walked in groups of
        # 16 -- CPCUnsupersivedCriterion._forward_in_head_groups)
        self.predictors = nn.ModuleList()
        self.RESIDUAL_STD = 0.01
        self.dimOutputAR = dimOutputAR
        # criterion.py:59,113-114: nn.Dropout(p=0.5) on every head's prediction (``--dropout``).  While it is active (training
        # mode) the predictions are formed as a tensor of their own -- one library GEMM for the K linear heads, or the transformer
        # predictors -- dropped out by torch and scored by the same kernels the transformer predictors use (scores_apart below);
        # in eval mode it is the identity and the linear heads stay fused in the criterion kernels.
        self.dropout = nn.Dropout(p=0.5) if dropout else None
        self.rnnMode = rnnMode
        for _ in range(nPredicts):
            if rnnMode == "transformer":
                from .transformers import buildTransformerAR
                self.predictors.append(buildTransformerAR(dimOutputEncoder, 1, sizeInputSeq, False,
                                                          dropout=transformerDropout))
            elif rnnMode in _TORCH_PREDICTORS:
                self.predictors.append(_TORCH_PREDICTORS[rnnMode](dimOutputAR, dimOutputEncoder))
            else:
                self.predictors.append(nn.Linear(dimOutputAR, dimOutputEncoder, bias=False))
                if dimOutputEncoder > dimOutputAR:
                    # criterion.py:92-95: a head wider than the context starts as N(0, 1) on its first dimOutputAR output rows
                    # and RESIDUAL_STD * N(0, 1) on the others
                    residual = dimOutputEncoder - dimOutputAR
                    with torch.no_grad():
                        self.predictors[-1].weight.copy_(torch.cat([torch.randn(dimOutputAR, dimOutputAR),
                                                                    self.RESIDUAL_STD * torch.randn(residual, dimOutputAR)], dim=0))

    @property
    def scores_apart(self):
        """True where the predictions exist as a tensor between the prediction networks and the scores (transformer predictors;
        any predictor with the reference's dropout active; any widths other than 256 / 256): InfoNCEScoresFunction -- or, at
        those other widths, ops.nce_wide_scores -- instead of the fused InfoNCEFunction."""
        return (self.wide or self.rnnMode == "transformer" or self.rnnMode in _TORCH_PREDICTORS
                or (self.dropout is not None and self.training))

    group_predictors = True      # False: the transformer predictors run head by head (the path a mixed set falls back to; tests)

    def predictions(self, c):
        """c (B,W,dimOutputAR) -> (B,W,K*dimOutputEncoder): head k at columns k*dimOutputEncoder.. (the layout the score kernels
        read; 256 / 256 in the north-star configuration).  K one-layer transformer
        predictors (the only kind buildTransformerAR(.., 1, .., False) builds) run in lock-step, one launch per kernel for all
        of them (ops.TransformerGroupFunction); the K linear heads as one GEMM on the stacked weight; anything else head by head.
        The reference's dropout (criterion.py:113-114: per head, independent elementwise masks) is one dropout of the whole tensor."""
        pred = self._predictions(c)
        return pred if self.dropout is None else self.dropout(pred)

    def _predictions(self, c):
        from .transformers import TransformerLayer
        layers = [p[0] if isinstance(p, nn.Sequential) and len(p) == 1 else None for p in self.predictors]
        if (self.group_predictors and self.rnnMode == "transformer" and len(layers) > 1
                and all(isinstance(l, TransformerLayer) and l.fused for l in layers)
                and len({(l.dropout_p, l.training, l.multihead.Att.relpos) for l in layers}) == 1 and c.is_cuda):
            from .ops import TransformerGroupFunction
            l0 = layers[0]
            p, seed = 0.0, 0
            if l0.training and l0.dropout_p > 0:
                p = l0.dropout_p
                seed = int(torch.empty((), dtype=torch.int64).random_().item()) & 0xFFFFFFFFFFFFFFFF
            kinds = []
            for i, get in enumerate(_LAYER_PARAMS):
                ps = [get(l) for l in layers]
                kinds.append(None if ps[0] is None else stacked_parameters(self, f"layer{i}", ps))
            return TransformerGroupFunction.apply(c, p, seed, len(layers), *kinds)
        if all(isinstance(p, nn.Linear) and p.bias is None for p in self.predictors):
            return torch.nn.functional.linear(c, self.stacked_weight())
        if self._hip_predictors_apply(c):
            self.last_path = "hip"
            return self._hip_predictions(c)
        self.last_path = "torch"
        out = [p(c) for p in self.predictors]
        return torch.cat([o[0] if isinstance(o, tuple) else o for o in out], dim=2)     # (recurrent cells return (y, state))

    def _hip_predictors_apply(self, c):
        """hipPredictors: do the K predictors run on the HIP kernels for this input?  Only this package's own ShiftedConv /
        FFNetwork (without dropout), or plain one-layer nn.LSTM / tanh nn.RNN cells of 256 -> 256 as the reference builds them, on
        CUDA fp32 input of a shape the kernels take; anything else stays on the torch modules."""
        if not self.hipPredictors or self.rnnMode not in _HIP_PREDICTORS or len(self.predictors) == 0:
            return False
        if not c.is_cuda or c.dtype != torch.float32 or c.dim() != 3 or c.shape[2] != 256:
            return False
        kind = _HIP_PREDICTORS[self.rnnMode]
        if not all(type(p) is kind for p in self.predictors):
            return False
        if kind in (nn.LSTM, nn.RNN):
            K, (B, W, _) = len(self.predictors), c.shape
            for p in self.predictors:
                if (p.num_layers != 1 or p.input_size != 256 or p.hidden_size != 256 or not p.bias or p.bidirectional
                        or p.dropout != 0):
                    return False
                if kind is nn.LSTM and (p.proj_size != 0 or not p.batch_first):
                    return False
                if kind is nn.RNN and (p.nonlinearity != "tanh" or p.batch_first):
                    return False
                if any(getattr(p, n).dtype != torch.float32 or not getattr(p, n).is_cuda for n in _CELL_PARAMS):
                    return False
            from .ops import lstm_group_supported, rnn_supported
            return lstm_group_supported(B, W, K) if kind is nn.LSTM else rnn_supported(B, W, K, 1)
        if kind is FFNetwork:
            if any(p.drop.p != 0 or not isinstance(p.lin1.module, nn.Linear) or not isinstance(p.lin2.module, nn.Linear)
                   or tuple(q.module.weight.shape) != (256, 256) or q.module.bias is None
                   for p in self.predictors for q in (p.lin1, p.lin2)):
                return False
            ks = 1
        else:
            ks = self.predictors[0].kernelSize
            if any(p.kernelSize != ks or not isinstance(p.module.module, nn.Conv1d) or p.module.module.bias is None
                   or tuple(p.module.module.weight.shape) != (256, 256, ks) for p in self.predictors):
                return False
        from .ops import pred_conv_supported
        return pred_conv_supported(c.shape[0], c.shape[1], len(self.predictors), ks)

    def _hip_predictions(self, c):
        """The K ShiftedConv / FFNetwork predictors as grouped causal convolutions (ops.PredConvFunction) on the heads' stacked
        parameters: one call for conv4 / conv8 / conv12, two for ffd (lin1 with its ReLU on the shared input, lin2 per head).
        The K nn.LSTM / nn.RNN predictors as K recurrences side by side (ops.LstmGroupFunction / ops.RnnFunction): one call."""
        from .ops import LstmGroupFunction, PredConvFunction, RnnFunction
        K = len(self.predictors)
        if self.rnnMode in ("LSTM", "RNN"):
            # the K cells' parameters, kind by kind, as views of one buffer each; the modules keep them under the reference's keys.
            # nn.RNN without batch_first (criterion.py:62-64) walks the batch axis of c: T = B, R = W, time-major
            n = self.predictors[0].weight_hh_l0.shape[0]
            shapes = ((K * n, 256), (K, n, 256), (K * n,), (K * n,))
            kinds = [stacked_parameters(self, name, [getattr(p, name) for p in self.predictors], shape)
                     for name, shape in zip(_CELL_PARAMS, shapes)]
            if self.rnnMode == "LSTM":
                return LstmGroupFunction.apply(c, False, *kinds)
            return RnnFunction.apply(c, None, True, False, *kinds)[0]

        def stacked(key, layers):
            ks = layers[0].module.weight[0, 0].numel()
            w = stacked_parameters(self, key + ".weight", [l.module.weight for l in layers], (K, 256, 256, ks))
            b = stacked_parameters(self, key + ".bias", [l.module.bias for l in layers])
            return w, b, layers[0].weight

        if self.rnnMode == "ffd":
            w1, b1, s1 = stacked("lin1", [p.lin1 for p in self.predictors])
            w2, b2, s2 = stacked("lin2", [p.lin2 for p in self.predictors])
            h = PredConvFunction.apply(c, w1, b1, s1, True, True)
            return PredConvFunction.apply(h, w2, b2, s2, False, False)
        w, b, s = stacked("conv", [p.module for p in self.predictors])
        return PredConvFunction.apply(c, w, b, s, False, True)

    def stacked_weight(self):
        """(K*256, 256): the K head weights stacked along the output dimension (stacked_parameters: no per-step cat)."""
        ws = [p.weight for p in self.predictors]
        return stacked_parameters(self, "heads", ws, (len(ws) * ws[0].shape[0], ws[0].shape[1]))

    def forward(self, c, candidates):
        """Reference API (criterion.py:97-118) on materialised candidates; kept for callers
        that use PredictionNetwork directly.  The criterion below does not go through it."""
        assert len(candidates) == len(self.predictors)
        out = []
        for k in range(len(self.predictors)):
            locC = self.predictors[k](c)
            if isinstance(locC, tuple):
                locC = locC[0]
            if self.dropout is not None:
                locC = self.dropout(locC)
            locC = locC.view(locC.size(0), 1, locC.size(1), locC.size(2))
            out.append((locC * candidates[k]).mean(dim=3))
        return out


class BaseCriterion(nn.Module):
    """cpc/criterion/criterion.py:121-127."""

    def warmUp(self):
        return False

    def update(self):
        return


class CPCUnsupersivedCriterion(BaseCriterion):
    """cpc/criterion/criterion.py:139-257."""

    def __init__(self,
                 nPredicts,             # Number of steps
                 dimOutputAR,           # Dimension of G_ar
                 dimOutputEncoder,      # Dimension of the convolutional net
                 negativeSamplingExt,   # Number of negative samples to draw
                 mode=None,
                 rnnMode=False,
                 dropout=False,
                 speakerEmbedding=0,
                 nSpeakers=0,
                 sizeInputSeq=128,
                 transformerDropout=0.1,
                 hipPredictors=False):  # ffd / conv4 / conv8 / conv12 / LSTM / RNN predictors on HIP kernels (PredictionNetwork)
        super().__init__()
        if speakerEmbedding > 0:
            # criterion.py:154-160, 238-241: a learned embedding of the speaker label widens the context the heads read
            if nSpeakers < 1:
                raise ValueError("speakerEmbedding needs nSpeakers >= 1")
            self.speakerEmb = nn.Embedding(nSpeakers, speakerEmbedding)
            dimOutputAR += speakerEmbedding
        else:
            self.speakerEmb = None
        self.wPrediction = PredictionNetwork(nPredicts, dimOutputAR, dimOutputEncoder, rnnMode=rnnMode,
                                             dropout=dropout, sizeInputSeq=sizeInputSeq - nPredicts,
                                             transformerDropout=transformerDropout, hipPredictors=hipPredictors)
        if self.speakerEmb is not None:
            self.wPrediction.wide = True          # (even at 256 + E -> 256 ... or 256 -> 256 heads: the context is formed here)
        self.nPredicts = nPredicts
        self.negativeSamplingExt = negativeSamplingExt
        # (any number: the kernels walk candidates in 16-wide tiles and mask the padding of the last one, ops.prepare_negatives)
        self.lossCriterion = nn.CrossEntropyLoss()   # kept for API parity; the fused kernel computes it
        if mode not in [None, "reverse"]:
            raise ValueError("Invalid mode")
        self.mode = mode

    def drawNegatives(self, batchSize, seqSize, windowSize, device):
        """The two draws of sampleClean in the reference's order (criterion.py:181-189):
        batchIdx in [0,B) first, then seqIdx in [1,S), both flat in (b,n,t) order."""
        n = self.negativeSamplingExt * windowSize * batchSize
        batchIdx = torch.randint(low=0, high=batchSize, size=(n,), device=device)
        seqIdx = torch.randint(low=1, high=seqSize, size=(n,), device=device)
        return batchIdx, seqIdx

    def negativeRows(self, batchIdx, seqIdx, batchSize, seqSize, windowSize):
        """criterion.py:191-199: row = ((seqIdx + t) mod S) + batchIdx*S, returned as the (B, W, N) int32
        layout the score kernel reads.  Torch reference of what cpc_nce_prepare computes on the device
        (used by tests; forward() calls the kernel)."""
        N = self.negativeSamplingExt
        t = torch.arange(windowSize, device=seqIdx.device).view(1, 1, windowSize)
        s = torch.remainder(seqIdx.view(batchSize, N, windowSize) + t, seqSize)
        ext = s + batchIdx.view(batchSize, N, windowSize) * seqSize
        return ext.permute(0, 2, 1).contiguous().to(torch.int32)

    def prepare_step(self, step, batchSize, seqSize, device, c_bound=None, negatives=None):
        """Everything of this criterion's step that depends on nothing the GPU is still to compute, queued on the step's side
        stream from the START of the step (``step``: the ops.StepContext the train loop has just entered) so that it runs beside
        the encoder: the negative draws with their index preparation (or the preparation of the caller's ``negatives``), and --
        linear heads, ``c_bound`` given: the context network bounds its output a priori, |c| <= c_bound (a GRU: 1) -- the
        operand bounds of the prediction GEMMs, whose reduction otherwise sits on the critical path between the context
        network and the first GEMM.  forward() picks the result up when the shapes match and falls back to doing it in line
        otherwise; calling this is optional."""
        from . import ops
        if (step is None or not step.overlap or torch.device(device).type != "cuda" or self.mode == "reverse"
                or self.nPredicts > _HEAD_TILE):
            return
        K, N = self.nPredicts, self.negativeSamplingExt
        W = seqSize - K
        main, side = torch.cuda.current_stream(device), step.side_stream(device)
        if step.begin is not None:
            side.wait_event(step.begin)
        given = None if negatives is None else id(negatives[0])
        with torch.cuda.stream(side):
            if negatives is None:
                negatives = self.drawNegatives(batchSize, seqSize, W, device)
            ext, perm, row_ptr = prepare_negatives(negatives[0], negatives[1], batchSize, seqSize, K, N)
            saved = None
            if c_bound is not None and not self.wPrediction.scores_apart:
                saved = ops.nce_bounds_into(self.wPrediction.stacked_weight(), c_bound, batchSize, seqSize, K, N)
            ready = torch.cuda.Event()
            ready.record(side)
        step.prepared = {"key": (batchSize, seqSize, K, N, torch.device(device)), "index": (ext, perm, row_ptr),
                         "saved": saved, "ready": ready, "given": given, "c_bound": c_bound}

    def forward(self, cFeature, encodedData, label, negatives=None):
        """-> (losses (1,K), acc (1,K)) as criterion.py:256-257.  ``negatives`` optionally
        supplies (batchIdx, seqIdx) instead of drawing them (parity tests)."""
        if self.mode == "reverse":
            encodedData = torch.flip(encodedData, [1])
            cFeature = torch.flip(cFeature, [1])
        batchSize, seqSize, _ = cFeature.size()
        windowSize = seqSize - self.nPredicts
        from . import ops
        if self.wPrediction.wide:
            ops._require_cuda(cFeature, "CPCUnsupersivedCriterion")
            ops._require_cuda(encodedData, "CPCUnsupersivedCriterion")
            if encodedData.shape[2] != self.wPrediction.dimOutputEncoder:
                raise ValueError(f"CPCUnsupersivedCriterion: encodedData has {encodedData.shape[2]} channels, the heads predict "
                                 f"{self.wPrediction.dimOutputEncoder}")
        if self.nPredicts > _HEAD_TILE:
            return self._forward_in_head_groups(cFeature, encodedData, negatives, label)
        step = ops.current()
        prepared, saved = (step.prepared if step is not None else None), None
        if step is not None:
            step.prepared = None
        if (prepared is not None and self.mode != "reverse"
                and prepared["given"] == (None if negatives is None else id(negatives[0])) and prepared["key"] == (batchSize, seqSize, self.nPredicts, self.negativeSamplingExt, cFeature.device)):
            # queued at the start of the step (prepare_step): long finished by now
            torch.cuda.current_stream().wait_event(prepared["ready"])
            ext, perm, row_ptr = prepared["index"]
            saved = prepared["saved"]
            # the workspace carries GEMM operand scales for |c| <= c_bound: taken only if THIS cFeature is the tensor the bounded
            # network returned (CPCAR.forward tags it); a transformed c, or one from a state assigned from outside, has its
            # bounds reduced in line instead (fp16 pieces overflow silently ~8x above the bound)
            tag = getattr(cFeature, "_cpc_abs_bound", None)
            if saved is not None and (tag is None or prepared["c_bound"] is None or tag > prepared["c_bound"]):
                saved = None
            for t in (ext, perm, row_ptr) + (() if saved is None else (saved,)):
                t.record_stream(torch.cuda.current_stream())
        elif negatives is None and step is not None and step.overlap and cFeature.is_cuda:
            # the draws and their index preparation depend on nothing the GPU is still computing (encoder, AR): issued
            # on the side stream they run beside the latency-bound recurrence instead of after it
            main, side = torch.cuda.current_stream(), step.side_stream(cFeature.device)
            # (holding them back until the recurrence starts was measured twice: 4.187 vs 4.162 ms/step in round 1, 3.426 vs
            # 3.373 with the paced polls of round 2 -- they disturb its hand-over more than they cost beside the first conv
            # layers, where the host-side lead puts them)
            if step.begin is not None:
                side.wait_event(step.begin)           # fork from the start of the step (ops.StepContext.__enter__)
            with torch.cuda.stream(side):
                negatives = self.drawNegatives(batchSize, seqSize, windowSize, cFeature.device)
                ext, perm, row_ptr = prepare_negatives(negatives[0], negatives[1], batchSize, seqSize, self.nPredicts,
                                                       self.negativeSamplingExt)
            main.wait_stream(side)
            for t in (ext, perm, row_ptr):
                t.record_stream(main)
        else:
            if negatives is None:
                negatives = self.drawNegatives(batchSize, seqSize, windowSize, cFeature.device)
            ext, perm, row_ptr = prepare_negatives(negatives[0], negatives[1], batchSize, seqSize, self.nPredicts,
                                                   self.negativeSamplingExt)
        if self.wPrediction.scores_apart:
            pred = self.wPrediction.predictions(self._context(cFeature, windowSize, label))
            if self.wPrediction.wide:
                losses, acc = nce_wide_scores(pred, encodedData, ext, perm, row_ptr, self.negativeSamplingExt)
            else:
                losses, acc = InfoNCEScoresFunction.apply(pred, encodedData, ext, perm, row_ptr, self.negativeSamplingExt)
        else:
            heads = [p.weight for p in self.wPrediction.predictors]
            # dz may be filled late (on the side stream) only if nobody outside this package can read it first: not in
            # mode 'reverse' (the flip above sits between the criterion and the encoder), not behind a foreign network
            defer = step is not None and step.overlap and ops.dz_may_be_deferred(cFeature, encodedData)
            losses, acc = InfoNCEFunction.apply(cFeature, encodedData, self.wPrediction.stacked_weight(), ext, perm,
                                                row_ptr, heads, defer, saved, self.negativeSamplingExt)
        return losses.view(1, -1), acc.view(1, -1)

    def _context(self, cFeature, windowSize, label):
        """The first W steps of the context as the prediction networks read them: with a speaker embedding
        (criterion.py:238-241) the embedded label of the sequence is appended to every step."""
        c = cFeature[:, :windowSize].contiguous()
        if self.speakerEmb is None:
            return c
        if label is None:
            raise ValueError("CPCUnsupersivedCriterion: speakerEmbedding needs the speaker labels")
        l_ = label.view(c.shape[0], 1).expand(c.shape[0], windowSize)
        return torch.cat([c, self.speakerEmb(l_)], dim=2)

    def _forward_in_head_groups(self, cFeature, encodedData, negatives, label=None):
        """nPredicts > 16 (no BASELINE config; the reference takes any): the same kernels on 16 heads at a time
        (ops.head_group -- every group sees the W = S - nPredicts windows of the whole criterion and the same negatives, head
        k's positive is z[t + k + 1]); the per-head losses and accuracies are independent, autograd adds the groups' dc / dz.
        Single stream, no overlap: not the tuned path."""
        B, S, _ = cFeature.size()
        K, N = self.nPredicts, self.negativeSamplingExt
        W = S - K
        if negatives is None:
            negatives = self.drawNegatives(B, S, W, cFeature.device)
        wp = self.wPrediction
        pred = wp.predictions(self._context(cFeature, W, label)) if wp.scores_apart else None
        C = wp.dimOutputEncoder
        wall = None if wp.scores_apart else wp.stacked_weight()
        losses, accs = [], []
        for k0 in range(0, K, _HEAD_TILE):
            kg = min(_HEAD_TILE, K - k0)
            ext, perm, row_ptr = prepare_negatives(negatives[0], negatives[1], B, S, kg, N, group=(k0, K))
            if wp.wide:
                l, a = nce_wide_scores(pred[:, :, k0 * C:(k0 + kg) * C], encodedData, ext, perm, row_ptr, N, (k0, K))
            elif wp.scores_apart:
                l, a = InfoNCEScoresFunction.apply(pred[:, :, k0 * 256:(k0 + kg) * 256], encodedData, ext, perm, row_ptr, N,
                                                   (k0, K))
            else:
                l, a = InfoNCEFunction.apply(cFeature, encodedData, wall[k0 * 256:(k0 + kg) * 256], ext, perm, row_ptr, None,
                                             False, None, N, (k0, K))
            losses.append(l)
            accs.append(a)
        return torch.cat(losses).view(1, -1), torch.cat(accs).view(1, -1)


# --------------------------------------------------------------------------- supervised criteria
# cpc/criterion/criterion.py:128-367: what linear-separability evaluation (cpc/eval/linear_separability.py) and
# train.py --supervised train on top of CPC features.  With 256 input features and one linear layer the loss, the accuracy and
# every gradient run in csrc/supervised.hip (ops.ClassifierXentFunction / ops.CtcXentFunction: CUDA fp32 only, CPU tensors
# raise); other widths and nLayers > 1 run on the modules' own torch ops (``hip_path`` is False), as the reference does.
# ``wideKernel`` (an addition; off by default): one linear layer on 1 to 512 features other than 256 runs the same Functions on the
# library's _d entry points for CUDA fp32 input (``hip_wide``; ``hip_path`` keeps its value) and the torch ops for anything else.

def _on_hip(layer, dim):
    return dim == 256 and isinstance(layer, nn.Linear)


def _on_hip_wide(layer, dim, wideKernel):
    return bool(wideKernel) and 1 <= dim <= 512 and dim != 256 and isinstance(layer, nn.Linear)


def _takes_wide(crit, features):
    return crit.hip_wide and features.is_cuda and features.dtype == torch.float32


class NoneCriterion(BaseCriterion):
    """cpc/criterion/criterion.py:130-136."""

    def forward(self, cFeature, encodedData, label):
        return torch.zeros(1, 1, device=cFeature.device), torch.zeros(1, 1, device=cFeature.device)


class SpeakerCriterion(BaseCriterion):
    """cpc/criterion/criterion.py:182-203: a linear classifier of the last frame's context vector."""

    def __init__(self, dimEncoder, nSpeakers, wideKernel=False):
        super().__init__()
        self.linearSpeakerClassifier = nn.Linear(dimEncoder, nSpeakers)
        self.lossCriterion = nn.CrossEntropyLoss()
        self.entropyCriterion = nn.LogSoftmax(dim=1)
        self.hip_path = _on_hip(self.linearSpeakerClassifier, dimEncoder)
        self.hip_wide = _on_hip_wide(self.linearSpeakerClassifier, dimEncoder, wideKernel)

    def forward(self, cFeature, otherEncoded, label):
        batchSize = cFeature.size(0)
        last = cFeature[:, -1, :]                              # read in place by the kernel (row stride S * 256)
        lin = self.linearSpeakerClassifier
        if self.hip_path or _takes_wide(self, last):
            return ClassifierXentFunction.apply(last, label, lin.weight, lin.bias)
        predictions = lin(last.reshape(batchSize, -1))
        loss = self.lossCriterion(predictions, label).view(1, -1)
        acc = (predictions.max(1)[1] == label).double().mean().view(1, -1)
        return loss, acc


class PhoneCriterion(BaseCriterion):
    """cpc/criterion/criterion.py:206-246: a per-frame classifier of the context vectors (or of the encoder's output when
    ``onEncoder``); nLayers > 1 stacks Linear / ReLU / Linear (nPhones wide) and runs on torch."""

    def __init__(self, dimEncoder, nPhones, onEncoder, nLayers=1, wideKernel=False):
        super().__init__()
        if nLayers == 1:
            self.PhoneCriterionClassifier = nn.Linear(dimEncoder, nPhones)
        else:
            outLayers = [nn.Linear(dimEncoder, nPhones)]
            for _ in range(nLayers - 1):
                outLayers.append(nn.ReLU())
                outLayers.append(nn.Linear(nPhones, nPhones))
            self.PhoneCriterionClassifier = nn.Sequential(*outLayers)
        self.lossCriterion = nn.CrossEntropyLoss()
        self.onEncoder = onEncoder
        self.hip_path = _on_hip(self.PhoneCriterionClassifier, dimEncoder)
        self.hip_wide = _on_hip_wide(self.PhoneCriterionClassifier, dimEncoder, wideKernel)

    def forward(self, cFeature, otherEncoded, label):
        features = otherEncoded if self.onEncoder else cFeature
        B, S = features.size(0), features.size(1)
        if label.dim() != 2 or tuple(label.shape) != (B, S):
            raise ValueError(f"PhoneCriterion: per-frame labels of shape ({B}, {S}) expected, got {tuple(label.shape)}")
        if self.hip_path or _takes_wide(self, features):
            lin = self.PhoneCriterionClassifier
            return ClassifierXentFunction.apply(features.reshape(B * S, -1), label.reshape(-1), lin.weight, lin.bias)
        predictions = self.getPrediction(features)
        predictions = predictions.view(-1, predictions.size(2))
        label = label.view(-1)
        loss = self.lossCriterion(predictions, label).view(1, -1)
        acc = (predictions.max(1)[1] == label).double().mean().view(1, -1)
        return loss, acc

    def getPrediction(self, cFeature):
        batchSize, seqSize = cFeature.size(0), cFeature.size(1)
        cFeature = cFeature.contiguous().view(batchSize * seqSize, -1)
        output = self.PhoneCriterionClassifier(cFeature)
        return output.view(batchSize, seqSize, -1)


def collapse_label_chain(labels):
    """cpc/criterion/seq_alignment.py:64-86 without the host round trip: (B, S) frame labels -> (the collapsed labels of all
    sequences one behind the other, their lengths (B,)) -- position 0 and every position whose label differs from the one
    before.  The HIP path collapses inside the kernel; this serves the torch path."""
    keep = torch.ones_like(labels, dtype=torch.bool)
    keep[:, 1:] = labels[:, 1:] != labels[:, :-1]
    return labels[keep], keep.sum(dim=1)


class CTCPhoneCriterion(BaseCriterion):
    """cpc/criterion/criterion.py:249-283: a per-frame classifier with one extra (blank) class trained with nn.CTCLoss on the
    collapsed frame labels; the second output is zeros(1, 1), as in the reference."""

    def __init__(self, dimEncoder, nPhones, onEncoder, wideKernel=False):
        super().__init__()
        self.PhoneCriterionClassifier = nn.Linear(dimEncoder, nPhones + 1)
        self.lossCriterion = nn.CTCLoss(blank=nPhones, zero_infinity=True)
        self.onEncoder = onEncoder
        if onEncoder:
            raise ValueError("On encoder version not implemented yet")
        self.BLANK_LABEL = nPhones
        self.hip_path = _on_hip(self.PhoneCriterionClassifier, dimEncoder)
        self.hip_wide = _on_hip_wide(self.PhoneCriterionClassifier, dimEncoder, wideKernel)

    def getPrediction(self, cFeature):
        B, S, H = cFeature.size()
        cFeature = cFeature.contiguous().view(B * S, H)
        return self.PhoneCriterionClassifier(cFeature).view(B, S, -1)

    def forward(self, cFeature, otherEncoded, label):
        B, S, H = cFeature.size()
        if label.dim() != 2 or tuple(label.shape) != (B, S):
            raise ValueError(f"CTCPhoneCriterion: per-frame labels of shape ({B}, {S}) expected, got {tuple(label.shape)}")
        if self.hip_path or _takes_wide(self, cFeature):
            lin = self.PhoneCriterionClassifier
            loss = CtcXentFunction.apply(cFeature, label, lin.weight, lin.bias)
            return loss, torch.zeros(1, 1, device=loss.device)
        predictions = F.log_softmax(self.getPrediction(cFeature), dim=2).permute(1, 0, 2)
        targets, sizes = collapse_label_chain(label.to(predictions.device))
        inputSizes = torch.full((B,), S, dtype=torch.int64, device=predictions.device)
        loss = self.lossCriterion(predictions, targets, inputSizes, sizes).view(1, -1)
        return loss, torch.zeros(1, 1, device=loss.device)


class ModelCriterionCombined(torch.nn.Module):
    """cpc/criterion/criterion.py:358-367."""

    def __init__(self, model, criterion):
        super().__init__()
        self.model = model
        self.criterion = criterion

    def forward(self, data, label):
        c_feature, encoded_data, label = self.model(data, label)
        loss, acc = self.criterion(c_feature, encoded_data, label)
        return loss, acc
