"""Drop-in replacements for the hot-path modules of the reference's cpc/model.py.

Same class names, constructor signatures, attributes and state-dict keys
(gEncoder.conv{i}.{weight,bias}, gEncoder.batchNorm{i}.{weight,bias} of shape (1,C,1),
gAR.baseNet.{weight,bias}_{ih,hh}_l{n}), so reference checkpoints load and the
reference's cpc/train.py loop can drive these modules unchanged.
forward/backward run in the HIP kernels of libcpc_hip.so.
"""
import torch
import torch.nn as nn

from . import ops
from .ops import (EncoderFunction, EncoderNormFunction, EncoderWideFunction, GruFunction, GruHiddenFunction, LstmFunction, LstmHiddenFunction,
                  RnnFunction)


class ChannelNorm(nn.Module):
    """cpc/model.py:25-58.  Inside CPCEncoder the normalisation is fused into the conv
    kernels; this module owns the affine parameters (checkpoint keys) and, when called on
    its own, evaluates the same formula with torch ops (not on the train-step hot path)."""

    def __init__(self, numFeatures, epsilon=1e-05, affine=True):
        super().__init__()
        self.epsilon, self.affine, self.p = epsilon, affine, 0
        shape = (1, numFeatures, 1)                      # broadcast over (batch, channel, time): the checkpoint layout
        self.weight = nn.Parameter(torch.ones(shape)) if affine else None
        self.bias = nn.Parameter(torch.zeros(shape)) if affine else None

    def reset_parameters(self):
        if self.affine:
            with torch.no_grad():
                self.weight.fill_(1.0)
                self.bias.zero_()

    def forward(self, x):
        var, mean = torch.var_mean(x, dim=1, keepdim=True)          # unbiased variance over the channels, as the reference
        xhat = (x - mean) * torch.rsqrt(var + self.epsilon)
        return torch.addcmul(self.bias, xhat, self.weight) if self.affine else xhat


class IDModule(nn.Module):
    """cpc/model.py:17-22 (normMode 'ID')."""

    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, x):
        return x


class CPCEncoder(nn.Module):
    """cpc/model.py:61-105: five strided Conv1d + norm + ReLU, downsampling 160.

    conv{i} / batchNorm{i} carry the reference's names, shapes and default initialisation.  The configuration every BASELINE
    config and the reference's defaults use -- 256 channels, normMode 'layerNorm' (ChannelNorm) -- runs cpc_encoder_forward
    (HIP, ``self.hip``); without the keyword below the reference's other options (``batchNorm`` / ``instanceNorm`` / ``ID``,
    other widths; cpc/model.py:73-80) are served by the modules' own torch ops: correct on any device, differentiable.

    ``encoderKernel=True`` (an addition; default off) takes any other width from 2 to 512 under 'layerNorm' to the encoder kernels
    of any width for CUDA fp32 input (``self.hip_wide``; ops.EncoderWideFunction, cpc_encoder_forward_c / _backward_c: exact-f32
    MFMAs on zero-padded storage).  ``self.hip`` keeps meaning the 256 kernels -- what the fused train step tests -- and stays
    False there; CPU input and other dtypes keep the torch ops.  Parameters, state-dict keys and shapes do not change.
    With the keyword the other three normModes run HIP kernels too (``self.hip_norm``; ops.EncoderNormFunction,
    cpc_encoder_forward_n / _backward_n) at every width from 2 to 512, 256 included: nn.BatchNorm1d's batch
    statistics and running buffers in training (``num_batches_tracked`` counted here, as a torch op) and its running statistics
    in eval mode, nn.InstanceNorm1d's per-utterance statistics, ID's plain ReLU.  A window too short for torch's own check (one
    value per channel), a BatchNorm1d whose ``momentum`` / ``eps`` / ``affine`` / ``track_running_stats`` were changed by hand,
    CPU input and other dtypes keep the torch ops and raise where torch raises.  ``self.hip`` and ``self.hip_wide`` stay False for
    these modes, so the fused one-call train step keeps declining such a model."""

    def __init__(self, sizeHidden=512, normMode="layerNorm", encoderKernel=False):
        super().__init__()
        validModes = ["batchNorm", "instanceNorm", "ID", "layerNorm"]
        if normMode not in validModes:
            raise ValueError(f"Norm mode must be in {validModes}")
        self.hip = normMode == "layerNorm" and sizeHidden == 256
        self.hip_wide = (bool(encoderKernel) and normMode == "layerNorm" and sizeHidden != 256
                         and 2 <= sizeHidden <= ops.ENCODER_WIDE_MAX)
        self.hip_norm = bool(encoderKernel) and normMode != "layerNorm" and 2 <= sizeHidden <= ops.ENCODER_WIDE_MAX
        self.normMode = normMode
        if normMode == "instanceNorm":
            def normLayer(c): return nn.InstanceNorm1d(c, affine=True)
        elif normMode == "ID":
            normLayer = IDModule
        elif normMode == "layerNorm":
            normLayer = ChannelNorm
        else:
            normLayer = nn.BatchNorm1d
        self.dimEncoded = sizeHidden
        self.conv0 = nn.Conv1d(1, sizeHidden, 10, stride=5, padding=3)
        self.batchNorm0 = normLayer(sizeHidden)
        self.conv1 = nn.Conv1d(sizeHidden, sizeHidden, 8, stride=4, padding=2)
        self.batchNorm1 = normLayer(sizeHidden)
        self.conv2 = nn.Conv1d(sizeHidden, sizeHidden, 4, stride=2, padding=1)
        self.batchNorm2 = normLayer(sizeHidden)
        self.conv3 = nn.Conv1d(sizeHidden, sizeHidden, 4, stride=2, padding=1)
        self.batchNorm3 = normLayer(sizeHidden)
        self.conv4 = nn.Conv1d(sizeHidden, sizeHidden, 4, stride=2, padding=1)
        self.batchNorm4 = normLayer(sizeHidden)
        self.DOWNSAMPLING = 160

    def getDimOutput(self):
        return self.conv4.out_channels

    def _flat_params(self):
        out = []
        for i in range(5):
            conv, norm = getattr(self, f"conv{i}"), getattr(self, f"batchNorm{i}")
            out += [conv.weight, conv.bias, norm.weight, norm.bias]
        return out

    def _norm_kernels_take(self, x):
        """Do the kernels of the other normModes compute what the torch modules would for this input?  Not below torch's
        minima (instanceNorm: two steps at the last layer; batchNorm in training: two values per channel), where torch raises,
        and not for norm modules whose settings were changed by hand."""
        if x.dim() != 3 or x.shape[1] != 1:
            return False
        lin = x.shape[2]
        for k, s, p in ((10, 5, 3), (8, 4, 2), (4, 2, 1), (4, 2, 1), (4, 2, 1)):
            if lin + 2 * p < k:
                return False
            lin = (lin + 2 * p - k) // s + 1
        norms = [getattr(self, f"batchNorm{i}") for i in range(5)]
        if self.normMode == "instanceNorm":
            return lin >= 2 and all(n.affine and not n.track_running_stats and n.eps == 1e-5 for n in norms)
        if self.normMode == "batchNorm":
            return ((not self.training or x.shape[0] * lin >= 2) and
                    all(n.affine and n.track_running_stats and n.momentum == 0.1 and n.eps == 1e-5
                        and n.running_mean is not None and n.running_mean.dtype == torch.float32 for n in norms))
        return True

    def _forward_norm(self, x):
        """z (B, L/160, C) on the kernels of batchNorm / instanceNorm / ID"""
        norms = [getattr(self, f"batchNorm{i}") for i in range(5)]
        running, training = None, self.training
        if self.normMode == "batchNorm":
            running = [t for n in norms for t in (n.running_mean, n.running_var)]
            if training:
                for n in norms:
                    n.num_batches_tracked.add_(1)
        if self.normMode == "ID":
            params = [t for i in range(5) for t in (getattr(self, f"conv{i}").weight, getattr(self, f"conv{i}").bias)]
        else:
            params = self._flat_params()
        return EncoderNormFunction.apply(x, self.normMode, training, running, 0.1, 1e-5, *params)

    def forward(self, x):
        """(B,1,L) -> (B,C,L/160), as the reference.  The kernels work channels-last, so the
        result is a (B,C,S) VIEW of a contiguous (B,S,C) tensor; CPCModel's permute(0,2,1)
        (model.py:287) therefore yields a contiguous (B,S,C) z at no cost."""
        if self.hip_wide and x.is_cuda and x.dtype == torch.float32 and self.conv0.weight.dtype == torch.float32:
            return EncoderWideFunction.apply(x, *self._flat_params()).permute(0, 2, 1)
        if self.hip_norm and x.is_cuda and x.dtype == torch.float32 and self.conv0.weight.dtype == torch.float32 \
                and self._norm_kernels_take(x):
            return self._forward_norm(x).permute(0, 2, 1)
        if not self.hip:
            for i in range(5):                                 # cpc/model.py:99-105 with the modules' own torch ops
                x = torch.relu(getattr(self, f"batchNorm{i}")(getattr(self, f"conv{i}")(x)))
            return x
        z = EncoderFunction.apply(x, *self._flat_params())
        return z.permute(0, 2, 1)


class LFBEnconder(nn.Module):
    """cpc/model.py:125-152 (--encoder_type lfb; the class name is the reference's): learned filter banks.  Conv1d(1, 2 dimEncoded,
    400), squared modulus of adjacent channel pairs, a Hann low-pass of 400 taps at stride 160 (padding 350), log(1 + |.|) and an
    InstanceNorm1d without affine parameters or running statistics (the same in train and eval mode).  Members and state-dict
    keys are the reference's: ``han``, ``conv.weight`` (2 dimEncoded, 1, 400), ``conv.bias``.

    Departure from the reference: its class has no ``DOWNSAMPLING`` attribute and no ``getDimOutput()``, so its own train.py and
    FeatureModule fail on it; this one carries ``DOWNSAMPLING = 160`` (the Hann stride) and ``getDimOutput()``.

    CUDA fp32 input with ``hip`` set and a shape ``ops.lfb_supported`` takes runs ops.LfbFunction (HIP: the conv output, 41 MB per
    1.28 s window at 256 filters, is never stored; ``self.han`` is the window the kernel reads).  Unlike CPCEncoder this module
    has a COMPLETE torch path -- the reference's formula in torch ops, any device, differentiable -- which serves every other
    width, other dtypes and the CPU, and ``hip=False`` selects it on the GPU too."""

    def __init__(self, dimEncoded, normalize=True, hip=True):
        super().__init__()
        self.dimEncoded = dimEncoded
        self.conv = nn.Conv1d(1, 2 * dimEncoded, 400, stride=1)
        self.register_buffer("han", torch.hann_window(400).view(1, 1, 400))
        self.instancenorm = nn.InstanceNorm1d(dimEncoded, momentum=1) if normalize else None
        self.hip = bool(hip)
        self.DOWNSAMPLING = 160

    def getDimOutput(self):
        return self.dimEncoded

    def forward(self, x):
        """(N, 1, L) -> (N, dimEncoded, (L - 99) // 160 + 1).  On the HIP path the result is the (N, D, F) view of a contiguous
        (N, F, D) tensor, so CPCModel's permute(0, 2, 1) yields a contiguous z."""
        N, _, L = x.size()
        if L < 400:
            raise ValueError(f"LFBEnconder: a window of {L} samples is shorter than the 400 filter taps")
        if self.hip and x.is_cuda and x.dtype == torch.float32 and self.conv.weight.dtype == torch.float32 \
                and ops.lfb_supported(N, L, self.dimEncoded):
            return ops.LfbFunction.apply(x, self.conv.weight, self.conv.bias, self.han, self.instancenorm is not None,
                                         torch.is_grad_enabled())
        x = self.conv(x).view(N, self.dimEncoded, 2, -1)
        x = x[:, :, 0, :] ** 2 + x[:, :, 1, :] ** 2
        x = torch.nn.functional.conv1d(x.reshape(N * self.dimEncoded, 1, -1), self.han, bias=None, stride=160, padding=350)
        x = torch.log(1 + torch.abs(x.view(N, self.dimEncoded, -1)))
        return x if self.instancenorm is None else self.instancenorm(x)


class MFCCEncoder(nn.Module):
    """cpc/model.py:108-122 (--encoder_type mfcc): the reference's hand-made baseline,
    torchaudio.transforms.MFCC(n_mfcc=dimEncoded, melkwargs={"n_mels": max(128, dimEncoded), "n_fft": 321}) followed by its
    permute -- restated here from torchaudio's documented defaults (sample rate 16 kHz, periodic Hann window of 321 points, hop
    160, centred frames with reflect padding, power spectrum, HTK mel scale over the grid linspace(0, 8000, 161) without area
    normalisation, 10 log10 with a floor 80 dB below the maximum of the WHOLE input tensor, orthonormal DCT-II), because
    torchaudio is not a dependency of this package.  The restatement matches torchaudio's documented formula; it has not been
    compared with an installed torchaudio.

    The tables are buffers under the names torchaudio gives them, so that a reference checkpoint loads into them:
    ``MFCC.MelSpectrogram.spectrogram.window`` (321), ``MFCC.MelSpectrogram.mel_scale.fb`` (161, M) and ``MFCC.dct_mat`` (M, D).
    These names are written from memory of torchaudio's modules and are unverified; every load in this package is strict=False,
    so a mismatch cannot break one.  ``basis`` (321, 322), the windowed DFT basis the kernel reads, is a non-persistent buffer
    derived from ``window``; it is rebuilt when a state dict is loaded.  There are no parameters and the waveform receives no
    gradient: the output never requires grad.

    Departure from the reference: its class has no ``DOWNSAMPLING`` attribute and no ``getDimOutput()``, so its own train.py and
    FeatureModule fail on it; this one carries ``DOWNSAMPLING = 160`` (the hop) and ``getDimOutput()``, as LFBEnconder does.

    ``topPerRow`` selects the scope of the maximum the dB floor hangs on: False (the default, the reference's behaviour: torchaudio
    packs an (N, M, F) input as one item, so a quiet row is floored by a loud row of the same batch) or True (each row by its own
    maximum: what calls on one row at a time give; harness.build_feature sets it around its batched call).

    CUDA fp32 input with ``hip`` set and a shape ``ops.mfcc_supported`` takes runs ops.mfcc (HIP, csrc/mfcc.hip: the frames, the
    spectrum and the power never reach memory).  Like LFBEnconder this module has a COMPLETE torch path -- the formula above on
    torch.stft and two matmuls, from float64 copies of the tables -- which serves every other dtype and the CPU, and
    ``hip=False`` selects it on the GPU too."""

    def __init__(self, dimEncoded, hip=True):
        super().__init__()
        self.dimEncoded = dimEncoded
        basis, fb, dct = ops.mfcc_tables(dimEncoded)
        self.MFCC = nn.Module()
        self.MFCC.MelSpectrogram = nn.Module()
        self.MFCC.MelSpectrogram.spectrogram = nn.Module()
        self.MFCC.MelSpectrogram.mel_scale = nn.Module()
        self.MFCC.MelSpectrogram.spectrogram.register_buffer("window", ops.mfcc_window().float())
        self.MFCC.MelSpectrogram.mel_scale.register_buffer("fb", fb)
        self.MFCC.register_buffer("dct_mat", dct)
        self.register_buffer("basis", basis, persistent=False)
        self._exact = ops.mfcc_tables64(dimEncoded)          # float64 on the CPU: what the torch path computes from
        self._cast = {}
        self.register_load_state_dict_post_hook(MFCCEncoder._after_load)
        self.hip = bool(hip)
        self.topPerRow = False
        self.DOWNSAMPLING = 160

    def _buffers3(self):
        return self.MFCC.MelSpectrogram.spectrogram.window, self.MFCC.MelSpectrogram.mel_scale.fb, self.MFCC.dct_mat

    def _after_load(self, incompatible_keys):
        """The loaded tables are the truth from now on: the torch path's copies and the kernel's basis follow them."""
        with torch.no_grad():
            self._exact = tuple(t.detach().to(device="cpu", dtype=torch.float64).clone() for t in self._buffers3())
            self._cast = {}
            self.basis.copy_(ops.mfcc_basis(self._exact[0]).to(self.basis))

    def _tables(self, device, dtype):
        key = (device, dtype)
        if key not in self._cast:
            self._cast = {key: tuple(t.to(device=device, dtype=dtype) for t in self._exact)}
        return self._cast[key]

    def getDimOutput(self):
        return self.dimEncoded

    def forward(self, x):
        """(N, 1, L) or (N, L) -> (N, dimEncoded, (L - 1) // 160 + 1).  On the HIP path the result is the (N, D, F) view of a
        contiguous (N, F, D) tensor, so CPCModel's permute(0, 2, 1) yields a contiguous z."""
        N, L = x.size(0), x.size(-1)
        if L < 161:
            raise ValueError(f"MFCCEncoder: a window of {L} samples is shorter than the 161 a reflect padding of 160 needs")
        x = x.detach().reshape(N, L)
        window, fb, dct = self._buffers3()
        if self.hip and x.is_cuda and x.dtype == torch.float32 and self.basis.is_cuda and self.basis.dtype == torch.float32 \
                and fb.dtype == torch.float32 and dct.dtype == torch.float32 and ops.mfcc_supported(N, L, self.dimEncoded):
            return ops.mfcc(x, self.basis, fb, dct, rowwise=self.topPerRow)
        with torch.no_grad():
            window, fb, dct = self._tables(x.device, x.dtype)
            spec = torch.stft(x, 321, hop_length=160, win_length=321, window=window, center=True, pad_mode="reflect",
                              normalized=False, onesided=True, return_complex=True)          # (N, 161, F)
            power = spec.real ** 2 + spec.imag ** 2
            db = 10.0 * torch.log10(torch.clamp(torch.matmul(power.transpose(1, 2), fb), min=1e-10))      # (N, F, M)
            top = db.amax(dim=(1, 2), keepdim=True) if self.topPerRow else db.amax()
            return torch.matmul(torch.maximum(db, top - 80.0), dct).permute(0, 2, 1)


class NoAr(nn.Module):
    """cpc/model.py:207-213 (--arMode no_ar): the identity.  ``hip`` / ``reverse`` / ``keepHidden`` / ``hidden`` are there for the
    code that reads or sets them on any autoregressor (the fused step's check, the evaluation scripts' keepHidden)."""

    def __init__(self, *args):
        super().__init__()
        self.hip = False
        self.reverse = False
        self.keepHidden = False
        self.hidden = None

    def forward(self, x):
        return x


class CPCAR(nn.Module):
    """cpc/model.py:155-204.  For the GRU of the north-star configuration (256 -> 256) baseNet is a torch.nn.GRU used as the
    parameter container (same keys / gate layout) and forward runs cpc_gru_forward (HIP, ``self.hip``).  The reference's other
    autoregressors -- ``LSTM`` (its argparse default, cpc_default_config.py:74), ``RNN``, other widths -- run through baseNet's
    own torch forward: same semantics incl. the carried hidden state, any device, not the hot path.
    ``lstmKernel=True`` (not in the reference's signature; default off) runs the LSTM of 256 -> 256 through cpc_lstm_forward
    (HIP, ``self.hip_lstm``) for CUDA fp32 input; baseNet stays the nn.LSTM parameter container.  ``rnnKernel=True`` does the same
    for mode ``RNN``: nn.RNN(256, 256, nLevelsGRU, batch_first=True) of 1..8 layers through cpc_rnn_forward (HIP,
    ``self.hip_rnn``), baseNet the nn.RNN parameter container.  ``self.hip`` keeps meaning the GRU kernel (what the fused train
    step checks).
    ``inputKernel=True`` (default off, as the two above) takes an encoder width other than 256 -- 1 <= dimEncoded <= 512,
    dimOutput == 256, 1..8 layers: MFCC at 13 / 40 / 80 coefficients, the learned filter bank at 64, CPCEncoder(512) -- to the
    same HIP recurrences for CUDA fp32 input (``self.hip_in``): layer 0's input projection runs at its true width
    (csrc/in_proj.hip, cpc_*_forward_in).  Mode GRU needs nothing else; LSTM and RNN also need their own keyword.  ``self.hip``,
    ``self.hip_lstm`` and ``self.hip_rnn`` stay False at such a width: they keep meaning the 256 -> 256 kernels.
    ``hiddenKernel=True`` (default off) takes a context width other than 256 -- 1 <= dimOutput <= 512, any dimEncoded in
    1..512, 1..8 layers: --hiddenGar 512 -- to the kernels of any hidden width for CUDA fp32 input.  Mode LSTM (with
    ``lstmKernel=True``, as above) runs ops.LstmHiddenFunction (cpc_lstm_forward_h; ``self.hip_hidden``, which keeps meaning the
    LSTM kernels).  Mode GRU needs nothing else -- ``inputKernel``'s rule -- and runs ops.GruHiddenFunction (cpc_gru_forward_h;
    ``self.hip_gru_hidden``); that is the one combination whose path the keyword changes for a GRU: (GRU, ``hiddenKernel=True``,
    dimOutput != 256) leaves nn.GRU's torch forward for the HIP recurrence.  The four attributes above stay False in both cases.
    The RNN at another context width keeps running baseNet's torch forward."""

    def __init__(self, dimEncoded, dimOutput, keepHidden, nLevelsGRU, mode="GRU", reverse=False, lstmKernel=False,
                 rnnKernel=False, inputKernel=False, hiddenKernel=False):
        super().__init__()
        self.RESIDUAL_STD = 0.1
        self._cell = mode if mode in ("LSTM", "RNN") else "GRU"
        self.hip_in = (bool(inputKernel) and dimOutput == 256 and dimEncoded != 256 and 1 <= dimEncoded <= ops.IN_PROJ_MAX
                       and 1 <= nLevelsGRU <= 8
                       and (self._cell == "GRU" or bool(lstmKernel if self._cell == "LSTM" else rnnKernel)))
        self.hip = mode not in ("LSTM", "RNN") and dimEncoded == 256 and dimOutput == 256
        self.hip_lstm = bool(lstmKernel) and mode == "LSTM" and dimEncoded == 256 and dimOutput == 256
        self.hip_rnn = (bool(rnnKernel) and mode == "RNN" and dimEncoded == 256 and dimOutput == 256
                        and 1 <= nLevelsGRU <= 8)
        self.hip_hidden = (bool(hiddenKernel) and bool(lstmKernel) and mode == "LSTM" and dimOutput != 256
                           and 1 <= dimOutput <= ops.LSTM_HIDDEN_MAX and 1 <= dimEncoded <= ops.IN_PROJ_MAX
                           and 1 <= nLevelsGRU <= 8)
        self.hip_gru_hidden = (bool(hiddenKernel) and self._cell == "GRU" and dimOutput != 256
                               and 1 <= dimOutput <= ops.GRU_HIDDEN_MAX and 1 <= dimEncoded <= ops.IN_PROJ_MAX
                               and 1 <= nLevelsGRU <= 8)
        cell = nn.LSTM if mode == "LSTM" else (nn.RNN if mode == "RNN" else nn.GRU)
        self.baseNet = cell(dimEncoded, dimOutput, num_layers=nLevelsGRU, batch_first=True)
        self.hidden = None
        self.keepHidden = keepHidden
        self.reverse = reverse

    def getDimOutput(self):
        return self.baseNet.hidden_size

    def _flat_params(self):
        out = []
        for l in range(self.baseNet.num_layers):
            out += [getattr(self.baseNet, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return out

    def forward(self, x):
        """(B, S, 256) -> (B, S, 256).  In reverse mode the sequence is processed back to front and handed back in its
        original order (cpc/model.py:185-204); the final hidden state is kept for the next call when keepHidden is set."""
        flip = (lambda t: torch.flip(t, [1])) if self.reverse else (lambda t: t)
        narrow = self.hip_in and x.is_cuda and x.dtype == torch.float32      # (another input width: the same Functions, cpc_*_in)
        if (self.hip_lstm or self.hip_hidden or narrow and self._cell == "LSTM") and x.is_cuda and x.dtype == torch.float32:
            fn = LstmHiddenFunction if self.hip_hidden else LstmFunction
            y, hN, cN = fn.apply(flip(x), self.hidden, False, *self._flat_params())
            if self.keepHidden:
                self.hidden = (hN.detach(), cN.detach())
            out = flip(y)
            # |h_t| = |o * tanh(c_t)| <= 1 at every step whatever (h0, c0) is: unlike the GRU, whose h_t mixes in h_{t-1},
            # the output never carries the initial state through, so no check of where self.hidden came from is needed
            out._cpc_abs_bound = 1.0
            return out
        if (self.hip_rnn or narrow and self._cell == "RNN") and x.is_cuda and x.dtype == torch.float32:
            y, hN = RnnFunction.apply(flip(x), self.hidden, False, False, *self._flat_params())
            if self.keepHidden:
                self.hidden = hN.detach()
            out = flip(y)
            out._cpc_abs_bound = 1.0                           # |tanh| <= 1 whatever h0 is
            return out
        if self.hip_gru_hidden and x.is_cuda and x.dtype == torch.float32:
            # the 256 GRU's rule below: |h_t| <= 1 from zero or from the module's own last state only
            bounded = self.hidden is None or self.hidden is getattr(self, "_own_hidden", None)
            y, h_last = GruHiddenFunction.apply(flip(x), self.hidden, False, *self._flat_params())
            if self.keepHidden:
                self.hidden = self._own_hidden = h_last.detach()
            out = flip(y)
            if bounded:
                out._cpc_abs_bound = 1.0
            return out
        if not (self.hip or narrow):                           # cpc/model.py:185-204 with baseNet's own torch forward
            y, h = self.baseNet(flip(x), self.hidden)
            if self.keepHidden:
                self.hidden = tuple(t.detach() for t in h) if isinstance(h, tuple) else h.detach()
            return flip(y)
        # |h_t| <= 1 holds when the recurrence starts from zero or from one of its OWN final states (a convex combination of
        # tanh outputs and the previous state); a state assigned from outside carries no such bound
        bounded = self.hidden is None or self.hidden is getattr(self, "_own_hidden", None)
        y, h_last = GruFunction.apply(flip(x), self.hidden, *self._flat_params())
        if self.keepHidden:
            self.hidden = self._own_hidden = h_last.detach()
        out = flip(y)
        if bounded:
            out._cpc_abs_bound = 1.0      # read by CPCUnsupersivedCriterion.forward: the a-priori operand bound of its fp16-piece
            #                               GEMMs applies to THIS tensor only (anything derived from it loses the tag)
        return out


class CPCModel(nn.Module):
    """cpc/model.py:276-289."""

    def __init__(self, encoder, AR):
        super().__init__()
        self.gEncoder = encoder
        self.gAR = AR

    def forward(self, batchData, label):
        encodedData = self.gEncoder(batchData).permute(0, 2, 1)
        cFeature = self.gAR(encodedData)
        return cFeature, encodedData, label
