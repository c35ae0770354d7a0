"""torch.autograd.Function wrappers over the C ABI (include/cpc_hip.h).

Each Function is one node of the autograd graph for a whole stage of the hot path
(encoder / autoregressor / criterion), so the Python overhead per train step is three
forward and three backward calls.  All device memory (outputs, saved activations,
scratch) comes from torch's caching allocator; kernels are enqueued on torch's current
stream of the input's device.  There is no CPU implementation: CPU tensors raise.
"""
import ctypes
import os
from contextlib import nullcontext as _nullcontext

import torch

from . import _lib
from ._lib import ptr as _p

_HID = 256


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"cpc_audio_amd.{what}: expected a tensor on an AMD GPU (got {t.device}); "
                           "this package has no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"cpc_audio_amd.{what}: fp32 expected, got {t.dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


_layout_cache = {}


def check_device_errors(clear=True):
    """Raise if a kernel of this library flagged an error on the current device since the last check (include/cpc_hip.h,
    cpc_device_error_flags): a persistent-recurrence workgroup that gave up polling, a negative index out of range.
    Synchronises with the device -- the train loops call it where they already synchronise (logging, epoch end)."""
    mask = _lib.get().cpc_device_error_flags(1 if clear else 0)
    if mask < 0:
        raise _lib.CpcHipError("cpc_device_error_flags could not read the device flags")
    what = []
    if mask & 1:
        what.append("a workgroup of the persistent GRU recurrence timed out waiting for its neighbours "
                    "(outputs contain NaN from that step on)")
    if mask & 2:
        what.append("cpc_nce_prepare received negative-sample indices outside [0,B) x [0,S) (they were clamped)")
    if mask & 4:
        what.append("a workgroup of the N-split conv forward timed out waiting for its partner's ChannelNorm statistics "
                    "(its rows contain NaN)")
    if mask & 8:
        what.append("a workgroup of the persistent LSTM recurrence timed out waiting for its neighbours "
                    "(outputs contain NaN from that step on)")
    if mask & 16:
        what.append("a supervised criterion received a label outside its class range (it was clamped; the loss is NaN)")
    if mask & 32:
        what.append("an ABX plan named a segment or size out of range (it was clamped; that score is NaN)")
    if mask & 64:
        what.append("a PER decode or alignment received a length outside its row or a blank outside [0, P) (that score is NaN)")
    if mask & 128:
        what.append("the phone classifier's CTC loss or seqNorm received an input or target length outside its range (it was "
                    "clamped; that sequence's loss is NaN)")
    if mask & 256:
        what.append("a workgroup of a persistent Elman RNN recurrence timed out waiting for its neighbours "
                    "(outputs contain NaN from that step on)")
    if what:
        raise _lib.CpcHipError("device-side error: " + "; ".join(what))

# ---- stream-level overlap inside one train step ---------------------------------------------------------------------
# The dz half of the criterion's backward (per-destination gather-GEMM + one dense GEMM) is not on the way to dc, and
# the network that consumes dc (the persistent GRU backward: 128 workgroups, latency-bound) leaves most of the chip
# idle; the weight-gradient GEMMs hang off the dx chain.  A train loop that wants them on side streams owns a
# StepContext and runs forward + backward inside ``with ctx:``.  All overlap state (events, launches held back)
# lives on that object -- only the side streams are per process, see _side_streams -- so two loops on two threads / devices (nn.DataParallel-style
# replicas) do not see each other.  The Functions pick the context up in forward (on the caller's
# thread) and carry it to backward on their autograd ctx: autograd runs backward on its own worker thread.
# Without an active context every Function is single-stream.
import threading

_tls = threading.local()


MAX_STREAM_CANDIDATES = 12


def streams_overlap(a, b):
    """True if a kernel on stream ``b`` runs while stream ``a`` is busy, i.e. the two do not share a hardware queue
    (cpc_streams_overlap: a ~3 ms blocking probe)."""
    lib = _lib.get()
    out = ctypes.c_int(0)
    lib.check(lib.cpc_streams_overlap(ctypes.c_void_p(a.cuda_stream), ctypes.c_void_p(b.cuda_stream), ctypes.byref(out)),
              "streams_overlap")
    return bool(out.value)


def pick_concurrent_stream(device, priority, beside):
    """A pooled stream that really executes beside every stream in ``beside``.  The HIP runtime maps streams onto four hardware
    queues per priority level in creation order (measured with this probe: torch's pool streams 1..6 pair up as (1,6) (2,5) (3,4)
    in a fresh process; after init_process_group("nccl"), which creates six streams of its own, the default stream shares a queue
    with pool stream 4), and two streams on one queue run in submission order whatever their events say.  Draw from torch's
    pool until the probe says the candidate overlaps with all of ``beside`` (at most MAX_STREAM_CANDIDATES draws, ~3 ms per
    probe, once per process); if none does, the last one is used and a warning names the cost.  During a stream capture nothing
    can be probed: plain draw.  CPC_STREAM_PROBE=0 switches the probe off."""
    st = torch.cuda.Stream(device=device, priority=priority)
    if os.environ.get("CPC_STREAM_PROBE", "1") == "0" or torch.cuda.is_current_stream_capturing():
        return st
    with torch.cuda.device(device):
        for n in range(MAX_STREAM_CANDIDATES):
            if all(streams_overlap(o, st) for o in beside):
                return st
            if n + 1 < MAX_STREAM_CANDIDATES:
                st = torch.cuda.Stream(device=device, priority=priority)
    import warnings
    warnings.warn(f"no stream found that runs beside the step's other streams after {MAX_STREAM_CANDIDATES} draws: the overlapped "
                  "parts of the train step will run in submission order (slower, not wrong)")
    return st


# The side streams themselves are per process and device, shared by every StepContext: a second train loop in the process (a
# second Trainer, the bench's bf16 pass) has nothing to gain from more of them (four hardware queues serve them all).  Two loops on two threads then
# enqueue on the same side streams: each orders its own work with its own events, the streams only add FIFO order between them.
# What two threads must NOT share is the MAIN stream: the C side's pooled events are keyed by it (csrc/capi.hip, stream_events),
# and a record of one thread between another's record and wait re-targets that wait -- with the shared side streams behind
# it, possibly in a circle.  Every step is therefore issued under a claim on (device, current stream), see issuing_step.
_side_streams = {}
_side_streams_lock = threading.Lock()
_issuing = {}                       # (device index, stream handle) -> [thread ident, depth] while a step is being issued
_issuing_lock = threading.Lock()


class issuing_step:
    """``with issuing_step(device):`` around the host-side issue of one train step (StepContext.__enter__ .. __exit__, the
    composite step's calls).  A second thread that starts issuing on the same device AND the same current stream meanwhile
    gets a RuntimeError instead of a step whose stream order is undefined: concurrent train loops on one device (threaded
    data-parallel replicas) each need a stream of their own -- ``with torch.cuda.stream(torch.cuda.Stream()):`` around the loop
    (tests/test_gpu_modules.py::test_two_trainers_on_two_threads_...).  The same thread may nest."""

    def __init__(self, device=None):
        self.device, self.key = device, None

    def __enter__(self):
        if not torch.cuda.is_available():
            return self
        dev = torch.cuda.current_device() if self.device is None else torch.device(self.device).index
        if dev is None:
            dev = torch.cuda.current_device()
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        me = threading.get_ident()
        with _issuing_lock:
            held = _issuing.get(key)
            if held is not None and held[0] != me:
                raise RuntimeError(f"cpc_audio_amd: two threads are issuing train steps on the same stream of cuda:{dev}; give "
                                   "every concurrent train loop its own stream (with torch.cuda.stream(torch.cuda.Stream()): ...)")
            if held is None:
                _issuing[key] = [me, 1]
            else:
                held[1] += 1
        self.key = key
        return self

    def __exit__(self, *exc):
        if self.key is not None:
            with _issuing_lock:
                held = _issuing.get(self.key)
                if held is not None:
                    held[1] -= 1
                    if held[1] <= 0:
                        del _issuing[self.key]
            self.key = None
        return False


def _new_side_stream(key, device, which):
    # All side streams at normal priority.  Round 4 ran the weight-gradient stream at high priority for a while -- its last
    # kernel, layer 1's weight gradient, is the tail of the step, and with priority its workgroups are dispatched ahead of
    # conv0's backward beside it: 2.865-2.873 vs 2.880-2.884 ms per step sustained on one box, no difference on another -- but
    # a high-priority stream gets a hardware queue of its own, and that queue must not be the process's FIFTH.  ROCclr's log
    # (AMD_LOG_LEVEL=3) of a run that had touched the GPU before init_process_group("nccl"): the default stream creates queue
    # 1, RCCL's streams queues 2-4 (the normal-priority pool is full at four), the side streams share those, the
    # high-priority stream creates queue 5 -- after which every kernel of the main stream on queue 1 runs 20-40 us longer,
    # alone or not, and the step takes 4.6 ms instead of 2.9 (the same with the roles mirrored, with all side streams at high
    # priority, or with GPU_MAX_HW_QUEUES=8; with the priority dropped, or GPU_MAX_HW_QUEUES <= 3, 2.89 ms in every creation
    # order).  A graph capture's warm-up stream, a second train loop or a caller's own stream would be a fifth queue just the
    # same; with normal-priority streams only, the process stays within the four queues of the normal pool whatever else it
    # creates.  CPC_SIDE_PRIORITY="2"-style lists of `which` opt back in (A/B runs).
    env = os.environ.get("CPC_SIDE_PRIORITY")
    hi = env is not None and str(which) in env.split(",")
    beside = [torch.cuda.current_stream(device)] + [v for k, v in _side_streams.items() if k[0] == key[0]]
    return pick_concurrent_stream(device, -1 if hi else 0, beside)


def _process_side_stream(key, device, which):
    with _side_streams_lock:
        st = _side_streams.get(key)
        if st is None:
            st = _side_streams[key] = _new_side_stream(key, device, which)
        return st


class StepContext:
    """Overlap state of one train loop.  ``overlap``: the criterion's dz path and head gradient on a side stream;
    ``wgrad_stream`` (with overlap): the encoder's / recurrence's weight-gradient GEMMs on their own stream."""

    def __init__(self, overlap=True, wgrad_stream=True):
        self.overlap = bool(overlap)
        self.wgrad_stream = bool(wgrad_stream)
        self._streams = {}
        self.side_events = []       # work the next backward op depends on (dz)
        self.late_events = []       # work only the optimiser reads (the prediction heads' weight gradient)
        self.wgrad_events = []      # the same on the weight-gradient stream (the recurrence's weight / bias gradients)
        self.deferred = []          # side-stream launches held back until the AR backward is in flight (it needs whole
        #                             CUs: its 768-thread workgroups cannot squeeze in beside a chip full of gather blocks)
        self.pre_encoder_backward = []   # callables(ctx) run when the encoder's backward starts: every other gradient
        #                             of the step is final (or queued on the side stream) by then -- FlatGradAllReduce.begin
        self.prepared = None        # what the criterion queued on the side stream at the start of the step
        #                             (CPCUnsupersivedCriterion.prepare_step): negative draws, index preparation, GEMM bounds

    def side_stream(self, device, which=0):
        """which = 0: the criterion's stream (negative draws, dz path, head gradient, early all-reduce bucket);
        1: forward-only preparation of the recurrence's backward (it must not queue in front of the negative draws);
        2: weight gradients."""
        key = (torch.device(device).index, which)
        st = self._streams.get(key)
        if st is None:
            st = self._streams[key] = _process_side_stream(key, device, which)
        return st

    def reserve(self, device):
        """Create the three side streams now.  Hardware queues are handed out in creation order and a process should not need
        more than four (side_stream above): streams created before init_process_group get queues of
        their own, RCCL's then share the fourth."""
        with torch.cuda.device(device):
            return [self.side_stream(device, which) for which in range(3)]

    def abandon(self):
        """After an exception inside an overlapped step: forget the launches still held back and the events not yet
        waited for (what was already enqueued simply completes), so that the next step does not start from stale state."""
        del self.deferred[:]
        del self.side_events[:]
        del self.late_events[:]
        del self.wgrad_events[:]
        self.prepared = None

    def launch_deferred(self):
        while self.deferred:
            self.deferred.pop(0)()

    def wait(self, final=True, wgrad=None):
        """Make the current stream wait for everything launched (or still held) for the side streams.  ``final=False``
        (used between the backward ops) leaves out what only the optimiser reads; the owner calls this with
        final=True after backward() and before touching any ``.grad``.  ``wgrad`` (default: same as ``final``): also
        wait for the weight-gradient stream."""
        self.launch_deferred()
        cur = torch.cuda.current_stream()
        while self.side_events:
            cur.wait_event(self.side_events.pop())
        while final and self.late_events:
            cur.wait_event(self.late_events.pop())
        while (final if wgrad is None else wgrad) and self.wgrad_events:
            cur.wait_event(self.wgrad_events.pop())

    def __enter__(self):
        claim = issuing_step()
        claim.__enter__()                                 # (raises before anything of this context is touched)
        try:
            # where the step starts on the caller's stream: side-stream work that depends on nothing of the step (the negative
            # draws) forks from HERE -- early enough to run beside the encoder, and an explicit fork, which a stream capture
            # (train.Trainer(graph=True)) needs to see the side stream's work as part of the step
            begin = None
            if self.overlap and torch.cuda.is_available():
                begin = torch.cuda.Event()
                begin.record()
        except BaseException as e:
            # __exit__ does not run when __enter__ raises: give the (device, stream) claim back here, or every other thread
            # is refused on this stream until the process ends
            claim.__exit__(type(e), e, e.__traceback__)
            raise
        self._claim, self.begin = claim, begin
        self._prev = getattr(_tls, "ctx", None)
        _tls.ctx = self
        return self

    def __exit__(self, et, ev, tb):
        _tls.ctx = self._prev
        self._claim.__exit__(et, ev, tb)
        if et is not None:
            self.abandon()
        return False


def current():
    """The StepContext active on this thread (None: single-stream)."""
    return getattr(_tls, "ctx", None)


def _overlap(step):
    return step is not None and step.overlap


def _wait(step, **kw):
    if step is not None:
        step.wait(**kw)


_VIEW_NODES = ("PermuteBackward0", "TransposeBackward0", "ViewBackward0", "UnsafeViewBackward0", "AliasBackward0")
_OWN_WAITING_NODES = ("GruFunctionBackward", "TransformerLayerFunctionBackward")


def dz_may_be_deferred(c, z):
    """Whether InfoNCEFunction.backward may hand autograd a dz that is filled later, on the side stream.  True only
    when this package can prove nobody reads it earlier: z reaches EncoderFunction through pure views (its backward
    waits first), and the other consumer of z -- the network that made c -- ends in one of this package's Functions
    (their backward waits before returning dx, which autograd then adds to dz).  Anything else -- criterion mode
    'reverse' puts a torch.flip between the criterion and the encoder, a foreign autoregressor -- gets dz on the
    current stream right away."""
    fn = z.grad_fn
    while fn is not None and type(fn).__name__ in _VIEW_NODES:
        fn = fn.next_functions[0][0]
    if fn is not None and type(fn).__name__ != "EncoderFunctionBackward":
        return False
    fn = c.grad_fn
    while fn is not None and type(fn).__name__ in _VIEW_NODES + ("FlipBackward0", "SliceBackward0"):
        fn = fn.next_functions[0][0]
    return fn is None or type(fn).__name__ in _OWN_WAITING_NODES

# Parity tests set KEEP_DEBUG = True to look at the encoder's saved activations (the ReLU
# masks of the device path, see oracle/cpc_oracle._ReluTieAware).  Never used by the product.
KEEP_DEBUG = False
debug_last = {}


def _layout(kind, fn, n, *args):
    key = (kind,) + args
    v = _layout_cache.get(key)
    if v is None:
        sizes = (ctypes.c_long * n)()
        _lib.Bound.check(fn(*args, sizes), kind)
        v = tuple(sizes)
        _layout_cache[key] = v
    return v


def _layout_takes(kind, *args):
    """Does the layout entry cpc_<kind> take this shape?  (_layout raises ValueError for one it refuses)"""
    try:
        _layout(kind, getattr(_lib.get(), "cpc_" + kind), 3, *(int(a) for a in args))
    except ValueError:
        return False
    return True


def saved_encoder_activations(saved, B, L):
    """fp32 copies (B, L_i, 256) of the four intermediate activations y0..y3 an EncoderFunction forward left in ``saved``
    (layers 0 and 1 are kept as two fp16 pieces per element in the default mode).  Parity tests only."""
    lib = _lib.get()
    with torch.cuda.device(saved.device) if saved.is_cuda else _nullcontext():
        sizes = _layout("encoder_layout", lib.cpc_encoder_layout, 22, B, L)
        out = []
        for i in range(4):
            y = torch.empty(B, sizes[3 + i], _HID, device=saved.device, dtype=torch.float32)
            lib.check(lib.cpc_encoder_saved_activation(_p(saved), i, _p(y), B, L, _stream() if saved.is_cuda else None),
                      "encoder_saved_activation")
            out.append(y)
    return out


class EncoderFunction(torch.autograd.Function):
    """wave (B,1,L) + the 20 encoder parameters (state-dict order) -> z (B, L/160, 256)."""

    @staticmethod
    def forward(ctx, wave, *params):
        _require_cuda(wave, "EncoderFunction")
        lib = _lib.get()
        B, ch, L = wave.shape
        if ch != 1:
            raise ValueError("CPCEncoder expects (B,1,L) waveforms")
        wave = wave.contiguous()
        params = [p.detach().contiguous() for p in params]
        with torch.cuda.device(wave.device):
            sizes = _layout("encoder_layout", lib.cpc_encoder_layout, 22, B, L)
            saved = torch.empty(sizes[0], device=wave.device, dtype=torch.float32)
            scratch = torch.empty(max(1, sizes[1]), device=wave.device, dtype=torch.float32)
            z = torch.empty(B, sizes[7], _HID, device=wave.device, dtype=torch.float32)
            lib.check(lib.cpc_encoder_forward(_p(wave), _ptrs(params), _p(saved), _p(scratch), _p(z), B, L,
                                              _stream()), "encoder_forward")
        ctx.save_for_backward(wave, saved, z, *params)
        ctx.dims = (B, L, sizes[2])
        ctx.step = current()
        if KEEP_DEBUG:
            debug_last["encoder"] = (saved, sizes, z)
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.get()
        # dz may carry the criterion's side-stream part.  The weight-gradient stream is not waited for here: the call
        # below runs its own GEMMs there and joins it before it returns.
        step = ctx.step
        _wait(step, final=False)
        if step is not None:
            for hook in step.pre_encoder_backward:
                hook(step)
        wave, saved, z, *params = ctx.saved_tensors
        B, L, nscr = ctx.dims
        dz = dz.contiguous()
        with torch.cuda.device(wave.device):
            scratch = torch.empty(nscr, device=wave.device, dtype=torch.float32)
            grads = [torch.empty_like(p) for p in params]
            if _overlap(step) and step.wgrad_stream:
                # the weight-gradient GEMMs beside the dx chain (its norm backwards stream, conv0's backward is
                # VALU-bound: both leave the matrix pipes idle); the call joins the two streams before it returns
                lib.check(lib.cpc_encoder_backward_streams(_p(wave), _ptrs(params), _p(saved), _p(z), _p(dz), _p(scratch),
                                                           _ptrs(grads), B, L, _stream(),
                                                           step.side_stream(wave.device, 2).cuda_stream), "encoder_backward")
            else:
                lib.check(lib.cpc_encoder_backward(_p(wave), _ptrs(params), _p(saved), _p(z), _p(dz), _p(scratch),
                                                   _ptrs(grads), B, L, _stream()), "encoder_backward")
        _wait(step)                            # the last backward op: everything on the side stream is due now
        return (None, *grads)


ENCODER_WIDE_MAX = 512  # widest CPCEncoder of the encoder kernels of any width (cpc_encoder_*_c; csrc/enc_wide.hip)


class EncoderWideFunction(torch.autograd.Function):
    """wave (B,1,L) + the 20 encoder parameters (state-dict order, C channels, 2 <= C <= 512) -> z (B, L/160, C), contiguous:
    cpc_encoder_forward_c / _backward_c (csrc/enc_wide.hip; C == 256 runs the 256 kernels behind the same entries).  A plain
    autograd node on the current stream: no step hooks, no side streams.  The wave receives no gradient."""

    @staticmethod
    def forward(ctx, wave, *params):
        _require_cuda(wave, "EncoderWideFunction")
        lib = _lib.get()
        B, ch, L = wave.shape
        if ch != 1 or len(params) != 20:
            raise ValueError("EncoderWideFunction expects (B,1,L) waveforms and the 20 encoder parameters")
        C = params[0].shape[0]
        want = []
        for i, k in enumerate((10, 8, 4, 4, 4)):
            want += [(C, 1 if i == 0 else C, k), (C,), (1, C, 1), (1, C, 1)]
        if not 2 <= C <= ENCODER_WIDE_MAX or [tuple(p.shape) for p in params] != want:
            raise NotImplementedError(f"cpc_audio_amd.EncoderWideFunction: 2 <= sizeHidden <= {ENCODER_WIDE_MAX} and the "
                                      f"reference's parameter shapes expected (conv0.weight {tuple(params[0].shape)})")
        wave = wave.contiguous()
        params = [p.detach().contiguous() for p in params]
        with torch.cuda.device(wave.device):
            sizes = _layout("encoder_layout_c", lib.cpc_encoder_layout_c, 22, B, L, C)
            saved = torch.empty(sizes[0], device=wave.device, dtype=torch.float32)
            scratch = torch.empty(max(1, sizes[1]), device=wave.device, dtype=torch.float32)
            z = torch.empty(B, sizes[7], C, device=wave.device, dtype=torch.float32)
            lib.check(lib.cpc_encoder_forward_c(_p(wave), _ptrs(params), _p(saved), _p(scratch), _p(z), B, L, C, _stream()),
                      "encoder_forward_c")
        ctx.save_for_backward(wave, saved, z, *params)
        ctx.dims = (B, L, C, sizes[2])
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.get()
        wave, saved, z, *params = ctx.saved_tensors
        B, L, C, nscr = ctx.dims
        dz = dz.contiguous()
        with torch.cuda.device(wave.device):
            scratch = torch.empty(nscr, device=wave.device, dtype=torch.float32)
            grads = [torch.empty_like(p) for p in params]
            lib.check(lib.cpc_encoder_backward_c(_p(wave), _ptrs(params), _p(saved), _p(z), _p(dz), _p(scratch), _ptrs(grads),
                                                 B, L, C, _stream()), "encoder_backward_c")
        return (None, *grads)


ENCODER_NORM_CODES = {"layerNorm": 0, "batchNorm": 1, "instanceNorm": 2, "ID": 3}      # `norm` of the cpc_encoder_*_n entries


class EncoderNormFunction(torch.autograd.Function):
    """wave (B,1,L), normMode, training, the ten running buffers (batchNorm: running_mean / running_var of layers 0..4; None
    otherwise), momentum, eps + the encoder parameters in state-dict order -> z (B, L/160, C), contiguous: cpc_encoder_forward_n /
    _backward_n (csrc/enc_wide.hip), 2 <= C <= 512.  The parameters are 20 under batchNorm / instanceNorm (norm weight
    and bias of shape (C,)) and the 10 conv tensors under ID.  A plain autograd node on the current stream, as
    EncoderWideFunction.  Under batchNorm in training the running buffers are updated in place by the forward call, once, outside
    the graph; num_batches_tracked is the module's to count.  The wave receives no gradient."""

    @staticmethod
    def forward(ctx, wave, normMode, training, running, momentum, eps, *params):
        _require_cuda(wave, "EncoderNormFunction")
        lib = _lib.get()
        B, ch, L = wave.shape
        norm = ENCODER_NORM_CODES[normMode]
        ident = normMode == "ID"
        if ch != 1 or norm == 0 or len(params) != (10 if ident else 20):
            raise ValueError("EncoderNormFunction expects (B,1,L) waveforms, normMode batchNorm / instanceNorm / ID and the "
                             "encoder's parameters in state-dict order")
        C = params[0].shape[0]
        want = []
        for i, k in enumerate((10, 8, 4, 4, 4)):
            want += [(C, 1 if i == 0 else C, k), (C,)] + ([] if ident else [(C,), (C,)])
        if not 2 <= C <= ENCODER_WIDE_MAX or [tuple(p.shape) for p in params] != want:
            raise NotImplementedError(f"cpc_audio_amd.EncoderNormFunction: 2 <= sizeHidden <= {ENCODER_WIDE_MAX} and the "
                                      f"reference's parameter shapes expected (conv0.weight {tuple(params[0].shape)})")
        if normMode == "batchNorm" and (running is None or len(running) != 10 or any(
                r.shape != (C,) or r.dtype != torch.float32 or not r.is_contiguous() or r.device != wave.device for r in running)):
            raise ValueError("EncoderNormFunction: batchNorm needs the ten (C,) fp32 running buffers on the wave's device")
        wave = wave.contiguous()
        params = [p.detach().contiguous() for p in params]
        slots = params if not ident else [t for i in range(5) for t in (params[2 * i], params[2 * i + 1], None, None)]
        training = 1 if training else 0
        with torch.cuda.device(wave.device):
            sizes = _layout("encoder_layout_n", lib.cpc_encoder_layout_n, 32, B, L, C, norm, training)
            saved = torch.empty(max(1, sizes[0]), device=wave.device, dtype=torch.float32)
            scratch = torch.empty(max(1, sizes[1]), device=wave.device, dtype=torch.float32)
            z = torch.empty(B, sizes[7], C, device=wave.device, dtype=torch.float32)
            lib.check(lib.cpc_encoder_forward_n(_p(wave), _ptrs(slots), _ptrs(list(running)) if normMode == "batchNorm" else None,
                                                _p(saved), _p(scratch), _p(z), B, L, C, norm, training, float(momentum), float(eps),
                                                _stream()), "encoder_forward_n")
        ctx.save_for_backward(wave, saved, z, *params)
        ctx.dims = (B, L, C, norm, training, sizes[2])
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.get()
        wave, saved, z, *params = ctx.saved_tensors
        B, L, C, norm, training, nscr = ctx.dims
        ident = norm == ENCODER_NORM_CODES["ID"]
        dz = dz.contiguous()
        with torch.cuda.device(wave.device):
            scratch = torch.empty(nscr, device=wave.device, dtype=torch.float32)
            grads = [torch.empty_like(p) for p in params]
            pad = (lambda ts: ts) if not ident else (lambda ts: [t for i in range(5) for t in (ts[2 * i], ts[2 * i + 1], None, None)])
            lib.check(lib.cpc_encoder_backward_n(_p(wave), _ptrs(pad(params)), _p(saved), _p(z), _p(dz), _p(scratch),
                                                 _ptrs(pad(grads)), B, L, C, norm, training, _stream()), "encoder_backward_n")
        return (None, None, None, None, None, None, *grads)


IN_PROJ_MAX = 512      # widest layer-0 input of the recurrent cells (cpc_*_in; csrc/in_proj.hip)
LSTM_HIDDEN_MAX = 512  # widest hidden state of the LSTM at any hidden width (cpc_lstm_*_h; csrc/lstm.hip)


def _cell_input_width(x, params, gates, what):
    """The input width D of a cell whose weight_ih_l0 is (gates * 256, D) and weight_hh_l0 (gates * 256, 256)."""
    D = x.shape[2]
    if (not 1 <= D <= IN_PROJ_MAX or tuple(params[0].shape) != (gates * _HID, D)
            or params[1].numel() != gates * _HID * _HID):
        raise NotImplementedError(f"the HIP {what} is built for dimOutput == 256 and 1 <= dimEncoded <= {IN_PROJ_MAX} "
                                  f"(x {tuple(x.shape)}, weight_ih_l0 {tuple(params[0].shape)})")
    return D


class GruFunction(torch.autograd.Function):
    """x (B,S,D), h0 (nl,B,256) or None, 4*nl GRU parameters -> y (B,S,256), hN (nl,B,256).  D == 256 is the path of the fused
    step (prepared coefficients, weight gradients on their own stream); any other D in 1..512 -- weight_ih_l0 (768, D) -- runs
    cpc_gru_forward_in / _backward_in: layer 0's input projection in csrc/in_proj.hip, the same recurrences, one stream."""

    @staticmethod
    def forward(ctx, x, h0, *params):
        _require_cuda(x, "GruFunction")
        lib = _lib.get()
        B, S, D = x.shape
        nl = len(params) // 4
        leaves = params                           # the tensors autograd knows (normally the module's Parameters)
        D = _cell_input_width(x, params, 3, "GRU")
        x = x.contiguous()
        params = [p.detach().contiguous() for p in params]
        h0c = None if h0 is None else h0.detach().contiguous()
        if D != _HID:
            with torch.cuda.device(x.device):
                sizes = _layout("gru_layout_in", lib.cpc_gru_layout_in, 3, B, S, nl, D)
                saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
                scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
                y = torch.empty(B, S, _HID, device=x.device, dtype=torch.float32)
                hN = torch.empty(nl, B, _HID, device=x.device, dtype=torch.float32)
                lib.check(lib.cpc_gru_forward_in(_p(x), _p(h0c), _ptrs(params), _p(saved), _p(scratch), _p(y), _p(hN), B, S, nl, D,
                                                 _stream()), "gru_forward_in")
            ctx.step = current()
            ctx.coef = None
            ctx.leaves = None
            ctx.save_for_backward(x, saved, y, *params)
            ctx.h0 = h0c
            ctx.dims = (B, S, nl, sizes[2])
            ctx.mark_non_differentiable(hN)
            ctx.set_materialize_grads(False)
            return y, hN
        with torch.cuda.device(x.device):
            sizes = _layout("gru_layout", lib.cpc_gru_layout, 3, B, S, nl)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
            y = torch.empty(B, S, _HID, device=x.device, dtype=torch.float32)
            hN = torch.empty(nl, B, _HID, device=x.device, dtype=torch.float32)
            # train loops (an overlapping StepContext): everything of the two-layer backward that depends on the forward only is
            # prepared now -- the gate-derivative coefficients by the forward recurrence itself (its gate threads hold their
            # inputs in registers), the hand-over buffers and the transposed weights on a side stream beside the criterion's
            # forward -- instead of between the criterion's backward and the recurrence
            coef = None
            step = ctx.step = current()
            if _overlap(step) and nl == 2 and any(ctx.needs_input_grad):
                ncoef = lib.cpc_gru_coef_floats(B, S, nl)
                if ncoef > 0:
                    coef = torch.empty(ncoef, device=x.device, dtype=torch.float32)
                    # the side stream may touch this block only once the current stream has passed this point: the allocator
                    # hands out memory whose previous user may still be queued on the current stream
                    allocated = torch.cuda.Event()
                    allocated.record()
            lib.check(lib.cpc_gru_forward_coef(_p(x), _p(h0c), _ptrs(params), _p(saved), _p(scratch), _p(y), _p(hN), _p(coef),
                                               B, S, nl, _stream()), "gru_forward")
            if coef is not None:
                main, side = torch.cuda.current_stream(), step.side_stream(x.device, 1)
                side.wait_event(allocated)                       # (the work itself depends on the parameters only)
                lib.check(lib.cpc_gru_backward_coef(_p(h0c), _ptrs(params), _p(saved), _p(y), _p(coef), 1, B, S, nl,
                                                    side.cuda_stream), "gru_backward_coef")
                for t in (coef, *params):
                    t.record_stream(side)
                ctx.coef_ready = torch.cuda.Event()
                ctx.coef_ready.record(side)
        ctx.coef = coef
        ctx.leaves = list(leaves) if all(isinstance(q, torch.Tensor) and q.is_leaf for q in leaves) else None
        ctx.save_for_backward(x, saved, y, *params)
        ctx.h0 = h0c
        ctx.dims = (B, S, nl, sizes[2])
        ctx.mark_non_differentiable(hN)
        ctx.set_materialize_grads(False)       # no zero-filled gradient for hN on every step
        return y, hN

    @staticmethod
    def backward(ctx, dy, _dhN):
        lib = _lib.get()
        x, saved, y, *params = ctx.saved_tensors
        B, S, nl, nscr = ctx.dims
        dy = torch.zeros_like(y) if dy is None else dy.contiguous()
        with torch.cuda.device(x.device):
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            grads = [torch.empty_like(p) for p in params]
            if ctx.coef is not None:
                torch.cuda.current_stream().wait_event(ctx.coef_ready)
            step = ctx.step
            D = x.shape[2]
            split = _overlap(step) and step.wgrad_stream and nl == 2 and ctx.leaves is not None
            if D != _HID:
                lib.check(lib.cpc_gru_backward_in(_p(x), _p(ctx.h0), _ptrs(params), _p(saved), _p(y), _p(dy), _p(scratch), _p(dx),
                                                  _ptrs(grads), B, S, nl, D, _stream()), "gru_backward_in")
            elif split:
                # dx on this stream; the weight / bias gradients -- read by nobody before the optimiser -- on the
                # weight-gradient stream, beside the start of the encoder's backward.  They are added to .grad there
                # (autograd gets None for them: it would accumulate on this stream, before they exist).
                wst = step.side_stream(x.device, 2)
                lib.check(lib.cpc_gru_backward_streams(_p(x), _p(ctx.h0), _ptrs(params), _p(saved), _p(y), _p(dy),
                                                       _p(ctx.coef), _p(scratch), _p(dx), _ptrs(grads), B, S, nl,
                                                       _stream(), wst.cuda_stream), "gru_backward")
                with torch.cuda.stream(wst), torch.no_grad():
                    for leaf, g in zip(ctx.leaves, grads):
                        if not leaf.requires_grad:
                            continue
                        if leaf.grad is None:
                            leaf.grad = g.view_as(leaf)
                        else:
                            leaf.grad.add_(g.view_as(leaf))
                            leaf.grad.record_stream(wst)
                for t in [scratch, saved, x, y, dy] + grads + ([] if ctx.coef is None else [ctx.coef]):
                    t.record_stream(wst)
                ev = torch.cuda.Event()
                ev.record(wst)
                step.wgrad_events.append(ev)
                grads = [None] * len(grads)
            else:
                lib.check(lib.cpc_gru_backward_with_coef(_p(x), _p(ctx.h0), _ptrs(params), _p(saved), _p(y), _p(dy),
                                                         _p(ctx.coef), _p(scratch), _p(dx), _ptrs(grads), B, S, nl,
                                                         _stream()), "gru_backward")
        ctx.coef = None                # its hand-over buffers are consumed: a second backward through this node recomputes
        _wait(ctx.step, final=False)   # starts the criterion's deferred dz path beside the recurrence just launched, and makes
        #                         this stream wait for it: autograd adds dx to that dz next
        return (dx, None, *grads)


class LstmFunction(torch.autograd.Function):
    """x (B,S,256), state None or (h0, c0) (each (nl,B,256)), 4*nl LSTM parameters -> y (B,S,256), (hN, cN) (each (nl,B,256)).

    The carried state is an input only: neither h0 nor c0 receives a gradient (the reference detaches it between calls,
    cpc/model.py:194-198), and hN / cN are not differentiable.  per_step: the one-launch-per-step kernels instead of the
    persistent recurrence (same bits; tests).  x may be (B,S,D) with weight_ih_l0 (1024, D), 1 <= D <= 512: layer 0's input
    projection then runs in csrc/in_proj.hip (cpc_lstm_forward_in / _backward_in)."""

    @staticmethod
    def forward(ctx, x, state, per_step, *params):
        _require_cuda(x, "LstmFunction")
        lib = _lib.get()
        B, S, D = x.shape
        nl = len(params) // 4
        D = _cell_input_width(x, params, 4, "LSTM")              # (D != 256: weight_ih_l0 (1024, D), cpc_lstm_*_in)
        x = x.contiguous()
        params = [p.detach().contiguous() for p in params]
        h0, c0 = (None, None) if state is None else (state[0].detach().contiguous(), state[1].detach().contiguous())
        flags = 1 if per_step else 0                      # CPC_LSTM_PER_STEP
        with torch.cuda.device(x.device):
            sizes = _layout("lstm_layout_in", lib.cpc_lstm_layout_in, 3, B, S, nl, D) if D != _HID else \
                _layout("lstm_layout", lib.cpc_lstm_layout, 3, B, S, nl)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
            y = torch.empty(B, S, _HID, device=x.device, dtype=torch.float32)
            hN = torch.empty(nl, B, _HID, device=x.device, dtype=torch.float32)
            cN = torch.empty(nl, B, _HID, device=x.device, dtype=torch.float32)
            if D != _HID:
                lib.check(lib.cpc_lstm_forward_in(_p(x), _p(h0), _p(c0), _ptrs(params), _p(saved), _p(scratch), _p(y), _p(hN),
                                                  _p(cN), B, S, nl, D, flags, _stream()), "lstm_forward_in")
            else:
                lib.check(lib.cpc_lstm_forward(_p(x), _p(h0), _p(c0), _ptrs(params), _p(saved), _p(scratch), _p(y), _p(hN), _p(cN),
                                               B, S, nl, flags, _stream()), "lstm_forward")
        ctx.save_for_backward(x, saved, y, *params)
        ctx.state = (h0, c0)
        ctx.dims = (B, S, nl, sizes[2], flags)
        ctx.mark_non_differentiable(hN, cN)
        ctx.set_materialize_grads(False)
        return y, hN, cN

    @staticmethod
    def backward(ctx, dy, _dhN, _dcN):
        lib = _lib.get()
        x, saved, y, *params = ctx.saved_tensors
        B, S, nl, nscr, flags = ctx.dims
        h0, c0 = ctx.state
        dy = torch.zeros_like(y) if dy is None else dy.contiguous()
        with torch.cuda.device(x.device):
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            grads = [torch.empty_like(p) for p in params]
            if x.shape[2] != _HID:
                lib.check(lib.cpc_lstm_backward_in(_p(x), _p(h0), _p(c0), _ptrs(params), _p(saved), _p(y), _p(dy), _p(scratch),
                                                   _p(dx), _ptrs(grads), B, S, nl, x.shape[2], flags, _stream()), "lstm_backward_in")
            else:
                lib.check(lib.cpc_lstm_backward(_p(x), _p(h0), _p(c0), _ptrs(params), _p(saved), _p(y), _p(dy), _p(scratch), _p(dx),
                                                _ptrs(grads), B, S, nl, flags, _stream()), "lstm_backward")
        return (dx, None, None, *grads)


def _hidden_forward(ctx, cell, ng, x, states, per_step, params):
    """forward of GruHiddenFunction (cell "gru", ng = 3) and LstmHiddenFunction ("lstm", 4): checks, allocation and the
    cpc_<cell>_forward_h call.  states: the carried (nl,B,H) tensors -- h0, for the LSTM also c0 -- all None or all given; one
    final state per carried one comes back behind y."""
    name, mod = f"{cell.capitalize()}HiddenFunction", cell.upper()
    _require_cuda(x, name)
    lib = _lib.get()
    nl = len(params) // 4
    if x.dim() != 3 or nl < 1 or len(params) != 4 * nl or params[1].dim() != 2 or params[0].dim() != 2:
        raise NotImplementedError(f"cpc_audio_amd.{name}: x (B,S,D) and 4 parameters per nn.{mod} layer expected")
    B, S, D = x.shape
    H = params[1].shape[1]
    shapes = []
    for l in range(nl):
        shapes += [(ng * H, D if l == 0 else H), (ng * H, H), (ng * H,), (ng * H,)]
    if [tuple(p.shape) for p in params] != shapes or x.dtype != torch.float32:
        raise NotImplementedError(f"cpc_audio_amd.{name}: fp32 nn.{mod}({D}, {H}, {nl}) parameters expected, got "
                                  f"{[tuple(p.shape) for p in params]}")
    x = x.contiguous()
    params = [p.detach().contiguous() for p in params]
    states = [None if s is None else s.detach().contiguous() for s in states]
    if states[0] is not None and any(tuple(s.shape) != (nl, B, H) for s in states):
        raise NotImplementedError(f"cpc_audio_amd.{name}: carried state of shape {(nl, B, H)} expected")
    flags = 1 if per_step else 0                      # CPC_GRU_PER_STEP, CPC_LSTM_PER_STEP
    with torch.cuda.device(x.device):
        sizes = _layout(f"{cell}_layout_h", getattr(lib, f"cpc_{cell}_layout_h"), 3, B, S, nl, D, H)
        saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
        scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
        y = torch.empty(B, S, H, device=x.device, dtype=torch.float32)
        finals = [torch.empty(nl, B, H, device=x.device, dtype=torch.float32) for _ in states]
        lib.check(getattr(lib, f"cpc_{cell}_forward_h")(_p(x), *(_p(s) for s in states), _ptrs(params), _p(saved), _p(scratch),
                                                        _p(y), *(_p(f) for f in finals), B, S, nl, D, H, flags, _stream()),
                  f"{cell}_forward_h")
    ctx.save_for_backward(x, saved, y, *params)
    ctx.states = states
    ctx.dims = (B, S, nl, D, H, sizes[2], flags)
    ctx.mark_non_differentiable(*finals)
    ctx.set_materialize_grads(False)
    return (y, *finals)


def _hidden_backward(ctx, cell, dy):
    """backward of the two: the cpc_<cell>_backward_h call -> (dx, None for the carried state, None for per_step, *grads)"""
    lib = _lib.get()
    x, saved, y, *params = ctx.saved_tensors
    B, S, nl, D, H, nscr, flags = ctx.dims
    dy = torch.zeros_like(y) if dy is None else dy.contiguous()
    with torch.cuda.device(x.device):
        scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(p) for p in params]
        lib.check(getattr(lib, f"cpc_{cell}_backward_h")(_p(x), *(_p(s) for s in ctx.states), _ptrs(params), _p(saved), _p(y),
                                                         _p(dy), _p(scratch), _p(dx), _ptrs(grads), B, S, nl, D, H, flags,
                                                         _stream()), f"{cell}_backward_h")
    return (dx, None, None, *grads)


def _hidden_paths(cell, clear):
    mask = getattr(_lib.get(), f"cpc_{cell}_paths_h")(1 if clear else 0)
    return {name for bit, name in ((1, "persistent"), (2, "per_step")) if mask & bit}


class LstmHiddenFunction(torch.autograd.Function):
    """nn.LSTM(D, H, nl, batch_first=True) at any hidden width: x (B,S,D), state None or (h0, c0) (each (nl,B,H)), 4*nl LSTM
    parameters at their true shapes -> y (B,S,H), (hN, cN) (each (nl,B,H)), 1 <= D, H <= 512 (cpc_lstm_forward_h / _backward_h:
    the recurrence runs at the padded width 128 * ceil(H / 128) on zero-padded weight copies; with H == 256 the entries are
    cpc_lstm_*_in).  Same calling convention as LstmFunction: the carried state gets no gradient, hN / cN are not
    differentiable, per_step selects the one-launch-per-step kernels (same bits)."""

    @staticmethod
    def forward(ctx, x, state, per_step, *params):
        return _hidden_forward(ctx, "lstm", 4, x, (None, None) if state is None else state, per_step, params)

    @staticmethod
    def backward(ctx, dy, _dhN, _dcN):
        return _hidden_backward(ctx, "lstm", dy)


def lstm_hidden_paths(clear=True):
    """Which recurrence kernels LstmHiddenFunction has launched since the last clearing call: a set out of "persistent" and
    "per_step" (cpc_lstm_paths_h; per_step is the residency fallback of a grid that cannot be co-resident, or the flag)."""
    return _hidden_paths("lstm", clear)


def lstm_hidden_supported(B, S, nl, D, H):
    """Does cpc_lstm_layout_h take nn.LSTM(D, H, nl) on (B, S, D)?"""
    return _layout_takes("lstm_layout_h", B, S, nl, D, H)


GRU_HIDDEN_MAX = 512   # widest hidden state of the GRU at any hidden width (cpc_gru_*_h; csrc/gru.hip)


class GruHiddenFunction(torch.autograd.Function):
    """nn.GRU(D, H, nl, batch_first=True) at any hidden width: x (B,S,D), h0 None or (nl,B,H), 4*nl GRU parameters at their true
    shapes -> y (B,S,H), hN (nl,B,H), 1 <= D, H <= 512 (cpc_gru_forward_h / _backward_h: the recurrence runs at the padded width
    128 * ceil(H / 128) on zero-padded weight copies; with H == 256 the entries are cpc_gru_*_in, which take no per_step).  A plain
    Function -- one stream, no prepared coefficients: the carried state gets no gradient, hN is not differentiable, per_step
    selects the one-launch-per-step kernels (same bits)."""

    @staticmethod
    def forward(ctx, x, h0, per_step, *params):
        return _hidden_forward(ctx, "gru", 3, x, (h0,), per_step, params)

    @staticmethod
    def backward(ctx, dy, _dhN):
        return _hidden_backward(ctx, "gru", dy)


def gru_hidden_paths(clear=True):
    """Which recurrence kernels GruHiddenFunction has launched since the last clearing call: a set out of "persistent" and
    "per_step" (cpc_gru_paths_h; per_step is the residency fallback of a grid that cannot be co-resident, or the flag)."""
    return _hidden_paths("gru", clear)


def gru_hidden_supported(B, S, nl, D, H):
    """Does cpc_gru_layout_h take nn.GRU(D, H, nl) on (B, S, D)?"""
    return _layout_takes("gru_layout_h", B, S, nl, D, H)


def lstm_supported(B, S, nl=1):
    """Does cpc_lstm_layout take nl layers on (B, S, 256)?"""
    return _layout_takes("lstm_layout", B, S, nl)


class LstmGroupFunction(torch.autograd.Function):
    """x (B,S,256) read by every head; the heads' nn.LSTM parameters one behind the other: w_ih (G*1024,256), w_hh (G,1024,256),
    b_ih, b_hh (G*1024) -> y (B,S,G*256), head g at columns g*256.. (cpc_lstm_group_forward / _backward): one layer, no carried
    state.  per_step: the one-launch-per-step kernels instead of the persistent recurrence (same bits; tests)."""

    @staticmethod
    def forward(ctx, x, per_step, w_ih, w_hh, b_ih, b_hh):
        _require_cuda(x, "LstmGroupFunction")
        lib = _lib.get()
        if (x.dim() != 3 or x.shape[2] != _HID or w_hh.dim() != 3 or tuple(w_hh.shape[1:]) != (4 * _HID, _HID)
                or tuple(w_ih.shape) != (w_hh.shape[0] * 4 * _HID, _HID) or b_ih.numel() != w_ih.shape[0]
                or b_hh.numel() != w_ih.shape[0]):
            raise NotImplementedError("cpc_audio_amd.LstmGroupFunction: x (B,S,256) and G stacked nn.LSTM(256, 256) parameters expected")
        B, S, _ = x.shape
        G = w_hh.shape[0]
        x = x.contiguous()
        w_ih, w_hh, b_ih, b_hh = (p.detach().contiguous() for p in (w_ih, w_hh, b_ih, b_hh))
        flags = 1 if per_step else 0                      # CPC_LSTM_PER_STEP
        with torch.cuda.device(x.device):
            sizes = _layout("lstm_group_layout", lib.cpc_lstm_group_layout, 3, B, S, G)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
            y = torch.empty(B, S, G * _HID, device=x.device, dtype=torch.float32)
            lib.check(lib.cpc_lstm_group_forward(_p(x), _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), _p(saved), _p(scratch), _p(y),
                                                 B, S, G, flags, _stream()), "lstm_group_forward")
        ctx.save_for_backward(x, saved, y, w_ih, w_hh, b_ih)
        ctx.dims = (B, S, G, sizes[2], flags)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 6
        lib = _lib.get()
        x, saved, y, w_ih, w_hh, b_ih = ctx.saved_tensors
        B, S, G, nscr, flags = ctx.dims
        with torch.cuda.device(x.device):
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            dw_ih, dw_hh, db_ih, db_hh = (torch.empty_like(t) for t in (w_ih, w_hh, b_ih, b_ih))
            lib.check(lib.cpc_lstm_group_backward(_p(x), _p(w_ih), _p(w_hh), _p(saved), _p(y), _p(dy.contiguous()), _p(scratch),
                                                  _p(dx), _p(dw_ih), _p(dw_hh), _p(db_ih), _p(db_hh), B, S, G, flags, _stream()),
                      "lstm_group_backward")
        return dx, None, dw_ih, dw_hh, db_ih, db_hh


def lstm_group_supported(B, S, G):
    """Does cpc_lstm_group_layout take G heads on (B, S, 256)?"""
    return _layout_takes("lstm_group_layout", B, S, G)


class RnnFunction(torch.autograd.Function):
    """Elman recurrences, nn.RNN(256, 256) with tanh (cpc_rnn_forward / _backward).  ``time_major``: x (T,R,256) -> y (T,R,G*256),
    head g at columns g*256.. -- the criterion's RNN predictors, which walk the batch axis of the context; otherwise x (R,T,256)
    -> y (R,T,G*256) -- the batch_first autoregressor (G = 1).  params: per layer weight_ih (G*256,256), weight_hh (G,256,256) or
    (256,256), bias_ih, bias_hh (G*256): the heads' tensors one behind the other; G > 1 only with one layer and without h0.
    h0: None or (nl,R,256); it receives no gradient (the reference detaches the carried state, cpc/model.py:194-198).
    -> y, hN (nl,R,256; not differentiable; None for G > 1).  per_step: one launch per step (same bits; tests).
    One head (G = 1) also takes x of width D with weight_ih_l0 (256, D), 1 <= D <= 512, in either layout (cpc_rnn_forward_in /
    _backward_in)."""

    @staticmethod
    def forward(ctx, x, h0, time_major, per_step, *params):
        _require_cuda(x, "RnnFunction")
        lib = _lib.get()
        nl = len(params) // 4
        # another input width D in 1..512 (weight_ih_l0 (256, D)): one head -- cpc_rnn_*_in
        D = x.shape[2] if x.dim() == 3 else _HID
        narrow = D != _HID
        if narrow and (nl < 1 or len(params) != 4 * nl or not 1 <= D <= IN_PROJ_MAX
                       or tuple(params[0].shape) != (_HID, D)):
            raise NotImplementedError("cpc_audio_amd.RnnFunction: an input width other than 256 takes one head with "
                                      f"weight_ih_l0 (256, D), 1 <= D <= {IN_PROJ_MAX}")
        if (x.dim() != 3 or nl < 1 or len(params) != 4 * nl or params[0].shape[0] % _HID
                or any(params[4 * l].shape[0] != params[0].shape[0] or (params[4 * l].shape[1] != _HID and (l > 0 or not narrow))
                       or params[4 * l + 1].numel() != params[0].shape[0] * _HID or params[4 * l + 2].numel() != params[0].shape[0]
                       or params[4 * l + 3].numel() != params[0].shape[0] for l in range(nl))):
            raise NotImplementedError("cpc_audio_amd.RnnFunction: x (.,.,256) and stacked nn.RNN(256, 256) parameters expected")
        G = params[0].shape[0] // _HID
        T, R = (x.shape[0], x.shape[1]) if time_major else (x.shape[1], x.shape[0])
        x = x.contiguous()
        params = [p.detach().contiguous() for p in params]
        h0 = None if h0 is None else h0.detach().contiguous()
        flags = (1 if per_step else 0) | (2 if time_major else 0)       # CPC_RNN_PER_STEP, CPC_RNN_TIME_MAJOR
        with torch.cuda.device(x.device):
            sizes = _layout("rnn_layout_in", lib.cpc_rnn_layout_in, 3, T, R, nl, D) if narrow else \
                _layout("rnn_layout", lib.cpc_rnn_layout, 3, T, R, G, nl)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
            y = torch.empty(x.shape[0], x.shape[1], G * _HID, device=x.device, dtype=torch.float32)
            hN = torch.empty(nl, R, _HID, device=x.device, dtype=torch.float32) if G == 1 else None
            if narrow:
                lib.check(lib.cpc_rnn_forward_in(_p(x), _p(h0), _ptrs(params), _p(saved), _p(scratch), _p(y), _p(hN), T, R, nl, D,
                                                 flags, _stream()), "rnn_forward_in")
            else:
                lib.check(lib.cpc_rnn_forward(_p(x), _p(h0), _ptrs(params), _p(saved), _p(scratch), _p(y), _p(hN), T, R, G, nl, flags,
                                              _stream()), "rnn_forward")
        ctx.save_for_backward(x, saved, y, *params)
        ctx.h0 = h0
        ctx.dims = (T, R, G, nl, sizes[2], flags)
        if hN is not None:
            ctx.mark_non_differentiable(hN)
        ctx.set_materialize_grads(False)
        return y, hN

    @staticmethod
    def backward(ctx, dy, _dhN):
        lib = _lib.get()
        x, saved, y, *params = ctx.saved_tensors
        T, R, G, nl, nscr, flags = ctx.dims
        dy = torch.zeros_like(y) if dy is None else dy.contiguous()
        with torch.cuda.device(x.device):
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            grads = [torch.empty_like(p) for p in params]
            if x.shape[2] != _HID:
                lib.check(lib.cpc_rnn_backward_in(_p(x), _p(ctx.h0), _ptrs(params), _p(saved), _p(y), _p(dy), _p(scratch), _p(dx),
                                                  _ptrs(grads), T, R, nl, x.shape[2], flags, _stream()), "rnn_backward_in")
            else:
                lib.check(lib.cpc_rnn_backward(_p(x), _p(ctx.h0), _ptrs(params), _p(saved), _p(y), _p(dy), _p(scratch), _p(dx),
                                               _ptrs(grads), T, R, G, nl, flags, _stream()), "rnn_backward")
        return (dx, None, None, None, *grads)


def rnn_supported(T, R, G=1, nl=1):
    """Does cpc_rnn_layout take T steps of R rows, G heads and nl layers?"""
    return _layout_takes("rnn_layout", T, R, G, nl)


CTC_MAX_SEQ = 512        # cpc_ctc_forward: longest sequence (frames) the one-workgroup recursion holds in LDS


def _labels_on(label, device):
    label = label.to(device, non_blocking=True)
    return (label if label.dtype == torch.int64 else label.to(torch.int64)).contiguous()


def _rows_of(x, what):
    """(R, 256) features with unit column stride: their row stride (cFeature[:, -1, :] is read in place)."""
    if x.dim() != 2 or x.shape[1] != _HID:
        raise NotImplementedError(f"cpc_audio_amd.{what}: the HIP classifier is built for 256 input features")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < _HID):
        x = x.contiguous()
    return x, max(int(x.stride(0)), _HID)


CLASSIFIER_MAX_DIM = 512      # widest feature row of the _d entry points (cpc_probe_*_d, cpc_classifier_*_d, cpc_ctc_forward_d)


def _rows_of_width(x, weight, what):
    """(R, D) features with unit column stride for a (C, D) weight, 1 <= D <= CLASSIFIER_MAX_DIM: (x, row stride, D).  256 goes
    through _rows_of and on to the 256 entry points, any other D to the _d ones."""
    if weight.dim() != 2:
        raise ValueError(f"{what}: a (C, D) weight expected, got {tuple(weight.shape)}")
    D = weight.shape[1]
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"{what}: features of shape {tuple(x.shape)} for a weight of shape {tuple(weight.shape)}")
    _require_cuda(x, what)
    if D == _HID:
        return (*_rows_of(x, what), D)
    if not 1 <= D <= CLASSIFIER_MAX_DIM:
        raise NotImplementedError(f"cpc_audio_amd.{what}: the HIP classifier takes 1 to {CLASSIFIER_MAX_DIM} input features, got {D}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < D):
        x = x.contiguous()
    return x, max(int(x.stride(0)), D), D


def _supervised_layout(lib, B, S, C, D, ctc):
    if D == _HID:
        return _layout("supervised_layout", lib.cpc_supervised_layout, 3, B, S, C, ctc)
    return _layout("supervised_layout_d", lib.cpc_supervised_layout_d, 3, B, S, C, D, ctc)


def _classifier_backward(x, ldx, weight, label, saved, dloss, dlogits, R, C, need_dx):
    lib = _lib.get()
    D = weight.shape[1]
    sizes = _supervised_layout(lib, R, 1, C, D, 0)
    scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
    dW, db = torch.empty_like(weight), torch.empty(C, device=x.device, dtype=torch.float32)
    dx = torch.empty(R, D, device=x.device, dtype=torch.float32) if need_dx else None
    args = (x.data_ptr(), ldx, _p(weight), _p(label), _p(saved), _p(dloss), _p(dlogits), _p(scratch), _p(dW), _p(db), _p(dx), R, C)
    if D == _HID:
        lib.check(lib.cpc_classifier_backward(*args, _stream()), "classifier_backward")
    else:
        lib.check(lib.cpc_classifier_backward_d(*args, D, _stream()), "classifier_backward_d")
    return dx, dW, db


class ClassifierXentFunction(torch.autograd.Function):
    """x (R,D) (any row stride), label (R,) int64, weight (C,D), bias (C,) -> loss (1,1) float32, acc (1,1) float64:
    nn.Linear + nn.CrossEntropyLoss() and (argmax == label).double().mean() (cpc/criterion/criterion.py:198-203, 226-231).
    D = 256 runs cpc_classifier_forward / _backward, any other D from 1 to 512 their _d twins.
    acc is not differentiable; x receives a gradient only when it requires one."""

    @staticmethod
    def forward(ctx, x, label, weight, bias):
        x, ldx, D = _rows_of_width(x, weight, "ClassifierXentFunction")     # (a CPU tensor raises there)
        lib = _lib.get()
        R, C = x.shape[0], weight.shape[0]
        label = _labels_on(label, x.device).view(-1)
        if label.numel() != R:
            raise ValueError(f"ClassifierXentFunction: {label.numel()} labels for {R} feature rows")
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        with torch.cuda.device(x.device):
            sizes = _supervised_layout(lib, R, 1, C, D, 0)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            loss = torch.empty(1, 1, device=x.device, dtype=torch.float32)
            acc = torch.empty(1, 1, device=x.device, dtype=torch.float64)
            args = (x.data_ptr(), ldx, _p(weight), _p(bias), _p(label), _p(saved), _p(loss), _p(acc), R, C)
            if D == _HID:
                lib.check(lib.cpc_classifier_forward(*args, _stream()), "classifier_forward")
            else:
                lib.check(lib.cpc_classifier_forward_d(*args, D, _stream()), "classifier_forward_d")
        ctx.save_for_backward(x, label, weight, saved)
        ctx.dims = (ldx, R, C)
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, dloss, _dacc):
        x, label, weight, saved = ctx.saved_tensors
        ldx, R, C = ctx.dims
        if dloss is None:
            return None, None, None, None
        with torch.cuda.device(x.device):
            dx, dW, db = _classifier_backward(x, ldx, weight, label, saved, dloss.contiguous(), None, R, C,
                                              ctx.needs_input_grad[0])
        return dx, None, dW, db


class CtcXentFunction(torch.autograd.Function):
    """x (B,S,D), label (B,S) int64 frame labels, weight (C,D), bias (C,) -> loss (1,1) float32: nn.Linear, log_softmax
    and nn.CTCLoss(blank=C-1, zero_infinity=True) on the collapsed labels with every input length S
    (cpc/criterion/criterion.py:265-283), 1 <= S <= CTC_MAX_SEQ.  D = 256 runs cpc_ctc_forward, any other D from 1 to 512
    cpc_ctc_forward_d."""

    @staticmethod
    def forward(ctx, x, label, weight, bias):
        if weight.dim() != 2 or x.dim() != 3 or x.shape[2] != weight.shape[1]:
            raise ValueError(f"CtcXentFunction: features of shape {tuple(x.shape)} for a weight of shape {tuple(weight.shape)}")
        _require_cuda(x, "CtcXentFunction")
        lib = _lib.get()
        B, S, D = x.shape
        if not 1 <= D <= CLASSIFIER_MAX_DIM:
            raise NotImplementedError(f"cpc_audio_amd.CtcXentFunction: the HIP classifier takes 1 to {CLASSIFIER_MAX_DIM} input "
                                      f"features, got {D}")
        C = weight.shape[0]
        if S > CTC_MAX_SEQ:
            raise ValueError(f"CtcXentFunction: sequences of at most {CTC_MAX_SEQ} frames are supported (got {S})")
        label = _labels_on(label, x.device)
        if tuple(label.shape) != (B, S):
            raise ValueError(f"CtcXentFunction: labels of shape {tuple(label.shape)} for features of shape {tuple(x.shape)}")
        x = x.contiguous()
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        with torch.cuda.device(x.device):
            sizes = _supervised_layout(lib, B, S, C, D, 1)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            loss = torch.empty(1, 1, device=x.device, dtype=torch.float32)
            args = (_p(x), _p(weight), _p(bias), _p(label), _p(saved), _p(loss), B, S, C)
            if D == _HID:
                lib.check(lib.cpc_ctc_forward(*args, _stream()), "ctc_forward")
            else:
                lib.check(lib.cpc_ctc_forward_d(*args, D, _stream()), "ctc_forward_d")
        ctx.save_for_backward(x, weight, saved)
        ctx.dims = (B, S, C, sizes[2])
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, weight, saved = ctx.saved_tensors
        B, S, C, ndl = ctx.dims
        if dloss is None:
            return None, None, None, None
        lib = _lib.get()
        with torch.cuda.device(x.device):
            dlogits = torch.empty(ndl, device=x.device, dtype=torch.float32)
            lib.check(lib.cpc_ctc_backward(_p(saved), _p(dloss.contiguous()), _p(dlogits), B, S, C, _stream()), "ctc_backward")
            D = weight.shape[1]
            dx, dW, db = _classifier_backward(x, D, weight, None, None, None, dlogits, B * S, C, ctx.needs_input_grad[0])
        return (None if dx is None else dx.view(B, S, D)), None, dW, db


# ---- the PER phone classifier (csrc/phone_head.hip) ----------------------------------------------------------------------
PHONE_HEAD_KERNEL, PHONE_HEAD_STRIDE = 8, 4
_CTC_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


PHONE_HEAD_MAX_DIM = 512      # widest feature row of cpc_phone_head_*_d, cpc_seqnorm_*_d and cpc_posterior_forward_d


def _width_checked(D, what):
    if not 1 <= int(D) <= PHONE_HEAD_MAX_DIM:
        raise NotImplementedError(f"cpc_audio_amd.{what}: the HIP kernels take 1 to {PHONE_HEAD_MAX_DIM} input features, got {D}")
    return int(D)


def phone_head_layout(B, S, C, Lmax=0, D=_HID):
    """(T, wr floats, scratch floats, logits floats, CTC saved floats) of cpc_phone_head_layout (D = 256) or
    cpc_phone_head_layout_d (any other D in 1..512; NotImplementedError beyond); ValueError for a shape the kernels do not take."""
    if D == _HID:
        return _layout("phone_head_layout", _lib.get().cpc_phone_head_layout, 5, int(B), int(S), int(C), int(Lmax))
    D = _width_checked(D, "phone_head_layout")
    return _layout("phone_head_layout_d", _lib.get().cpc_phone_head_layout_d, 5, int(B), int(S), int(C), int(Lmax), D)


def phone_head_supported(B, S, C, Lmax=0, D=_HID):
    try:
        phone_head_layout(B, S, C, Lmax, D)
    except (ValueError, NotImplementedError):
        return False
    return True


def _phone_head_inputs(x, weight, what):
    """The contiguous features; their width D is the weight's (ValueError otherwise) and lies in 1..512."""
    if x.dim() != 3 or weight.dim() != 3 or weight.shape[2] != PHONE_HEAD_KERNEL:
        raise NotImplementedError(f"cpc_audio_amd.{what}: the HIP phone head is built for (B, S, D) features and a "
                                  "(C, D, 8) weight")
    if x.shape[2] != weight.shape[1]:
        raise ValueError(f"{what}: features of shape {tuple(x.shape)} for a weight of shape {tuple(weight.shape)}")
    _width_checked(x.shape[2], what)
    _require_cuda(x, what)
    return x.contiguous()


def _phone_head_forward(x, weight, bias, sizes):
    lib = _lib.get()
    B, S, D = x.shape
    C = weight.shape[0]
    wr = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
    scratch = torch.empty(sizes[2], device=x.device, dtype=torch.float32)
    logits = torch.empty(B, sizes[0], C, device=x.device, dtype=torch.float32)
    args = (_p(x), _p(weight), _p(bias), _p(wr), _p(scratch), _p(logits), B, S, C)
    if D == _HID:
        lib.check(lib.cpc_phone_head_forward(*args, _stream()), "phone_head_forward")
    else:
        lib.check(lib.cpc_phone_head_forward_d(*args, D, _stream()), "phone_head_forward_d")
    return logits, wr


def phone_head_logits(x, weight, bias):
    """x (B, S, D) channels-last, weight (C, D, 8), bias (C), 1 <= D <= 512 -> logits (B, (S - 8) // 4 + 1, C): nn.Conv1d(D, C,
    8, stride 4) of the permuted features, permuted back.  256 features go to the 256 entry points, any other width to the _d
    ones.  Not differentiable (evaluation: val_step, perStep)."""
    x = _phone_head_inputs(x.detach(), weight, "phone_head_logits")
    weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
    with torch.cuda.device(x.device):
        sizes = phone_head_layout(x.shape[0], x.shape[1], weight.shape[0], 0, x.shape[2])
        return _phone_head_forward(x, weight, bias, sizes)[0]


class PhoneHeadCtcFunction(torch.autograd.Function):
    """x (B, S, D), weight (C, D, 8), bias (C), in_len (B) int64 windows per utterance, targets (B, Lmax) int64 padded,
    tgt_len (B) int64, blank, reduction -> loss (1,) float32 ((B,) for 'none'): nn.Conv1d(D, C, 8, stride 4), log_softmax
    and nn.CTCLoss(blank, reduction, zero_infinity=True), 1 <= D <= 512 (256: the 256 entry points, otherwise the _d ones).
    Lengths and targets stay on the device.  x receives a gradient only when it requires one."""

    @staticmethod
    def forward(ctx, x, weight, bias, in_len, targets, tgt_len, blank, reduction):
        x = _phone_head_inputs(x, weight, "PhoneHeadCtcFunction")
        lib = _lib.get()
        B, S, D = x.shape
        C = weight.shape[0]
        red = _CTC_REDUCTIONS[reduction]
        targets = targets.to(x.device, non_blocking=True)
        if targets.dtype != torch.int64:
            targets = targets.to(torch.int64)
        if targets.dim() != 2 or targets.shape[0] != B:
            raise ValueError(f"PhoneHeadCtcFunction: targets of shape {tuple(targets.shape)} for {B} utterances")
        Lmax = targets.shape[1]
        if Lmax and targets.stride(1) != 1:
            targets = targets.contiguous()
        in_len, tgt_len = _labels_on(in_len, x.device).view(-1), _labels_on(tgt_len, x.device).view(-1)
        if in_len.numel() != B or tgt_len.numel() != B:
            raise ValueError(f"PhoneHeadCtcFunction: {in_len.numel()} input and {tgt_len.numel()} target lengths for {B} utterances")
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        with torch.cuda.device(x.device):
            sizes = phone_head_layout(B, S, C, Lmax, D)
            T = sizes[0]
            logits, wr = _phone_head_forward(x, weight, bias, sizes)
            saved = torch.empty(sizes[4], device=x.device, dtype=torch.float32)
            loss = torch.empty(B if red == 0 else 1, device=x.device, dtype=torch.float32)
            lib.check(lib.cpc_ctc_seq_forward(_p(logits), _p(in_len), targets.data_ptr() if Lmax else None,
                                              targets.stride(0) if Lmax else 0, _p(tgt_len), _p(saved), _p(loss), B, T, C, Lmax,
                                              int(blank), red, _stream()), "ctc_seq_forward")
        ctx.save_for_backward(x, wr, logits, saved)
        ctx.dims = (B, S, T, C, Lmax, int(blank), red, sizes[2])
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, wr, logits, saved = ctx.saved_tensors
        B, S, T, C, Lmax, blank, red, nscr = ctx.dims
        if dloss is None:
            return (None,) * 8
        lib = _lib.get()
        with torch.cuda.device(x.device):
            dlogits = torch.empty_like(logits)
            lib.check(lib.cpc_ctc_seq_backward(_p(logits), _p(saved), _p(dloss.contiguous()), _p(dlogits), B, T, C, Lmax, blank,
                                               red, _stream()), "ctc_seq_backward")
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            D = x.shape[2]
            dW = torch.empty(C, D, PHONE_HEAD_KERNEL, device=x.device, dtype=torch.float32)
            db = torch.empty(C, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            args = (_p(x), _p(wr), _p(dlogits), _p(scratch), _p(dW), _p(db), _p(dx), B, S, C)
            if D == _HID:
                lib.check(lib.cpc_phone_head_backward(*args, _stream()), "phone_head_backward")
            else:
                lib.check(lib.cpc_phone_head_backward_d(*args, D, _stream()), "phone_head_backward_d")
        return dx, dW, db, None, None, None, None, None


# ---- the feed-forward prediction networks: ffd, conv4 / conv8 / conv12 (csrc/pred_conv.hip) ------------------------------
def pred_conv_layout(B, W, G, ks):
    """(wr floats, backward scratch floats, y floats) of cpc_pred_conv_layout; ValueError for a shape the kernels do not take."""
    return _layout("pred_conv_layout", _lib.get().cpc_pred_conv_layout, 3, int(B), int(W), int(G), int(ks))


def pred_conv_supported(B, W, G, ks):
    """The shapes cpc_pred_conv_forward / _backward take: 1 <= G <= 64 heads, 1 <= ks <= 16 taps, B, W >= 1 and
    B W G 256 < 2^31."""
    return _layout_takes("pred_conv_layout", B, W, G, ks)


class PredConvFunction(torch.autograd.Function):
    """x (B, W, 256) read by every head, or (B, W, G*256) with head g at columns g*256.. (``shared`` False); weight
    (G, 256, 256, ks): the heads' Conv1d weights stacked (an nn.Linear weight is ks = 1); bias (G, 256); scale: the equalized
    layer's constant; relu -> (B, W, G*256), head g at columns g*256..:
    act(scale * (bias_g + causal conv of x_g with weight_g over the time axis)), frames in front of a window read as zero
    (cpc_pred_conv_forward / _backward).  Saves x, and y when relu is set."""

    @staticmethod
    def forward(ctx, x, weight, bias, scale, relu, shared):
        _require_cuda(x, "PredConvFunction")
        lib = _lib.get()
        if weight.dim() != 4 or tuple(weight.shape[1:3]) != (_HID, _HID) or tuple(bias.shape) != (weight.shape[0], _HID):
            raise NotImplementedError("cpc_audio_amd.PredConvFunction: a (G, 256, 256, ks) weight and a (G, 256) bias expected")
        G, ks = weight.shape[0], weight.shape[3]
        if x.dim() != 3 or x.shape[2] != (_HID if shared else G * _HID):
            raise NotImplementedError(f"cpc_audio_amd.PredConvFunction: x of shape {tuple(x.shape)} for {G} heads "
                                      f"({'shared' if shared else 'per-head'} input)")
        B, W, _ = x.shape
        x = x.contiguous()
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        with torch.cuda.device(x.device):
            sizes = pred_conv_layout(B, W, G, ks)
            wr = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            y = torch.empty(B, W, G * _HID, device=x.device, dtype=torch.float32)
            lib.check(lib.cpc_pred_conv_forward(_p(x), _p(weight), _p(bias), _p(wr), _p(y), B, W, G, ks, int(bool(shared)),
                                                float(scale), int(bool(relu)), _stream()), "pred_conv_forward")
        ctx.save_for_backward(x, weight, *((y,) if relu else ()))
        ctx.dims = (B, W, G, ks, bool(shared), float(scale), bool(relu), sizes[1])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors[:2]
        B, W, G, ks, shared, scale, relu, nscr = ctx.dims
        if dy is None:
            return (None,) * 6
        y = ctx.saved_tensors[2] if relu else None
        lib = _lib.get()
        with torch.cuda.device(x.device):
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            dw = torch.empty_like(weight)
            db = torch.empty(G, _HID, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            lib.check(lib.cpc_pred_conv_backward(_p(x), _p(weight), _p(y), _p(dy.contiguous()), _p(scratch), _p(dw), _p(db),
                                                 _p(dx), B, W, G, ks, int(shared), scale, int(relu), _stream()),
                      "pred_conv_backward")
        return dx, dw, db, None, None, None


# ---- the PER phone classifier's front: seqNorm and dropout (csrc/seqnorm.hip) ------------------------------------------
def seqnorm_supported(B, S, D=_HID):
    """The shapes cpc_seqnorm_forward (D = 256) and cpc_seqnorm_forward_d take: B >= 1, S >= 1, 1 <= D <= 512, B * S * D < 2^31."""
    return B >= 1 and S >= 1 and 1 <= D <= PHONE_HEAD_MAX_DIM and B * S * D < (1 << 31)


class SeqNormFunction(torch.autograd.Function):
    """x (B, S, D), 1 <= D <= 512 (256: the 256 entry points, otherwise the _d ones), lengths (B) int64 valid frames per
    utterance or None (all S), scale (B, D) or None, normalise -> y (B, S, D): per utterance and channel, (x - mean) / sqrt(var + 1e-8) with the mean and the unbiased variance of the
    valid frames, applied to every frame, times scale (CTCphone_criterion's seqNorm with Dropout2d's per-channel factor);
    normalise False: x * scale.  The lengths stay on the device.  Neither lengths nor scale receives a gradient; when x does
    not require one, no statistics are kept and backward launches nothing.  x is never written."""

    @staticmethod
    def forward(ctx, x, lengths, scale, normalise):
        if x.dim() != 3:
            raise NotImplementedError("cpc_audio_amd.SeqNormFunction: built for (B, S, D) features")
        if scale is not None and (scale.dim() != 2 or scale.shape[1] != x.shape[2]):
            raise ValueError(f"SeqNormFunction: scale of shape {tuple(scale.shape)} for features of shape {tuple(x.shape)}")
        _width_checked(x.shape[2], "SeqNormFunction")
        _require_cuda(x, "SeqNormFunction")
        lib = _lib.get()
        B, S, D = x.shape
        x = x.contiguous()
        normalise = bool(normalise)
        if lengths is not None:
            lengths = _labels_on(lengths, x.device).view(-1)
            if lengths.numel() != B:
                raise ValueError(f"SeqNormFunction: {lengths.numel()} lengths for {B} utterances")
        if scale is not None:
            _require_cuda(scale, "SeqNormFunction")
            if tuple(scale.shape) != (B, D):
                raise ValueError(f"SeqNormFunction: scale of shape {tuple(scale.shape)} for {B} utterances")
            scale = scale.detach().contiguous()
        need_dx = ctx.needs_input_grad[0]
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            stats = torch.empty(B, 2, D, device=x.device, dtype=torch.float32) if need_dx and normalise else None
            args = (_p(x), _p(lengths), _p(scale), _p(y), _p(stats), B, S)
            if D == _HID:
                lib.check(lib.cpc_seqnorm_forward(*args, int(normalise), _stream()), "seqnorm_forward")
            else:
                lib.check(lib.cpc_seqnorm_forward_d(*args, D, int(normalise), _stream()), "seqnorm_forward_d")
        if need_dx:
            ctx.save_for_backward(*(t for t in (x if normalise else None, lengths, scale, stats) if t is not None))
            ctx.have = (normalise, lengths is not None, scale is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        normalise, has_len, has_scale = ctx.have
        saved = list(ctx.saved_tensors)
        x = saved.pop(0) if normalise else None
        lengths = saved.pop(0) if has_len else None
        scale = saved.pop(0) if has_scale else None
        stats = saved.pop(0) if normalise else None
        lib = _lib.get()
        dy = dy.contiguous()
        B, S, D = dy.shape
        with torch.cuda.device(dy.device):
            dx = torch.empty_like(dy)
            args = (_p(x), _p(dy), _p(lengths), _p(scale), _p(stats), _p(dx), B, S)
            if D == _HID:
                lib.check(lib.cpc_seqnorm_backward(*args, int(normalise), _stream()), "seqnorm_backward")
            else:
                lib.check(lib.cpc_seqnorm_backward_d(*args, D, int(normalise), _stream()), "seqnorm_backward_d")
        return dx, None, None, None


# ---- the learned-filter-bank encoder (csrc/lfb.hip) -----------------------------------------------------------------------
_LFB_TAPS = 400


def lfb_frames(L):
    """Frames of a window of L samples: the Hann low-pass has 400 taps, stride 160 and padding 350 over the L - 399 conv positions."""
    return (L - 99) // 160 + 1


def lfb_supported(N, L, D):
    """The shapes cpc_lfb_energy_forward / _backward take: N >= 1, L >= 400, D a multiple of 32 up to 512, N F D < 2^31 and
    N (L - 399) < 2^31."""
    return (N >= 1 and L >= _LFB_TAPS and D >= 32 and D % 32 == 0 and D <= 512 and N * lfb_frames(L) * D < (1 << 31)
            and N * (L - 399) < (1 << 31))


class LfbFunction(torch.autograd.Function):
    """x (N, 1, L) or (N, L), weight (2D, 1, 400), bias (2D), han (400 values), normalise, grad_enabled (the caller's
    torch.is_grad_enabled(): inside forward grad mode is always off) -> the (N, D, F) VIEW of a contiguous
    (N, F, D) tensor: LFBEnconder's forward (conv, squared modulus of channel pairs, Hann low-pass at stride 160, log(1 + |.|),
    instance norm over the frames) in two launches, cpc_lfb_energy_forward and cpc_lfb_lognorm_forward.  The conv output is never
    stored: x, the pooled energies s (N, F, D) and the norm's statistics are all that is saved, and nothing is saved when neither
    weight nor bias requires a gradient or grad mode is off.  backward: cpc_lfb_lognorm_backward, then cpc_lfb_energy_backward,
    which recomputes the conv; the waveform and the window receive no gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, han, normalise, grad_enabled):
        _require_cuda(x, "LfbFunction")
        lib = _lib.get()
        N, L = x.shape[0], x.shape[-1]
        D = weight.shape[0] // 2
        if x.numel() != N * L or tuple(weight.shape) != (2 * D, 1, _LFB_TAPS) or han.numel() != _LFB_TAPS:
            raise ValueError(f"LfbFunction: x {tuple(x.shape)}, weight {tuple(weight.shape)}, han {tuple(han.shape)}")
        if not lfb_supported(N, L, D):
            raise NotImplementedError(f"cpc_audio_amd.LfbFunction: unsupported shape N={N} L={L} D={D} (ops.lfb_supported)")
        x = x.detach().contiguous()
        w, b, h = weight.detach().contiguous(), bias.detach().contiguous(), han.detach().contiguous()
        normalise = bool(normalise)
        need = bool(grad_enabled) and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        with torch.cuda.device(x.device):
            F, fwd_bytes, _ = _layout("lfb_layout", lib.cpc_lfb_layout, 3, N, L, D)
            s = torch.empty(N, F, D, device=x.device, dtype=torch.float32)
            y = torch.empty_like(s)
            ws = torch.empty(fwd_bytes // 4, device=x.device, dtype=torch.float32) if fwd_bytes else None
            stats = torch.empty(N, 2, D, device=x.device, dtype=torch.float32) if need and normalise else None
            lib.check(lib.cpc_lfb_energy_forward(_p(x), _p(w), _p(b), _p(h), _p(s), _p(ws), N, L, D, _stream()),
                      "lfb_energy_forward")
            lib.check(lib.cpc_lfb_lognorm_forward(_p(s), _p(y), _p(stats), N, F, D, int(normalise), _stream()),
                      "lfb_lognorm_forward")
        if need:
            ctx.save_for_backward(*(t for t in (x, w, b, h, s, stats) if t is not None))    # w, b, h: the parameters' own storage
            ctx.normalise = normalise
        return y.permute(0, 2, 1)

    @staticmethod
    def backward(ctx, dy):
        if dy is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None, None, None, None
        saved = list(ctx.saved_tensors)
        x, w, b, h, s = saved[:5]
        stats = saved[5] if ctx.normalise else None
        lib = _lib.get()
        N, F, D = s.shape
        L = x.shape[-1]
        dy = dy.permute(0, 2, 1).contiguous()
        with torch.cuda.device(dy.device):
            bwd_bytes = _layout("lfb_layout", lib.cpc_lfb_layout, 3, N, L, D)[2]
            ds = torch.empty_like(s)
            dW = torch.empty(2 * D, 1, _LFB_TAPS, device=dy.device, dtype=torch.float32)
            db = torch.empty(2 * D, device=dy.device, dtype=torch.float32)
            ws = torch.empty(bwd_bytes // 4, device=dy.device, dtype=torch.float32)
            lib.check(lib.cpc_lfb_lognorm_backward(_p(s), _p(stats), _p(dy), _p(ds), N, F, D, int(ctx.normalise), _stream()),
                      "lfb_lognorm_backward")
            lib.check(lib.cpc_lfb_energy_backward(_p(x), _p(w), _p(b), _p(h), _p(ds), _p(dW), _p(db), _p(ws), N, L, D, _stream()),
                      "lfb_energy_backward")
        return None, dW, db, None, None, None


# ---- the MFCC encoder (csrc/mfcc.hip) ----------------------------------------------------------------------------------------
_MFCC_FFT, _MFCC_HOP, _MFCC_BINS = 321, 160, 161


def mfcc_frames(L):
    """Frames of a window of L samples: centred frames of 321 samples at a hop of 160 over the reflect-padded window."""
    return (L - 1) // _MFCC_HOP + 1


def mfcc_mels(D):
    """The reference's n_mels for n_mfcc = D (cpc/model.py:116)."""
    return max(128, D)


def mfcc_supported(N, L, D):
    """The shapes cpc_mfcc_meldb / cpc_mfcc_dct take: N >= 1, L >= 161, 1 <= D <= 512, N F max(128, D) < 2^31."""
    return N >= 1 and L >= _MFCC_BINS and 1 <= D <= 512 and N * mfcc_frames(L) * mfcc_mels(D) < (1 << 31)


def mfcc_window():
    """The periodic Hann window of 321 points in float64."""
    return 0.5 - 0.5 * torch.cos(2 * torch.pi * torch.arange(_MFCC_FFT, dtype=torch.float64) / _MFCC_FFT)


def mfcc_basis(window):
    """The windowed DFT basis (321, 322) the kernel reads, fp32: columns 0..160 w[j] cos(2 pi j k / 321), columns 161..321
    -w[j] sin(2 pi j k / 321); formed in float64 from ``window`` (321 values, any dtype) and rounded once."""
    w = window.detach().reshape(-1).to(device="cpu", dtype=torch.float64)
    jk = torch.arange(_MFCC_FFT, dtype=torch.int64)[:, None] * torch.arange(_MFCC_BINS, dtype=torch.int64)[None, :]
    ang = 2 * torch.pi * (jk % _MFCC_FFT).double() / _MFCC_FFT          # (the angle reduced exactly, in integers)
    return torch.cat([w[:, None] * torch.cos(ang), -w[:, None] * torch.sin(ang)], dim=1).float()


def mfcc_tables64(D):
    """(window (321), fb (161, M), dct (M, D)) in float64 on the CPU, M = max(128, D): the periodic Hann window, the HTK mel
    filter bank over the grid linspace(0, 8000, 161) without area normalisation and the orthonormal DCT-II."""
    M = mfcc_mels(D)
    freqs = torch.linspace(0, 8000, _MFCC_BINS, dtype=torch.float64)
    m_max = 2595.0 * torch.log10(torch.tensor(1.0 + 8000.0 / 700.0, dtype=torch.float64)).item()
    f_pts = 700.0 * (10.0 ** (torch.linspace(0, m_max, M + 2, dtype=torch.float64) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]                              # (161, M + 2)
    fb = torch.clamp(torch.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)
    m = torch.arange(M, dtype=torch.float64)[:, None]
    d = torch.arange(D, dtype=torch.float64)[None, :]
    dct = torch.cos(torch.pi / M * (m + 0.5) * d) * (2.0 / M) ** 0.5
    dct[:, 0] *= 0.5 ** 0.5
    return mfcc_window(), fb, dct


def mfcc_tables(D):
    """The three read-only tables of the MFCC encoder as fp32 CPU tensors, built in float64 and rounded once (include/cpc_hip.h):
    basis (321, 322), fb (161, M) and dct (M, D), M = max(128, D)."""
    window, fb, dct = mfcc_tables64(D)
    return mfcc_basis(window), fb.float(), dct.float()


def mfcc(x, basis, fb, dct, rowwise=False):
    """x (N, 1, L) or (N, L) fp32 on the GPU and the tables of ``mfcc_tables`` on the same device -> the (N, D, F) VIEW of a
    contiguous (N, F, D) tensor: MFCCEncoder's forward in two launches, cpc_mfcc_meldb and cpc_mfcc_dct.  ``rowwise``: the dB floor
    hangs 80 dB below the maximum of each row instead of the whole call.  Nothing is differentiated: the result never requires
    grad, and the unclamped dB tensor and the partial maxima are temporaries of the caching allocator on the current stream."""
    _require_cuda(x, "mfcc")
    lib = _lib.get()
    N, L = x.shape[0], x.shape[-1]
    M, D = dct.shape
    if (x.numel() != N * L or tuple(basis.shape) != (_MFCC_FFT, 2 * _MFCC_BINS) or tuple(fb.shape) != (_MFCC_BINS, M)
            or M != mfcc_mels(D)):
        raise ValueError(f"mfcc: x {tuple(x.shape)}, basis {tuple(basis.shape)}, fb {tuple(fb.shape)}, dct {tuple(dct.shape)}")
    if not mfcc_supported(N, L, D):
        raise NotImplementedError(f"cpc_audio_amd.mfcc: unsupported shape N={N} L={L} D={D} (ops.mfcc_supported)")
    for t in (basis, fb, dct):
        _require_cuda(t, "mfcc")
    x = x.detach().contiguous()
    basis, fb, dct = basis.detach().contiguous(), fb.detach().contiguous(), dct.detach().contiguous()
    with torch.cuda.device(x.device):
        F, M_, ws_bytes = _layout("mfcc_layout", lib.cpc_mfcc_layout, 3, N, L, D)
        db = torch.empty(N, F, M, device=x.device, dtype=torch.float32)
        ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
        y = torch.empty(N, F, D, device=x.device, dtype=torch.float32)
        lib.check(lib.cpc_mfcc_meldb(_p(x), _p(basis), _p(fb), _p(db), _p(ws), N, L, D, _stream()), "mfcc_meldb")
        lib.check(lib.cpc_mfcc_dct(_p(db), _p(ws), _p(dct), _p(y), N, F, D, int(bool(rowwise)), _stream()), "mfcc_dct")
    return y.permute(0, 2, 1)


# ---- the frozen linear-separability step in one C call (csrc/probe.hip) ------------------------------------------------
_probe_workspaces = {}


def _probe_setup(x, label, weight, what):
    x, ldx, D = _rows_of_width(x, weight, what)                              # (a CPU tensor raises there)
    R, C = x.shape[0], weight.shape[0]
    label = _labels_on(label, x.device).view(-1)
    if label.numel() != R:
        raise ValueError(f"{what}: {label.numel()} labels for {R} feature rows")
    lib = _lib.get()
    stream = _stream()
    key = (R, C, D, x.device, stream)
    ws = _probe_workspaces.get(key)
    if ws is None:                                       # once per shape (and stream: calls on one stream are ordered)
        if D == _HID:
            sizes = _layout("probe_layout", lib.cpc_probe_layout, 3, R, C)
        else:
            sizes = _layout("probe_layout_d", lib.cpc_probe_layout_d, 3, R, C, D)
        ws = _probe_workspaces[key] = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
    return lib, x, ldx, label, R, C, D, ws, stream


def _probe_outputs(x, out):
    if out is not None:
        return out
    return (torch.empty(1, 1, device=x.device, dtype=torch.float32), torch.empty(1, 1, device=x.device, dtype=torch.float64))


@torch.no_grad()
def probe_train_step(x, label, weight, bias, optimizer, accum=None, out=None, grads=None):
    """One frozen probe step (cpc_probe_train_step; weight (C,D) with D != 256: cpc_probe_train_step_d): x (R,D) (any row
    stride), label (R,) -> loss (1,1) float32 and acc (1,1)
    float64 of nn.Linear(weight, bias) + mean cross-entropy BEFORE the update, and ``optimizer`` (optim.Adam)'s update of
    weight and bias in place, moments and step count included.  accum: two device doubles that receive += loss, += acc;
    out: (loss, acc) tensors to write instead of new ones; grads: (dW, db) tensors that receive the gradients."""
    lib, x, ldx, label, R, C, D, ws, stream = _probe_setup(x, label, weight, "probe_train_step")
    for p in (weight, bias):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise TypeError("probe_train_step: dense fp32 parameters on the GPU expected")
    group, moments, bc1, bc2s = optimizer.fused_step_state([weight, bias])
    (mW, vW), (mb, vb) = moments
    loss, acc = _probe_outputs(x, out)
    dW, db = grads if grads is not None else (None, None)
    beta1, beta2 = group["betas"]
    with torch.cuda.device(x.device):
        tail = (_p(weight), _p(bias), _p(mW), _p(vW), _p(mb), _p(vb), float(group["lr"]), beta1, beta2, float(group["eps"]), bc1,
                bc2s, _p(ws), _p(loss), _p(acc), _p(accum), _p(dW), _p(db), stream)
        if D == _HID:
            lib.check(lib.cpc_probe_train_step(x.data_ptr(), ldx, _p(label), R, C, *tail), "probe_train_step")
        else:
            lib.check(lib.cpc_probe_train_step_d(x.data_ptr(), ldx, _p(label), R, C, D, *tail), "probe_train_step_d")
    return loss, acc


@torch.no_grad()
def probe_eval(x, label, weight, bias, accum=None, out=None):
    """Loss (1,1) float32 and accuracy (1,1) float64 of the linear classifier on x (R,D), label (R,) (cpc_probe_eval; D != 256:
    cpc_probe_eval_d); accum / out as in probe_train_step."""
    lib, x, ldx, label, R, C, D, ws, stream = _probe_setup(x, label, weight, "probe_eval")
    loss, acc = _probe_outputs(x, out)
    with torch.cuda.device(x.device):
        tail = (_p(weight.detach().contiguous()), _p(bias.detach().contiguous()), _p(ws), _p(loss), _p(acc), _p(accum), stream)
        if D == _HID:
            lib.check(lib.cpc_probe_eval(x.data_ptr(), ldx, _p(label), R, C, *tail), "probe_eval")
        else:
            lib.check(lib.cpc_probe_eval_d(x.data_ptr(), ldx, _p(label), R, C, D, *tail), "probe_eval_d")
    return loss, acc


# ---- phone posteriors for feature export (csrc/posterior.hip) -----------------------------------------------------------
POSTERIOR_MAX_CLASSES = 8192


@torch.no_grad()
def posterior(x, weight, bias, one_hot=False, wide=False):
    """softmax(x weight^T + bias) per row -- float32 (R, C) -- or, with ``one_hot``, the int64 (R, C) one-hot of each row's
    argmax (the first index on ties), in one launch (cpc_posterior_forward).  x: CUDA fp32 (R, 256) with any row stride;
    runs on the current stream.  Evaluation only: not differentiable.
    wide: x (R, D) and weight (C, D) with 1 <= D <= 512 (cpc_posterior_forward_d; 256 still goes to the 256 entry point); a
    width mismatch is a ValueError, a width outside the range NotImplementedError.  Without it any width but 256 is refused."""
    if wide:
        x, ldx, D = _rows_of_width(x, weight, "posterior")                   # (a CPU tensor raises there, behind the widths)
    else:
        _require_cuda(x, "posterior")
        x, ldx = _rows_of(x, "posterior")
        D = _HID
    R, C = x.shape[0], weight.shape[0]
    weight, bias = weight.detach(), bias.detach()
    if tuple(weight.shape) != (C, D) or tuple(bias.shape) != (C,):
        raise ValueError(f"posterior: weight (C, {D}) and bias (C,) expected, got {tuple(weight.shape)} and {tuple(bias.shape)}")
    for t in (weight, bias):
        if t.device != x.device or t.dtype != torch.float32:
            raise TypeError("posterior: fp32 parameters on the features' device expected")
    out = torch.empty(R, C, device=x.device, dtype=torch.int64 if one_hot else torch.float32)
    lib = _lib.get()
    args = (x.data_ptr(), ldx, _p(weight.contiguous()), _p(bias.contiguous()), R, C)
    with torch.cuda.device(x.device):
        if D == _HID:
            lib.check(lib.cpc_posterior_forward(*args, 1 if one_hot else 0, _p(out), None, _stream()), "posterior_forward")
        else:
            lib.check(lib.cpc_posterior_forward_d(*args, D, 1 if one_hot else 0, _p(out), None, _stream()), "posterior_forward_d")
    return out


def candidate_destinations(ext, B, S, K):
    """(perm, row_ptr) for cpc_nce_backward: the B*W*(N+K) candidate slots sorted (stably) by the
    row of z.view(B*S,256) their gradient lands on.  ext: (B,W,N) int32 negative rows; the K
    positives of window (b,t) land on rows b*S + t + k, k = 1..K (criterion.py:210-215)."""
    W = ext.shape[1]
    dev = ext.device
    b = torch.arange(B, device=dev, dtype=torch.int32).view(B, 1, 1)
    t = torch.arange(W, device=dev, dtype=torch.int32).view(1, W, 1)
    k = torch.arange(1, K + 1, device=dev, dtype=torch.int32).view(1, 1, K)
    dest = torch.cat([ext, b * S + t + k], dim=2).reshape(-1)
    sorted_dest, perm = torch.sort(dest, stable=True)
    bounds = torch.arange(B * S + 1, device=dev, dtype=torch.int32)
    row_ptr = torch.searchsorted(sorted_dest, bounds)
    return perm.to(torch.int32), row_ptr.to(torch.int32)


class head_group:
    """``with head_group(lib, (k0, k_total)):`` -- the cpc_nce_* calls inside work on heads k0 .. of a criterion with k_total
    prediction steps (cpc_nce_head_group: the score tiles hold 16 heads, more are walked in groups).  The setting belongs to the
    calling thread, so every function that makes such calls -- autograd runs backward on a thread of its own -- brackets its own."""

    def __init__(self, lib, group):
        self.lib, self.group = lib, group

    def __enter__(self):
        if self.group is not None:
            self.lib.check(self.lib.cpc_nce_head_group(int(self.group[0]), int(self.group[1])), "nce_head_group")

    def __exit__(self, *exc):
        if self.group is not None:
            self.lib.cpc_nce_head_group(0, 0)
        return False


def prepare_negatives(batchIdx, seqIdx, B, S, K, N, group=None):
    """(ext (B,W,Np), perm, row_ptr) int32 from the two int64 draws of sampleClean -- cpc_nce_prepare.  Np = N rounded up to the
    kernels' 16-wide candidate tile (cpc_nce_padded_negatives): the padding entries are masked by position in the scoring
    kernels, so every call that takes these lists is also told N.  ``group`` = (k0, k_total): the lists of heads k0 .. k0+K-1 of
    a criterion with k_total > 16 prediction steps (head_group)."""
    lib = _lib.get()
    W = S - (K if group is None else group[1])
    Np = int(lib.cpc_nce_padded_negatives(N))
    dev = batchIdx.device
    batchIdx, seqIdx = batchIdx.contiguous(), seqIdx.contiguous()
    if batchIdx.dtype != torch.int64 or seqIdx.dtype != torch.int64 or batchIdx.numel() != B * N * W:
        raise ValueError("prepare_negatives: expected two int64 tensors of B*N*W draws")
    with torch.cuda.device(dev):
        ext = torch.empty(B, W, Np, device=dev, dtype=torch.int32)
        perm = torch.empty(B * W * (Np + K), device=dev, dtype=torch.int32)
        row_ptr = torch.empty(B * S + 1, device=dev, dtype=torch.int32)
        work = torch.empty(B * W * (Np + K) + 2 * B * S + 2, device=dev, dtype=torch.int32)
        with head_group(lib, group):
            lib.check(lib.cpc_nce_prepare(_p(batchIdx), _p(seqIdx), _p(ext), _p(perm), _p(row_ptr), _p(work), B, S, K, N,
                                          _stream()), "nce_prepare")
    return ext, perm, row_ptr


class InfoNCEFunction(torch.autograd.Function):
    """c, z (B,S,256), wall (K*256,256), ext (B,W,N) int32, perm, row_ptr -> losses (K), acc (K).
    ``heads``: optionally the K leaf parameters (256,256) that ``wall`` is the row-wise concatenation of.  With
    an overlapping StepContext their gradient is then formed on the side stream as well and accumulated into ``.grad`` directly
    (bit-identical values; ``wall`` itself receives no gradient), which takes that GEMM off the path to the encoder."""

    @staticmethod
    def forward(ctx, c, z, wall, ext, perm, row_ptr, heads=None, defer_dz=False, saved=None, n_valid=None, group=None):
        """saved: optionally the workspace of this call with the GEMM operand bounds already in it (nce_bounds_into).
        n_valid: negatives per window as drawn when ext's rows are padded to the 16-wide tile (prepare_negatives).
        group: (k0, k_total) when ``wall`` holds heads k0 .. of a criterion with k_total > 16 prediction steps (head_group)."""
        _require_cuda(c, "InfoNCEFunction")
        lib = _lib.get()
        B, S, H = c.shape
        K = wall.shape[0] // _HID
        W, N = ext.shape[1], ext.shape[2]
        if n_valid is not None:
            if int(lib.cpc_nce_padded_negatives(int(n_valid))) != N:
                raise ValueError("InfoNCEFunction: ext is not padded for n_valid negatives")
            N = int(n_valid)
        if H != _HID or z.shape != (B, S, _HID) or W != S - (K if group is None else group[1]) or ext.dtype != torch.int32:
            raise ValueError("InfoNCEFunction: inconsistent shapes")
        c, z, wall, ext = c.contiguous(), z.contiguous(), wall.detach().contiguous(), ext.contiguous()
        with torch.cuda.device(c.device), head_group(lib, group):
            sizes = _layout(f"nce_layout{group or ''}", lib.cpc_nce_layout, 6, B, S, K, N)
            fwd = lib.cpc_nce_forward_prepared
            if saved is None or saved.numel() != sizes[0] or saved.device != c.device:
                saved = torch.empty(sizes[0], device=c.device, dtype=torch.float32)
                fwd = lib.cpc_nce_forward
            scratch = torch.empty(sizes[1], device=c.device, dtype=torch.float32)
            losses = torch.empty(K, device=c.device, dtype=torch.float32)
            acc = torch.empty(K, device=c.device, dtype=torch.float32)
            lib.check(fwd(_p(c), _p(z), _p(wall), _p(ext), _p(saved), _p(scratch), _p(losses), _p(acc), B, S, K, N,
                          _stream()), "nce_forward")
        ctx.save_for_backward(c, z, wall, ext, saved, perm, row_ptr)
        ctx.dims = (B, S, K, N, sizes[2])
        ctx.group = group
        ctx.set_materialize_grads(False)       # no zero-filled gradient for the accuracies
        ctx.heads = list(heads) if heads is not None else None
        ctx.step = current()
        ctx.defer_dz = bool(defer_dz)          # the caller's proof that nobody reads dz early (dz_may_be_deferred)
        if ctx.heads is not None and (len(ctx.heads) != K or any(h.shape != (_HID, _HID) for h in ctx.heads)):
            raise ValueError("InfoNCEFunction: heads must be the K (256,256) weights stacked in wall")
        ctx.mark_non_differentiable(acc)
        return losses, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        lib = _lib.get()
        c, z, wall, ext, saved, perm, row_ptr = ctx.saved_tensors
        B, S, K, N, nscr = ctx.dims
        gloss = torch.zeros(K, device=c.device) if gloss is None else gloss.contiguous()
        with torch.cuda.device(c.device):
            scratch = torch.empty(nscr, device=c.device, dtype=torch.float32)
            dc, dz, dwall = torch.empty_like(c), torch.empty_like(z), torch.empty_like(wall)
            step = ctx.step
            if _overlap(step) and ctx.group is None:
                main, side = torch.cuda.current_stream(), step.side_stream(c.device)
                ready = torch.cuda.Event()
                heads = ctx.heads if ctx.heads is not None and any(h.requires_grad for h in ctx.heads) else None
                # dc (and dwall, unless the leaf weights are known) now, on this stream; dz = NULL leaves the dz path out
                lib.check(lib.cpc_nce_backward_streams(_p(c), _p(z), _p(wall), _p(ext), _p(perm), _p(row_ptr), _p(saved),
                                                       _p(gloss), _p(scratch), _p(dc), None,
                                                       None if heads else _p(dwall), B, S, K, N,
                                                       main.cuda_stream, main.cuda_stream), "nce_backward")
                ready.record(main)

                def dz_path():            # ... dz later, on the side stream, once the AR backward has been launched
                    side.wait_event(ready)
                    lib.check(lib.cpc_nce_backward_dz(_p(c), _p(wall), _p(perm), _p(row_ptr), _p(saved), _p(scratch), _p(dz),
                                                      B, S, K, N, side.cuda_stream), "nce_backward_dz")
                    for t in (dz, scratch, c, wall, perm, row_ptr, saved):
                        t.record_stream(side)                     # the allocator must not recycle them early
                    ev = torch.cuda.Event()
                    ev.record(side)
                    step.side_events.append(ev)
                if ctx.defer_dz:
                    step.deferred.append(dz_path)
                else:
                    # somebody this package does not know may read dz as soon as this backward returns (criterion mode
                    # 'reverse': a torch.flip; a foreign autoregressor): it is formed now, on this stream
                    lib.check(lib.cpc_nce_backward_dz(_p(c), _p(wall), _p(perm), _p(row_ptr), _p(saved), _p(scratch), _p(dz),
                                                      B, S, K, N, main.cuda_stream), "nce_backward_dz")
                    ready.record(main)         # the head gradient on the side stream reads the same scratch
                if heads:
                    dheads = dwall
                    def dwall_path():     # ... and the head-weight gradient after it: only the optimiser reads it
                        side.wait_event(ready)
                        with torch.cuda.stream(side):
                            lib.check(lib.cpc_nce_backward_dwall(_p(c), _p(saved), _p(scratch), _p(dheads), B, S, K, N,
                                                                 side.cuda_stream), "nce_backward_dwall")
                            with torch.no_grad():
                                for k, h in enumerate(heads):
                                    if not h.requires_grad:
                                        continue
                                    g = dheads[k * _HID:(k + 1) * _HID]
                                    if h.grad is None:
                                        h.grad = g
                                    else:
                                        h.grad.add_(g)
                                        h.grad.record_stream(side)
                        for t in (c, scratch, dheads, saved):
                            t.record_stream(side)
                        ev = torch.cuda.Event()
                        ev.record(side)
                        step.late_events.append(ev)
                    step.deferred.append(dwall_path)
                    dwall = None
            else:
                with head_group(lib, ctx.group):
                    lib.check(lib.cpc_nce_backward(_p(c), _p(z), _p(wall), _p(ext), _p(perm), _p(row_ptr), _p(saved),
                                                   _p(gloss), _p(scratch), _p(dc), _p(dz), _p(dwall), B, S, K, N,
                                                   _stream()), "nce_backward")
        return dc, dz, dwall, None, None, None, None, None, None, None, None


def nce_bounds_into(wall, c_bound, B, S, K, N):
    """A workspace for InfoNCEFunction(saved=...) with the operand bounds of the criterion's GEMMs already in it
    (cpc_nce_bounds on the current stream): max|wall| reduced now -- the weights do not change inside a step -- and |c|
    bounded a priori by ``c_bound``."""
    lib = _lib.get()
    with torch.cuda.device(wall.device):
        sizes = _layout("nce_layout", lib.cpc_nce_layout, 6, B, S, K, N)
        saved = torch.empty(sizes[0], device=wall.device, dtype=torch.float32)
        lib.check(lib.cpc_nce_bounds(None, float(c_bound), _p(wall.detach()), _p(saved), B, S, K, N, _stream()), "nce_bounds")
    return saved


class InfoNCEScoresFunction(torch.autograd.Function):
    """pred (B,W,K*256) from any prediction network, z (B,S,256), ext, perm, row_ptr -> losses (K), acc (K)."""

    @staticmethod
    def forward(ctx, pred, z, ext, perm, row_ptr, n_valid=None, group=None):
        _require_cuda(pred, "InfoNCEScoresFunction")
        lib = _lib.get()
        B, S, H = z.shape
        W, N = ext.shape[1], ext.shape[2]
        if n_valid is not None:                       # (ext rows padded to the 16-wide tile: prepare_negatives)
            if int(lib.cpc_nce_padded_negatives(int(n_valid))) != N:
                raise ValueError("InfoNCEScoresFunction: ext is not padded for n_valid negatives")
            N = int(n_valid)
        K = S - W if group is None else pred.shape[2] // _HID        # (group = (k0, k_total): pred holds heads k0 .. k0+K-1)
        if (H != _HID or pred.shape != (B, W, K * _HID) or ext.dtype != torch.int32
                or (group is not None and W != S - group[1])):
            raise ValueError("InfoNCEScoresFunction: inconsistent shapes")
        pred, z, ext = pred.contiguous(), z.contiguous(), ext.contiguous()
        with torch.cuda.device(z.device), head_group(lib, group):
            sizes = _layout(f"nce_layout{group or ''}", lib.cpc_nce_layout, 6, B, S, K, N)
            saved = torch.empty(sizes[0], device=z.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=z.device, dtype=torch.float32)
            losses = torch.empty(K, device=z.device, dtype=torch.float32)
            acc = torch.empty(K, device=z.device, dtype=torch.float32)
            lib.check(lib.cpc_nce_scores_forward(_p(pred), _p(z), _p(ext), _p(saved), _p(scratch), _p(losses), _p(acc),
                                                 B, S, K, N, _stream()), "nce_scores_forward")
        ctx.save_for_backward(pred, z, ext, saved, perm, row_ptr)
        ctx.dims = (B, S, K, N, sizes[2])
        ctx.group = group
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(acc)
        return losses, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        lib = _lib.get()
        pred, z, ext, saved, perm, row_ptr = ctx.saved_tensors
        B, S, K, N, nscr = ctx.dims
        gloss = torch.zeros(K, device=z.device) if gloss is None else gloss.contiguous()
        with torch.cuda.device(z.device), head_group(lib, ctx.group):
            scratch = torch.empty(nscr, device=z.device, dtype=torch.float32)
            dpred, dz = torch.empty_like(pred), torch.empty_like(z)
            lib.check(lib.cpc_nce_scores_backward(_p(pred), _p(z), _p(ext), _p(perm), _p(row_ptr), _p(saved), _p(gloss),
                                                  _p(scratch), _p(dpred), _p(dz), B, S, K, N, _stream()),
                      "nce_scores_backward")
        return dpred, dz, None, None, None, None, None


NCE_WIDE_MAX = 512        # widest encoder the width-parametric score kernels take (csrc/nce_wide.hip: eight 64-float blocks)


def nce_wide_supported(C):
    """Do the width-parametric score kernels (cpc_nce_wide_*) take an encoder of width C?  1 <= C <= 512."""
    return 1 <= int(C) <= NCE_WIDE_MAX


def nce_wide_padded_width(C):
    """C rounded up to the kernels' 64-float channel block (cpc_nce_wide_padded_width)."""
    if not nce_wide_supported(C):
        raise NotImplementedError(f"the HIP score kernels take encoder widths 1 .. {NCE_WIDE_MAX}, got {C}")
    return (int(C) + 63) // 64 * 64


class InfoNCEWideScoresFunction(torch.autograd.Function):
    """InfoNCEScoresFunction at any encoder width C <= 512: pred (B,W,K*Cp) from any prediction network, z (B,S,Cp) with
    Cp = nce_wide_padded_width(C) and ZERO columns C .. Cp-1 of every head / row, ext, perm, row_ptr -> losses (K), acc (K)
    (cpc_nce_wide_{forward,backward}: exact-f32 MFMAs, dz through per-candidate rows and the destination-sorted gather).  The
    gradients have the inputs' padded shapes and are exactly zero in the padding columns; nce_wide_scores pads for the caller."""

    @staticmethod
    def forward(ctx, pred, z, ext, perm, row_ptr, C, n_valid=None, group=None):
        _require_cuda(pred, "InfoNCEWideScoresFunction")
        _require_cuda(z, "InfoNCEWideScoresFunction")
        lib = _lib.get()
        B, S, Cp = z.shape
        W, N = ext.shape[1], ext.shape[2]
        C = int(C)
        if n_valid is not None:                       # (ext rows padded to the 16-wide tile: prepare_negatives)
            if int(lib.cpc_nce_padded_negatives(int(n_valid))) != N:
                raise ValueError("InfoNCEWideScoresFunction: ext is not padded for n_valid negatives")
            N = int(n_valid)
        if Cp != nce_wide_padded_width(C):
            raise ValueError(f"InfoNCEWideScoresFunction: z must be padded to {nce_wide_padded_width(C)} channels for C = {C}")
        K = S - W if group is None else pred.shape[2] // Cp          # (group = (k0, k_total): pred holds heads k0 .. k0+K-1)
        if (pred.shape != (B, W, K * Cp) or ext.dtype != torch.int32 or (group is not None and W != S - group[1])):
            raise ValueError("InfoNCEWideScoresFunction: inconsistent shapes")
        pred, z, ext = pred.contiguous(), z.contiguous(), ext.contiguous()
        with torch.cuda.device(z.device), head_group(lib, group):
            sizes = _layout(f"nce_wide_layout{group or ''}", lib.cpc_nce_wide_layout, 5, B, S, K, N, C)
            saved = torch.empty(sizes[0], device=z.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=z.device, dtype=torch.float32)
            losses = torch.empty(K, device=z.device, dtype=torch.float32)
            acc = torch.empty(K, device=z.device, dtype=torch.float32)
            lib.check(lib.cpc_nce_wide_forward(_p(pred), _p(z), _p(ext), _p(saved), _p(scratch), _p(losses), _p(acc),
                                               B, S, K, N, C, _stream()), "nce_wide_forward")
        ctx.save_for_backward(pred, z, ext, saved, perm, row_ptr)
        ctx.dims = (B, S, K, N, C, sizes[2])
        ctx.group = group
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(acc)
        return losses, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        lib = _lib.get()
        pred, z, ext, saved, perm, row_ptr = ctx.saved_tensors
        B, S, K, N, C, nscr = ctx.dims
        gloss = torch.zeros(K, device=z.device) if gloss is None else gloss.contiguous()
        with torch.cuda.device(z.device), head_group(lib, ctx.group):
            scratch = torch.empty(nscr, device=z.device, dtype=torch.float32)
            dpred, dz = torch.empty_like(pred), torch.empty_like(z)
            lib.check(lib.cpc_nce_wide_backward(_p(pred), _p(z), _p(ext), _p(perm), _p(row_ptr), _p(saved), _p(gloss),
                                                _p(scratch), _p(dpred), _p(dz), B, S, K, N, C, _stream()),
                      "nce_wide_backward")
        return dpred, dz, None, None, None, None, None, None


def nce_wide_scores(pred, z, ext, perm, row_ptr, n_valid=None, group=None):
    """InfoNCEWideScoresFunction on unpadded tensors: pred (B,W,K*C), z (B,S,C) -> losses (K), acc (K).  The channel padding is
    made here with differentiable torch ops, and only when C is not a multiple of 64 (otherwise nothing is copied)."""
    _require_cuda(pred, "nce_wide_scores")
    _require_cuda(z, "nce_wide_scores")
    B, S, C = z.shape
    Cp = nce_wide_padded_width(C)
    if pred.dim() != 3 or pred.shape[2] % C != 0:
        raise ValueError("nce_wide_scores: pred must be (B, W, K*C)")
    if Cp != C:
        Bp, W, KC = pred.shape
        pred = torch.nn.functional.pad(pred.reshape(Bp, W, KC // C, C), (0, Cp - C)).reshape(Bp, W, KC // C * Cp)
        z = torch.nn.functional.pad(z, (0, Cp - C))
    return InfoNCEWideScoresFunction.apply(pred, z, ext, perm, row_ptr, C, n_valid, group)


class TransformerGroupFunction(torch.autograd.Function):
    """x (B,S,256), dropout probability, seed, G + the 13 parameter kinds of G TransformerLayers, each stacked (G, ...)
    (Krelpos possibly None) -> (B,S,G*256), layer g at columns g*256..: the K transformer predictors of the criterion on the
    same input, every kernel launched once for all of them (cpc_transformer_group_{forward,backward}).  Layer g's dropout
    masks are those of a single-layer call with seed + g."""

    @staticmethod
    def forward(ctx, x, drop_p, seed, G, *params):
        _require_cuda(x, "TransformerGroupFunction")
        lib = _lib.get()
        B, S, D = x.shape
        if D != _HID:
            raise NotImplementedError("the HIP transformer layer is built for d_model == 256")
        if S > 512:
            raise NotImplementedError("the HIP attention kernels hold sequences of at most 512 steps")
        if S > 128 and (float(drop_p) > 0 or (torch.is_grad_enabled() and (x.requires_grad or any(
                p is not None and p.requires_grad for p in params)))):
            # (callers -- transformers.TransformerLayer -- route such calls to the torch-op forward)
            raise NotImplementedError("beyond 128 steps the HIP transformer layer is forward-only (inference, no dropout)")
        x = x.contiguous()
        params = [None if p is None else p.detach().contiguous() for p in params]
        if any(p is not None and p.shape[0] != G for p in params):
            raise ValueError("TransformerGroupFunction: every parameter kind must be stacked (G, ...)")
        if params[4] is not None and tuple(params[4].shape[1:]) != (32, S):
            raise ValueError(f"Krelpos is {tuple(params[4].shape[1:])}; the layers were built for sequences of "
                             f"{params[4].shape[2]} steps, got {S} (cpc/transformers.py:22-24)")
        with torch.cuda.device(x.device):
            sizes = _layout("transformer_layout", lib.cpc_transformer_layout, 8, B, S)
            saved = torch.empty(G * sizes[0], device=x.device, dtype=torch.float32)
            scratch = torch.empty(G * sizes[1], device=x.device, dtype=torch.float32)
            out = torch.empty(B, S, G * _HID, device=x.device, dtype=torch.float32)
            lib.check(lib.cpc_transformer_group_forward(_p(x), _ptrs(params), _p(saved), _p(scratch), _p(out), B, S, G,
                                                        float(drop_p), int(seed), _stream()), "transformer_group_forward")
        ctx.drop = (float(drop_p), int(seed))
        if KEEP_DEBUG:                      # one entry per layer, as G single-layer calls would leave
            for g in range(G):
                debug_last.setdefault("transformer", []).append((saved[g * sizes[0]:(g + 1) * sizes[0]], sizes))
        ctx.has_rel = params[4] is not None
        ctx.step = current()
        ctx.save_for_backward(x, saved, *[p for p in params if p is not None])
        ctx.dims = (B, S, G, sizes[2])
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.get()
        x, saved, *ps = ctx.saved_tensors
        params = ps if ctx.has_rel else ps[:4] + [None] + ps[4:]
        B, S, G, nscr = ctx.dims
        dy = dy.contiguous()
        with torch.cuda.device(x.device):
            scratch = torch.empty(G * nscr, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            grads = [None if p is None else torch.empty_like(p) for p in params]
            lib.check(lib.cpc_transformer_group_backward(_p(x), _ptrs(params), _p(saved), _p(dy), _p(scratch), _p(dx),
                                                         _ptrs(grads), B, S, G, ctx.drop[0], ctx.drop[1], _stream()),
                      "transformer_group_backward")
        _wait(ctx.step, final=False)
        return (dx, None, None, None, *grads)


class TransformerLayerFunction(torch.autograd.Function):
    """x (B,S,256), dropout probability, seed + the 13 layer parameters (state-dict order, Krelpos possibly None) -> (B,S,256).
    One TransformerLayer of cpc/transformers.py:103-111 through cpc_transformer_layer_{forward,backward}_dropout."""

    @staticmethod
    def forward(ctx, x, drop_p, seed, *params):
        """drop_p, seed: dropout probability of this call (0: none) and the 64-bit seed its masks derive from."""
        _require_cuda(x, "TransformerLayerFunction")
        lib = _lib.get()
        B, S, D = x.shape
        if D != _HID:
            raise NotImplementedError("the HIP transformer layer is built for d_model == 256")
        if S > 512:
            raise NotImplementedError("the HIP attention kernels hold sequences of at most 512 steps")
        if S > 128 and (float(drop_p) > 0 or (torch.is_grad_enabled() and (x.requires_grad or any(
                p is not None and p.requires_grad for p in params)))):
            # (callers -- transformers.TransformerLayer -- route such calls to the torch-op forward)
            raise NotImplementedError("beyond 128 steps the HIP transformer layer is forward-only (inference, no dropout)")
        x = x.contiguous()
        params = [None if p is None else p.detach().contiguous() for p in params]
        if params[4] is not None and tuple(params[4].shape) != (32, S):
            raise ValueError(f"Krelpos is {tuple(params[4].shape)}; the layer was built for sequences of "
                             f"{params[4].shape[1]} steps, got {S} (cpc/transformers.py:22-24)")
        with torch.cuda.device(x.device):
            sizes = _layout("transformer_layout", lib.cpc_transformer_layout, 8, B, S)
            saved = torch.empty(sizes[0], device=x.device, dtype=torch.float32)
            scratch = torch.empty(sizes[1], device=x.device, dtype=torch.float32)
            out = torch.empty(B, S, _HID, device=x.device, dtype=torch.float32)
            lib.check(lib.cpc_transformer_layer_forward_dropout(_p(x), _ptrs(params), _p(saved), _p(scratch), _p(out), B, S,
                                                                float(drop_p), int(seed), _stream()),
                      "transformer_layer_forward")
        ctx.drop = (float(drop_p), int(seed))
        if KEEP_DEBUG:                      # parity tests read the FFN's ReLU mask (oracle _ReluTieAware)
            debug_last.setdefault("transformer", []).append((saved, sizes))
        ctx.has_rel = params[4] is not None
        ctx.step = current()
        ctx.save_for_backward(x, saved, *[p for p in params if p is not None])
        ctx.dims = (B, S, sizes[2])
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.get()
        x, saved, *ps = ctx.saved_tensors
        params = ps if ctx.has_rel else ps[:4] + [None] + ps[4:]
        B, S, nscr = ctx.dims
        dy = dy.contiguous()
        with torch.cuda.device(x.device):
            scratch = torch.empty(nscr, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            grads = [None if p is None else torch.empty_like(p) for p in params]
            lib.check(lib.cpc_transformer_layer_backward_dropout(_p(x), _ptrs(params), _p(saved), _p(dy), _p(scratch), _p(dx),
                                                                 _ptrs(grads), B, S, ctx.drop[0], ctx.drop[1], _stream()),
                      "transformer_layer_backward")
        _wait(ctx.step, final=False)
        return (dx, None, None, *grads)


# ---- PER evaluation (csrc/ctc_decode.hip); the drivers live in seq_alignment.py ---------------------------------------
def ctc_beam_search(probs, lengths, n_keep, blank, n_out=1):
    """Batched CTC prefix beam search on the device: seq_alignment.beam_search_batch."""
    from .seq_alignment import beam_search_batch
    return beam_search_batch(probs, lengths, n_keep, blank, n_out)


def nw_align_score(ref, ref_len, hyp, hyp_len, d=-1, m=-1, r=0, normalize=True):
    """Batched Needleman-Wunsch score on the device (get_seq_PER by default): seq_alignment.seq_per_batch."""
    from .seq_alignment import seq_per_batch
    return seq_per_batch(ref, ref_len, hyp, hyp_len, d, m, r, normalize)
