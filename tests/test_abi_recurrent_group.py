"""The C ABI and the module surface of the recurrent prediction networks and the RNN autoregressor (csrc/lstm.hip: cpc_lstm_group_*;
csrc/rnn.hip: cpc_rnn_*; ``hipPredictors`` with --rnnMode LSTM / RNN; CPCAR(mode="RNN", rnnKernel=True)) -- no GPU needed."""
import ctypes
import json
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpc_lstm_group_layout", "cpc_lstm_group_forward", "cpc_lstm_group_backward", "cpc_rnn_layout", "cpc_rnn_forward",
           "cpc_rnn_backward")


def _built():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    return _lib.bind(build.build())


def test_symbols_are_declared_bound_and_exported():
    from cpc_audio_amd import _lib
    header = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\(", header, re.M), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"^int\s+" + name + r"\(([^;]*)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name      # header and table agree
    assert re.search(r"^#define CPC_DEVERR_RNN_POLL_TIMEOUT 256$", header, re.M)
    assert re.search(r"^#define CPC_RNN_PER_STEP 1$", header, re.M) and re.search(r"^#define CPC_RNN_TIME_MAJOR 2$", header, re.M)
    # the existing LSTM entry points keep their argument lists
    assert len(_lib.SIGNATURES["cpc_lstm_forward"][1]) == 14 and len(_lib.SIGNATURES["cpc_lstm_backward"][1]) == 15
    bound = _built()                        # raises if a declared symbol is missing from the gfx950 build
    for name in SYMBOLS:
        assert hasattr(bound, name)
    assert bound.cpc_abi_version() == 16 and _lib.EXPECTED_ABI == 16      # symbols were added, none changed


def test_device_error_bit_is_named():
    import inspect
    from cpc_audio_amd import ops
    src = inspect.getsource(ops.check_device_errors)
    assert "mask & 256" in src and "RNN" in src


def test_lstm_group_limits_and_argument_errors_answer_before_any_launch():
    bound = _built()
    sizes = (ctypes.c_long * 3)()
    assert bound.cpc_lstm_group_layout(64, 116, 12, sizes) == 0
    M = 64 * 116
    assert sizes[0] == M * 12 * 1024 + M * 12 * 256 and sizes[1] == M * 12 * 1024 and sizes[2] > sizes[1] + 2 * 12 * 256 * 1024
    assert bound.cpc_lstm_group_layout(1, 1, 64, sizes) == 0                        # the stated limits
    assert bound.cpc_lstm_group_layout(1 << 10, 1 << 5, 64, sizes) == 0             # B S G = 2^21
    for bad in ((0, 116, 12), (2, 0, 12), (2, 116, 0), (2, 116, 65), (1 << 10, 1 << 5, 65), ((1 << 10) + 1, 1 << 5, 64),
                (1 << 20, 1 << 20, 1)):                                             # B S alone overflows an int
        assert bound.cpc_lstm_group_layout(*bad, sizes) == 1, bad                   # CPC_ERR_SHAPE
    assert bound.cpc_lstm_group_layout(2, 116, 12, None) == 2                       # CPC_ERR_ARG
    p = ctypes.c_void_p(8)
    fwd = lambda *a, B=2, S=116, G=12, flags=0: bound.cpc_lstm_group_forward(*a, B, S, G, flags, None)
    bwd = lambda *a, B=2, S=116, G=12, flags=0: bound.cpc_lstm_group_backward(*a, B, S, G, flags, None)
    assert fwd(*[p] * 8, G=65) == 1 and fwd(*[p] * 8, B=0) == 1 and fwd(*[p] * 8, S=0) == 1
    assert fwd(*[p] * 8, flags=2) == 2
    for k in range(8):
        assert fwd(*[None if q == k else p for q in range(8)]) == 2, k
    assert bwd(*[p] * 12, G=0) == 1 and bwd(*[p] * 12, flags=4) == 2
    for k in range(12):
        assert bwd(*[None if q == k else p for q in range(12)]) == 2, k


def test_rnn_limits_and_argument_errors_answer_before_any_launch():
    bound = _built()
    sizes = (ctypes.c_long * 3)()
    assert bound.cpc_rnn_layout(64, 116, 12, 1, sizes) == 0
    M = 64 * 116
    assert sizes[1] == M * 12 * 256 and sizes[2] > sizes[1] + 2 * 12 * 65536
    assert bound.cpc_rnn_layout(128, 64, 1, 8, sizes) == 0 and sizes[0] == 7 * 128 * 64 * 256
    assert bound.cpc_rnn_layout(1, 1, 64, 1, sizes) == 0
    for bad in ((0, 4, 1, 1), (4, 0, 1, 1), (4, 4, 0, 1), (4, 4, 65, 1), (4, 4, 1, 0), (4, 4, 1, 9),
                (4, 4, 2, 2),                              # several heads with stacked layers
                (1 << 11, 1 << 10, 2, 1), (1 << 20, 1 << 20, 1, 1)):
        assert bound.cpc_rnn_layout(*bad, sizes) == 1, bad                          # CPC_ERR_SHAPE
    assert bound.cpc_rnn_layout(4, 4, 1, 1, None) == 2                              # CPC_ERR_ARG
    p = ctypes.c_void_p(8)
    arr = (ctypes.c_void_p * 8)(*[8] * 8)
    hole = (ctypes.c_void_p * 8)(8, 8, None, 8, 8, 8, 8, 8)

    def fwd(x=p, h0=None, params=arr, saved=p, scratch=p, y=p, hN=None, T=4, R=4, G=1, nl=1, flags=0):
        return bound.cpc_rnn_forward(x, h0, params, saved, scratch, y, hN, T, R, G, nl, flags, None)

    def bwd(x=p, h0=None, params=arr, saved=p, y=p, dy=p, scratch=p, dx=p, grads=arr, T=4, R=4, G=1, nl=1, flags=0):
        return bound.cpc_rnn_backward(x, h0, params, saved, y, dy, scratch, dx, grads, T, R, G, nl, flags, None)

    for call in (fwd, bwd):
        assert call(T=0) == 1 and call(R=0) == 1 and call(G=65) == 1 and call(nl=9) == 1 and call(G=2, nl=2) == 1
        assert call(flags=4) == 2
        assert call(x=None) == 2 and call(params=None) == 2 and call(params=hole) == 2 and call(saved=None) == 2
        assert call(scratch=None) == 2 and call(y=None) == 2
        assert call(G=2, h0=p) == 2                         # a carried state exists for one head only
    assert fwd(G=2, hN=p) == 2
    assert bwd(dy=None) == 2 and bwd(dx=None) == 2 and bwd(grads=None) == 2 and bwd(grads=hole) == 2
    assert fwd(nl=2, params=hole) == 2                      # 8 parameter pointers expected, one of them NULL


@pytest.mark.parametrize("mode", ["RNN", "LSTM"])
def test_flag_keeps_the_state_dict_and_the_cpu_path(mode):
    """hipPredictors=True: the reference's state-dict keys and shapes; CPU input takes the torch modules, bit-equal to the
    flag off."""
    import torch
    from cpc_audio_amd.criterion import PredictionNetwork
    from cpc_audio_amd.train import build_criterion
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "predictors_meta.json")))
    shapes = {k: tuple(v) for k, v in meta["modes"][mode]["keys"].items()}
    torch.manual_seed(5)
    on = PredictionNetwork(3, 256, 256, mode, hipPredictors=True)
    off = PredictionNetwork(3, 256, 256, mode)
    assert on.hipPredictors and not off.hipPredictors and on.scores_apart and on.last_path is None
    assert {k: tuple(v.shape) for k, v in on.state_dict().items()} == shapes
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    off.load_state_dict(on.state_dict(), strict=True)
    c = torch.randn(2, 6, 256)
    a, b = on.predictions(c), off.predictions(c)
    assert on.last_path == "torch" and off.last_path == "torch"
    assert a.shape == (2, 6, 3 * 256) and torch.equal(a, b)
    assert build_criterion(rnnMode=mode, hipPredictors=True).wPrediction.hipPredictors
    assert not build_criterion(rnnMode=mode).wPrediction.hipPredictors        # off by default


@pytest.mark.parametrize("nl,reverse", [(1, False), (2, True)])
def test_rnn_autoregressor_on_cpu_input_is_nn_rnn(nl, reverse):
    """CPCAR(mode="RNN", rnnKernel=True) on CPU input runs baseNet's own forward: equal to nn.RNN, carried state included."""
    import torch
    from cpc_audio_amd.model import CPCAR
    from cpc_audio_amd.train import build_model
    torch.manual_seed(2)
    ar = CPCAR(256, 256, True, nl, mode="RNN", reverse=reverse, rnnKernel=True)
    plain = CPCAR(256, 256, True, nl, mode="RNN", reverse=reverse)
    assert ar.hip_rnn and not ar.hip and not ar.hip_lstm and not plain.hip_rnn
    assert isinstance(ar.baseNet, torch.nn.RNN) and list(ar.state_dict().keys()) == list(plain.state_dict().keys())
    plain.load_state_dict(ar.state_dict())
    ref = torch.nn.RNN(256, 256, num_layers=nl, batch_first=True)
    ref.load_state_dict(ar.baseNet.state_dict())
    h = None
    for _ in range(2):
        x = torch.randn(2, 5, 256)
        xin = torch.flip(x, [1]) if reverse else x
        want, h = ref(xin, h)
        want = torch.flip(want, [1]) if reverse else want
        assert torch.equal(ar(x), want) and torch.equal(plain(x), want)
    assert not CPCAR(256, 256, False, 1, mode="LSTM", rnnKernel=True).hip_rnn
    assert not CPCAR(256, 128, False, 1, mode="RNN", rnnKernel=True).hip_rnn
    assert build_model(arMode="RNN", nLevelsGRU=1, rnnKernel=True).gAR.hip_rnn
    assert not build_model(arMode="RNN", nLevelsGRU=1).gAR.hip_rnn
