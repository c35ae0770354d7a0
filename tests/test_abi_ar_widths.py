"""The surface of the width-generic autoregressors (no GPU): the inputKernel keyword of model.CPCAR / train.build_model, the
cpc_*_in and cpc_in_proj_* symbols, and the argument checks that return before any launch."""
import ctypes
import os
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cpc_in_proj_scratch_floats", "cpc_in_proj_forward", "cpc_in_proj_backward"] + \
    [f"cpc_{c}_{f}_in" for c in ("gru", "lstm", "rnn") for f in ("layout", "forward", "backward")]


def test_the_keyword_sets_an_attribute_of_its_own():
    from cpc_audio_amd.model import CPCAR
    ar = CPCAR(40, 256, False, 2, inputKernel=True)
    assert ar.hip_in is True and ar.hip is False and ar.hip_lstm is False and ar.hip_rnn is False
    other = CPCAR(40, 128, False, 2, inputKernel=True)                  # another context width: torch, as before
    assert other.hip_in is False and other.hip is False
    assert CPCAR(40, 256, False, 2).hip_in is False                     # off by default
    assert CPCAR(513, 256, False, 2, inputKernel=True).hip_in is False and CPCAR(40, 256, False, 9, inputKernel=True).hip_in is False
    same = CPCAR(256, 256, False, 2, inputKernel=True)                  # 256 -> 256 stays what it was
    assert same.hip is True and same.hip_in is False
    # LSTM and RNN take their own keyword as well
    assert CPCAR(40, 256, False, 1, mode="LSTM", inputKernel=True).hip_in is False
    lstm = CPCAR(40, 256, False, 1, mode="LSTM", inputKernel=True, lstmKernel=True)
    assert lstm.hip_in is True and lstm.hip_lstm is False and lstm.hip is False
    assert CPCAR(40, 256, False, 1, mode="RNN", inputKernel=True, lstmKernel=True).hip_in is False
    rnn = CPCAR(13, 256, False, 3, mode="RNN", inputKernel=True, rnnKernel=True)
    assert rnn.hip_in is True and rnn.hip_rnn is False and rnn.hip is False


@pytest.mark.parametrize("mode", ["GRU", "LSTM", "RNN"])
def test_cpu_input_runs_the_torch_module(mode):
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(0)
    ar = CPCAR(40, 256, True, 2, mode=mode, inputKernel=True, lstmKernel=True, rnnKernel=True)
    assert ar.hip_in
    x = torch.randn(2, 5, 40)
    y = ar(x)
    want, h = ar.baseNet(x)
    assert torch.equal(y, want)
    kept = ar.hidden if isinstance(ar.hidden, tuple) else (ar.hidden,)
    for a, b in zip(kept, h if isinstance(h, tuple) else (h,)):
        assert torch.equal(a, b)
    assert not hasattr(y, "_cpc_abs_bound")


def test_build_model_passes_the_keyword_and_keeps_the_state_dict():
    from cpc_audio_amd import train
    m = train.build_model(encoder_type="mfcc", hiddenEncoder=40, mfccKernel=True, inputKernel=True)
    assert m.gAR.hip_in is True and m.gAR.hip is False
    assert train.build_model(encoder_type="mfcc", hiddenEncoder=40, mfccKernel=True).gAR.hip_in is False
    assert train.build_model().gAR.hip_in is False and train.build_model(inputKernel=True).gAR.hip is True
    ref = torch.nn.GRU(40, 256, 2, batch_first=True)
    got = {k: tuple(v.shape) for k, v in m.gAR.state_dict().items()}
    assert list(got) == ["baseNet." + k for k in ref.state_dict()]
    assert got == {"baseNet." + k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert got["baseNet.weight_ih_l0"] == (768, 40)


def test_header_and_signature_table_carry_the_new_entries():
    from cpc_audio_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and f"{name}(" in text, name
    # symbols were added, none changed: the old entries keep their signatures and the version its value
    assert _lib.SIGNATURES["cpc_gru_forward"] == (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_int] * 3 + [ctypes.c_void_p])
    assert _lib.SIGNATURES["cpc_gru_forward_in"] == (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_int] * 4 + [ctypes.c_void_p])


def test_library_exports_the_new_symbols_and_checks_widths_before_any_launch():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    lib = _lib.bind(build.build())
    assert lib.cpc_abi_version() == _lib.EXPECTED_ABI
    for name in NEW:
        assert hasattr(lib, name)
    sizes, old = (ctypes.c_long * 3)(), (ctypes.c_long * 3)()
    for lay in (lib.cpc_gru_layout_in, lib.cpc_lstm_layout_in, lib.cpc_rnn_layout_in):
        assert lay(4, 8, 2, 0, sizes) == 1 and lay(4, 8, 2, 513, sizes) == 1          # CPC_ERR_SHAPE
        assert lay(4, 8, 2, 40, None) == 2                                            # CPC_ERR_ARG
        assert lay(4, 8, 2, 40, sizes) == 0 and lay(4, 8, 2, 512, sizes) == 0 and lay(4, 8, 2, 1, sizes) == 0
    assert lib.cpc_gru_layout_in(4, 8, 2, 256, sizes) == 0 and lib.cpc_gru_layout(4, 8, 2, old) == 0 and tuple(sizes) == tuple(old)
    assert lib.cpc_lstm_layout_in(4, 8, 2, 256, sizes) == 0 and lib.cpc_lstm_layout(4, 8, 2, old) == 0 and tuple(sizes) == tuple(old)
    assert lib.cpc_rnn_layout_in(8, 4, 2, 256, sizes) == 0 and lib.cpc_rnn_layout(8, 4, 1, 2, old) == 0 and tuple(sizes) == tuple(old)
    assert lib.cpc_in_proj_scratch_floats(8192, 768, 40) > 768 * 64 and lib.cpc_in_proj_scratch_floats(8192, 768, 513) == 0
    assert lib.cpc_in_proj_forward(None, 40, None, None, None, None, 32, 768, 0, None) == 1
    assert lib.cpc_in_proj_forward(None, 40, None, None, None, None, 32, 768, 40, None) == 2
    assert lib.cpc_in_proj_backward(None, 40, None, None, None, None, None, 32, 768, 513, None) == 1
    assert lib.cpc_in_proj_backward(None, 40, None, None, None, None, None, 32, 768, 40, None) == 2
    assert lib.cpc_gru_forward_in(None, None, None, None, None, None, None, 4, 8, 2, 513, None) == 1
    assert lib.cpc_gru_forward_in(None, None, None, None, None, None, None, 4, 8, 2, 40, None) == 2
