"""The LSTM entry points of the gfx950 library (cpc_lstm_layout / _forward / _backward): exported, declared in the header
and the signature table, and their argument checks answer before any launch -- so this runs without a GPU."""
import ctypes
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM_SYMBOLS = ("cpc_lstm_layout", "cpc_lstm_forward", "cpc_lstm_backward")


def _bound():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    return _lib.bind(build.build())


def test_lstm_symbols_are_declared_and_in_the_signature_table():
    from cpc_audio_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    assert re.search(r"#define CPC_DEVERR_LSTM_POLL_TIMEOUT 8\b", text)
    assert re.search(r"#define CPC_LSTM_PER_STEP 1\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in LSTM_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    assert _lib.EXPECTED_ABI == 16


def test_lstm_symbols_are_exported_and_the_abi_version_moved():
    bound = _bound()
    from cpc_audio_amd import _lib
    assert bound.cpc_abi_version() == _lib.EXPECTED_ABI == 16
    for name in LSTM_SYMBOLS:
        assert callable(getattr(bound, name))


def test_lstm_layout_sizes_and_shape_errors():
    bound = _bound()
    sizes = (ctypes.c_long * 3)()
    for bad in [(0, 128, 1), (64, 0, 1), (64, 128, 0), (64, 128, 9), (-1, 128, 1), (1 << 12, 1 << 10, 1)]:
        assert bound.cpc_lstm_layout(*bad, sizes) == 1, bad        # CPC_ERR_SHAPE
    assert bound.cpc_lstm_layout(64, 128, 1, None) == 2            # CPC_ERR_ARG
    B, S = 64, 128
    rows = B * S
    assert bound.cpc_lstm_layout(B, S, 1, sizes) == 0
    one = tuple(sizes)
    # saved: 4 activated gates + c per step; forward scratch: the input projection of every step
    assert one[0] >= rows * (4 + 1) * 256 and one[1] >= rows * 4 * 256
    assert bound.cpc_lstm_layout(B, S, 2, sizes) == 0
    two = tuple(sizes)
    assert two[0] >= 2 * one[0] + rows * 256                        # + layer 0's output, the input of layer 1
    assert two[1] == one[1] and two[2] == one[2]                    # scratch serves one layer at a time


def test_lstm_argument_errors_without_a_gpu():
    bound = _bound()
    B, S, nl = 2, 3, 1
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)                           # never dereferenced: every call below is refused first
    params = (ctypes.c_void_p * 4)(p, p, p, p)
    grads = (ctypes.c_void_p * 4)(p, p, p, p)
    fwd = lambda **kw: bound.cpc_lstm_forward(*{**dict(x=p, h0=None, c0=None, params=params, saved=p, scratch=p, y=p, hN=p,  # noqa: E731
                                                      cN=p, B=B, S=S, nl=nl, flags=0), **kw}.values(), None)
    bwd = lambda **kw: bound.cpc_lstm_backward(*{**dict(x=p, h0=None, c0=None, params=params, saved=p, y=p, dy=p, scratch=p,  # noqa: E731
                                                       dx=p, grads=grads, B=B, S=S, nl=nl, flags=0), **kw}.values(), None)
    for call in (fwd, bwd):
        assert call(B=0) == 1 and call(S=-2) == 1 and call(nl=0) == 1 and call(nl=9) == 1
        assert call(flags=4) == 2 and call(flags=-1) == 2
        assert call(x=None) == 2 and call(params=None) == 2 and call(saved=None) == 2 and call(scratch=None) == 2
        assert call(h0=p) == 2 and call(c0=p) == 2                 # the carried state is (h0, c0) or nothing
        assert call(params=(ctypes.c_void_p * 4)(p, None, p, p)) == 2
    assert fwd(y=None) == 2 and fwd(hN=None) == 2 and fwd(cN=None) == 2
    assert bwd(y=None) == 2 and bwd(dy=None) == 2 and bwd(dx=None) == 2 and bwd(grads=None) == 2
    assert bwd(grads=(ctypes.c_void_p * 4)(p, p, p, None)) == 2
