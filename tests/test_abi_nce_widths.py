"""The C ABI of the width-parametric InfoNCE scores (csrc/nce_wide.hip): the four entry points are declared in include/cpc_hip.h,
listed in the ctypes signature table and exported by the library built for gfx950; the ABI version stays 16 (symbols are
added, none changed); the shape and pointer checks answer before any launch."""
import ctypes
import os
import re
import shutil

import pytest

from cpc_audio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cpc_nce_wide_padded_width", "cpc_nce_wide_layout", "cpc_nce_wide_forward", "cpc_nce_wide_backward"]
needs_lib = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                               reason="needs the built library")


def test_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "cpc_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.EXPECTED_ABI == 16
    assert len(_lib.SIGNATURES["cpc_nce_wide_layout"][1]) == 6
    assert len(_lib.SIGNATURES["cpc_nce_wide_forward"][1]) == 13 and len(_lib.SIGNATURES["cpc_nce_wide_backward"][1]) == 16


@needs_lib
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.get()
    for name in SYMBOLS:
        assert callable(getattr(lib, name)), name
    assert lib.cpc_abi_version() == 16


@needs_lib
@pytest.mark.parametrize("C,Cp", [(0, 0), (-3, 0), (1, 64), (13, 64), (64, 64), (65, 128), (320, 320), (512, 512), (513, 0)])
def test_padded_width(C, Cp):
    assert _lib.get().cpc_nce_wide_padded_width(C) == Cp


@needs_lib
@pytest.mark.parametrize("B,S,K,N,C", [(2, 20, 5, 16, 0), (2, 20, 5, 16, 513), (2, 40, 17, 16, 40), (2, 20, 5, 0, 40),
                                       (2, 5, 5, 16, 40), (0, 20, 5, 16, 40)], ids=["C0", "C513", "K17", "N0", "S<=K", "B0"])
def test_shape_checks_answer_before_any_launch(B, S, K, N, C):
    lib = _lib.get()
    sizes = (ctypes.c_long * 5)(-1, -1, -1, -1, -1)
    assert lib.cpc_nce_wide_layout(B, S, K, N, C, sizes) == 1 and list(sizes) == [-1] * 5
    assert lib.cpc_nce_wide_forward(None, None, None, None, None, None, None, B, S, K, N, C, None) == 1
    assert lib.cpc_nce_wide_backward(None, None, None, None, None, None, None, None, None, None, B, S, K, N, C, None) == 1


@needs_lib
def test_null_pointers_are_refused():
    lib = _lib.get()
    assert lib.cpc_nce_wide_layout(2, 20, 5, 16, 40, None) == 2
    assert lib.cpc_nce_wide_forward(None, None, None, None, None, None, None, 2, 20, 5, 16, 40, None) == 2
    assert lib.cpc_nce_wide_backward(None, None, None, None, None, None, None, None, None, None, 2, 20, 5, 16, 40, None) == 2


@needs_lib
def test_layout_sizes_grow_with_the_width():
    lib = _lib.get()
    B, S, K, N = 4, 32, 12, 24
    W, Np = S - K, 32
    prev = None
    for C in (13, 64, 65, 256, 320, 512):
        sizes = (ctypes.c_long * 5)()
        assert lib.cpc_nce_wide_layout(B, S, K, N, C, sizes) == 0
        Cp = lib.cpc_nce_wide_padded_width(C)
        assert sizes[0] >= B * W * K * (Np + 1) + B * W * K and sizes[3] == 0 and sizes[4] >= B * W * K * (Np + 1)
        assert sizes[2] >= B * W * (Np + K) * Cp                      # the candidate rows V
        if prev is not None:
            assert sizes[2] >= prev[2] and sizes[0] == prev[0] and sizes[1] == prev[1]    # only V depends on the width
        prev = list(sizes)
    small, big = (ctypes.c_long * 5)(), (ctypes.c_long * 5)()
    assert lib.cpc_nce_wide_layout(B, S, K, N, 40, small) == 0 and lib.cpc_nce_wide_layout(B, S, K, N, 512, big) == 0
    assert big[2] > small[2]
    # V passes 2^31 floats at B = 256, S = 130, C = 512: sized in 64-bit
    assert lib.cpc_nce_wide_layout(256, 130, 12, 128, 512, big) == 0 and big[2] > 2 ** 31
