"""The C ABI of the MFCC kernels (csrc/mfcc.hip): the three entry points are declared in include/cpc_hip.h, listed in the ctypes
signature table and exported by the library, the ABI version stays 16 (adding symbols is compatible), and the argument checks
answer before any launch -- with NULL tensor pointers, which a launch would fault on."""
import ctypes
import os
import re
import shutil

import pytest

from cpc_audio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cpc_mfcc_layout", "cpc_mfcc_meldb", "cpc_mfcc_dct"]
needs_lib = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                               reason="needs the built library")


def test_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "cpc_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.EXPECTED_ABI == 16
    assert len(_lib.SIGNATURES["cpc_mfcc_layout"][1]) == 4
    assert len(_lib.SIGNATURES["cpc_mfcc_meldb"][1]) == 9 and len(_lib.SIGNATURES["cpc_mfcc_dct"][1]) == 9


@needs_lib
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.get()
    for name in SYMBOLS:
        assert callable(getattr(lib, name)), name
    assert lib.cpc_abi_version() == 16


@needs_lib
@pytest.mark.parametrize("N,L,D", [(1, 160, 40), (1, 161, 0), (1, 161, 513), (0, 161, 40), (1 << 20, 64000, 40)],
                         ids=["L160", "D0", "D513", "N0", "overflow"])
def test_shape_checks_answer_before_any_launch(N, L, D):
    lib = _lib.get()
    sizes = (ctypes.c_long * 3)(-1, -1, -1)
    assert lib.cpc_mfcc_layout(N, L, D, sizes) == 1 and list(sizes) == [-1, -1, -1]
    assert lib.cpc_mfcc_meldb(None, None, None, None, None, N, L, D, None) == 1
    F = max((L - 1) // 160 + 1, 1)
    assert lib.cpc_mfcc_dct(None, None, None, None, N, 1 if L < 161 else F, D, 0, None) == 1


@needs_lib
def test_null_pointers_and_flags_are_refused():
    lib = _lib.get()
    assert lib.cpc_mfcc_layout(1, 161, 40, None) == 2
    assert lib.cpc_mfcc_meldb(None, None, None, None, None, 1, 161, 40, None) == 2
    assert lib.cpc_mfcc_dct(None, None, None, None, 1, 2, 40, 0, None) == 2
    buf = (ctypes.c_float * 4096)()
    out = (ctypes.c_float * 4096)()
    p, q = ctypes.addressof(buf), ctypes.addressof(out)
    assert lib.cpc_mfcc_dct(p, p, p, q, 1, 2, 40, 2, None) == 2                     # rowwise is 0 or 1
    assert lib.cpc_mfcc_dct(p, p, p, q, 1, 2, 40, -1, None) == 2
    assert lib.cpc_mfcc_dct(None, None, None, None, 1, 2, 40, 2, None) == 2


@needs_lib
def test_layout_of_the_workload():
    lib = _lib.get()
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_mfcc_layout(2, 20480, 256, sizes) == 0 and sizes[0] == 128 and sizes[1] == 256 and sizes[2] == 2 * 4 * 4
    assert lib.cpc_mfcc_layout(1, 161, 13, sizes) == 0 and list(sizes) == [2, 128, 4]
    assert lib.cpc_mfcc_layout(1, 64000, 512, sizes) == 0 and list(sizes) == [400, 512, 13 * 4]
