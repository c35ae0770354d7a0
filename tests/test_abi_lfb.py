"""The C ABI of the learned-filter-bank kernels (csrc/lfb.hip): the five entry points are declared in include/cpc_hip.h, listed
in the ctypes signature table and exported by the library, the ABI version stays 16 (adding symbols is compatible), and the
argument checks answer before any launch -- with NULL tensor pointers, which a launch would fault on."""
import ctypes
import os
import re
import shutil

import pytest

from cpc_audio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cpc_lfb_layout", "cpc_lfb_energy_forward", "cpc_lfb_energy_backward", "cpc_lfb_lognorm_forward",
           "cpc_lfb_lognorm_backward"]
needs_lib = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                               reason="needs the built library")


def test_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "cpc_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.EXPECTED_ABI == 16
    assert len(_lib.SIGNATURES["cpc_lfb_energy_forward"][1]) == 10 and len(_lib.SIGNATURES["cpc_lfb_energy_backward"][1]) == 12
    assert len(_lib.SIGNATURES["cpc_lfb_lognorm_forward"][1]) == 8 and len(_lib.SIGNATURES["cpc_lfb_lognorm_backward"][1]) == 9


@needs_lib
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.get()
    for name in SYMBOLS:
        assert callable(getattr(lib, name)), name
    assert lib.cpc_abi_version() == 16


@needs_lib
@pytest.mark.parametrize("N,L,D", [(1, 400, 48), (1, 400, 544), (1, 399, 32), (0, 400, 32), (1, 400, 0),
                                   (1 << 20, 64000, 32), (1 << 12, (1 << 19) + 399, 32)])
def test_shape_checks_answer_before_any_launch(N, L, D):
    lib = _lib.get()
    sizes = (ctypes.c_long * 3)(-1, -1, -1)
    assert lib.cpc_lfb_layout(N, L, D, sizes) == 1 and list(sizes) == [-1, -1, -1]
    assert lib.cpc_lfb_energy_forward(None, None, None, None, None, None, N, L, D, None) == 1
    assert lib.cpc_lfb_energy_backward(None, None, None, None, None, None, None, None, N, L, D, None) == 1
    if N < 1 or D % 32 or not 32 <= D <= 512:                   # (the lognorm calls take F, not L)
        assert lib.cpc_lfb_lognorm_forward(None, None, None, N, 2, D, 1, None) == 1
        assert lib.cpc_lfb_lognorm_backward(None, None, None, None, N, 2, D, 1, None) == 1


@needs_lib
def test_null_pointers_and_flags_are_refused():
    lib = _lib.get()
    assert lib.cpc_lfb_layout(1, 400, 32, None) == 2
    assert lib.cpc_lfb_energy_forward(None, None, None, None, None, None, 1, 400, 32, None) == 2
    assert lib.cpc_lfb_energy_backward(None, None, None, None, None, None, None, None, 1, 400, 32, None) == 2
    assert lib.cpc_lfb_lognorm_forward(None, None, None, 1, 2, 32, 1, None) == 2
    assert lib.cpc_lfb_lognorm_backward(None, None, None, None, 1, 2, 32, 0, None) == 2
    assert lib.cpc_lfb_lognorm_forward(None, None, None, 1, 1, 32, 1, None) == 1          # F is never 1
    assert lib.cpc_lfb_lognorm_forward(None, None, None, 1 << 16, 1 << 10, 32, 1, None) == 1     # N F D = 2^31
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_lfb_layout(2, 2000, 32, sizes) == 0 and sizes[0] == 12 and sizes[1] == 0 and sizes[2] > 0
