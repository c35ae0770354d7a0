"""The surface of the encoder's other normModes (no GPU): the cpc_encoder_*_n symbols and their argument and shape checks, which
return before any launch."""
import ctypes
import os
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cpc_encoder_layout_n", "cpc_encoder_forward_n", "cpc_encoder_backward_n", "cpc_encoder_saved_activation_n"]
SHAPE, ARG = 1, 2            # CPC_ERR_SHAPE, CPC_ERR_ARG
LAYER, BATCH, INSTANCE, ID = 0, 1, 2, 3


def _library():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    return _lib.bind(build.build())


def test_header_and_signature_table_carry_the_new_entries():
    from cpc_audio_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and f"int {name}(" in text, name
    i, p, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert _lib.EXPECTED_ABI == 16
    assert _lib.SIGNATURES["cpc_encoder_layout_n"] == (i, [i, i, i, i, i, p])
    assert _lib.SIGNATURES["cpc_encoder_forward_n"] == (i, [p] * 6 + [i, i, i, i, i, f, f, p])
    assert _lib.SIGNATURES["cpc_encoder_backward_n"] == (i, [p] * 7 + [i, i, i, i, i, p])
    assert _lib.SIGNATURES["cpc_encoder_saved_activation_n"] == (i, [p, i, p, i, i, i, i, p])
    # symbols were added, none changed
    assert _lib.SIGNATURES["cpc_encoder_layout_c"] == (i, [i, i, i, p])
    assert _lib.SIGNATURES["cpc_encoder_forward_c"] == (i, [p] * 5 + [i, i, i, p])
    assert _lib.SIGNATURES["cpc_encoder_backward_c"] == (i, [p] * 7 + [i, i, i, p])


def test_library_exports_the_symbols_and_checks_before_any_launch():
    lib = _library()
    assert lib.cpc_abi_version() == 16
    for name in NEW:
        assert hasattr(lib, name)
    sizes = (ctypes.c_long * 32)()
    B, L, C = 2, 1280, 40
    for norm in (BATCH, INSTANCE, ID):
        assert lib.cpc_encoder_layout_n(B, L, C, norm, 1, sizes) == 0
        assert [sizes[3 + i] for i in range(5)] == [256, 64, 32, 16, 8] and all(sizes[k] > 0 for k in range(3))
        assert sizes[26] == 64 and sizes[27] == (B if norm == INSTANCE else 1)
        assert lib.cpc_encoder_layout_n(B, L, 256, norm, 1, sizes) == 0 and sizes[26] == 256      # 256 runs the padded path
        for Cbad in (0, 1, 513):
            assert lib.cpc_encoder_layout_n(B, L, Cbad, norm, 1, sizes) == SHAPE
        assert lib.cpc_encoder_layout_n(B, L, C, norm, 1, None) == ARG
    for bad in (-1, 4, 17):
        assert lib.cpc_encoder_layout_n(B, L, C, bad, 1, sizes) == ARG
    # layerNorm is the _c entry: its 22 slots
    old = (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout_n(B, L, C, LAYER, 1, sizes) == 0 and lib.cpc_encoder_layout_c(B, L, C, old) == 0
    assert list(sizes)[:22] == list(old)
    # the minima of the torch modules: L = 170 gives L_4 = 1
    assert lib.cpc_encoder_layout_n(2, 170, C, INSTANCE, 1, sizes) == SHAPE
    assert lib.cpc_encoder_layout_n(2, 170, C, INSTANCE, 0, sizes) == SHAPE
    assert lib.cpc_encoder_layout_n(1, 170, C, BATCH, 1, sizes) == SHAPE
    assert lib.cpc_encoder_layout_n(1, 170, C, BATCH, 0, sizes) == 0           # eval mode reduces nothing
    assert lib.cpc_encoder_layout_n(2, 170, C, BATCH, 1, sizes) == 0           # B L_4 = 2
    assert lib.cpc_encoder_layout_n(1, 170, C, ID, 1, sizes) == 0
    assert lib.cpc_encoder_layout_n(65536, 1280, C, INSTANCE, 1, sizes) == SHAPE          # one grid row per utterance
    assert lib.cpc_encoder_layout_n(65535, 1280, C, INSTANCE, 1, sizes) == 0
    assert lib.cpc_encoder_layout_n(65536, 1280, C, BATCH, 1, sizes) == 0

    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    z = torch.full((B, 8, C), 7.0)
    buf = torch.full((1024,), 7.0)
    ptrs = (ctypes.c_void_p * 20)(*[P(buf)] * 20)
    run = (ctypes.c_void_p * 10)(*[P(buf)] * 10)
    holes = (ctypes.c_void_p * 10)(*([P(buf)] * 9 + [None]))
    fwd, bwd, act = lib.cpc_encoder_forward_n, lib.cpc_encoder_backward_n, lib.cpc_encoder_saved_activation_n
    for bad in (-1, 4):
        assert fwd(P(buf), ptrs, run, P(buf), P(buf), P(z), B, L, C, bad, 1, 0.1, 1e-5, None) == ARG
        assert bwd(P(buf), ptrs, P(buf), P(z), P(z), P(buf), ptrs, B, L, C, bad, 1, None) == ARG
        assert act(P(buf), 0, P(z), B, L, C, bad, None) == ARG
    assert fwd(P(buf), ptrs, None, P(buf), P(buf), P(z), B, L, C, BATCH, 1, 0.1, 1e-5, None) == ARG
    assert fwd(P(buf), ptrs, None, P(buf), P(buf), P(z), B, L, C, BATCH, 0, 0.1, 1e-5, None) == ARG
    assert fwd(P(buf), ptrs, holes, P(buf), P(buf), P(z), B, L, C, BATCH, 1, 0.1, 1e-5, None) == ARG
    assert fwd(P(buf), ptrs, run, P(buf), P(buf), P(z), 2, 170, C, INSTANCE, 1, 0.1, 1e-5, None) == SHAPE
    assert fwd(P(buf), ptrs, run, P(buf), P(buf), P(z), 1, 170, C, BATCH, 1, 0.1, 1e-5, None) == SHAPE
    assert bwd(P(buf), ptrs, P(buf), P(z), P(z), P(buf), ptrs, 2, 170, C, INSTANCE, 1, None) == SHAPE
    assert bwd(P(buf), ptrs, P(buf), P(z), P(z), P(buf), ptrs, 1, 170, C, BATCH, 1, None) == SHAPE
    for norm in (BATCH, INSTANCE, ID):
        for Cbad in (0, 1, 513):
            assert fwd(P(buf), ptrs, run, P(buf), P(buf), P(z), B, L, Cbad, norm, 1, 0.1, 1e-5, None) == SHAPE
            assert bwd(P(buf), ptrs, P(buf), P(z), P(z), P(buf), ptrs, B, L, Cbad, norm, 1, None) == SHAPE
            assert act(P(buf), 0, P(z), B, L, Cbad, norm, None) == SHAPE
        assert fwd(None, ptrs, run, P(buf), P(buf), P(z), B, L, C, norm, 1, 0.1, 1e-5, None) == ARG
        assert fwd(P(buf), None, run, P(buf), P(buf), P(z), B, L, C, norm, 1, 0.1, 1e-5, None) == ARG
        assert bwd(P(buf), ptrs, P(buf), P(z), None, P(buf), ptrs, B, L, C, norm, 1, None) == ARG
        assert bwd(P(buf), ptrs, P(buf), P(z), P(z), P(buf), None, B, L, C, norm, 1, None) == ARG
        assert act(P(buf), 4, P(z), B, L, C, norm, None) == ARG
    # a NULL norm slot is an error except under ID
    gaps = (ctypes.c_void_p * 20)(*[None if q % 4 >= 2 else P(buf) for q in range(20)])
    assert fwd(P(buf), gaps, run, P(buf), P(buf), P(z), B, L, C, INSTANCE, 1, 0.1, 1e-5, None) == ARG
    assert bwd(P(buf), ptrs, P(buf), P(z), P(z), P(buf), gaps, B, L, C, BATCH, 1, None) == ARG
    assert bool((z == 7.0).all()) and bool((buf == 7.0).all())             # nothing was launched
