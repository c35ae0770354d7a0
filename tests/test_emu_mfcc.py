"""The MFCC kernels (csrc/mfcc.hip) on the host SIMT emulator against the float64 numpy oracle of tests/mfcc_util.py: the fused
frames + windowed DFT + power + mel product + decibels (cpc_mfcc_meldb) and the clamp + DCT (cpc_mfcc_dct) for both scopes of the
maximum.  Every output and workspace buffer carries 64 canary floats that must stay untouched, the inputs keep their bits, and
two calls give the same bits.  Shapes, variants and tolerances: tests/mfcc_util.py (a workgroup owns 32 frames: L = 161 is two
frames made mostly of reflected samples, 320 / 321 step the frame count, 2000 is 13 frames in a ragged tile, D = 13 and 40 are
ragged column tiles, D = 256 has 58 empty filters)."""
import math

import pytest
import torch

import mfcc_util as U
from emu_util import emu


@pytest.mark.parametrize("N,L,D", U.CASES_CPU)
def test_stages_match_float64_emulated(N, L, D):
    lib = emu()
    U.check_stages(lib, U.case(N, L, seed=N + L + D), D)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("variant", U.VARIANTS)
def test_input_variants_emulated(variant):
    lib = emu()
    N, L, D = U.VARIANT_SHAPE
    db, (y, y_row) = U.check_stages(lib, U.case(N, L, seed=7, variant=variant), D, variant=variant)
    if variant == "silence":                                    # every filter gives exactly -100 dB
        assert bool((db == -100.0).all())
        assert U.rel_err(y[:, :, 0], torch.full((N, U.frames(L)), -100.0 * math.sqrt(U.mels(D)))) < 1e-5
        assert float(y[:, :, 1:].abs().max()) <= 1e-3
    if variant == "quiet_row":                                  # the floor of the whole call bites row 1, its own does not
        assert not torch.equal(y[1], y_row[1]) and torch.equal(y[0], y_row[0])
    assert lib.cpc_device_error_flags(1) == 0


def test_more_than_one_frame_tile_per_row_emulated():
    """5000 samples: 32 frames, exactly one tile; 5121: 33 frames, a second tile of one frame."""
    lib = emu()
    for L in (5000, 5121):
        U.check_stages(lib, U.case(2, L, seed=L), 13)
    assert lib.cpc_device_error_flags(1) == 0


def test_empty_filters_give_the_floor_emulated():
    lib = emu()
    db, _ = U.check_stages(lib, U.case(1, 1040, seed=3), 256)
    assert int((db == -100.0).all(dim=1).sum()) == U.EMPTY_FILTERS[256]


def test_arguments_are_checked_before_any_launch_emulated():
    lib = emu()
    buf = torch.full((64,), 7.0)
    P = U.P
    for N, L, D in [(1, 160, 40), (1, 161, 0), (1, 161, 513), (0, 161, 40), (1 << 20, 64000, 40)]:
        assert lib.cpc_mfcc_meldb(P(buf), P(buf), P(buf), P(buf), P(buf), N, L, D, None) == 1
    for N, F, D in [(1, 1, 40), (1, 2, 0), (1, 2, 513), (0, 2, 40), (1 << 16, 1 << 8, 40)]:
        assert lib.cpc_mfcc_dct(P(buf), P(buf), P(buf), P(torch.empty(1)), N, F, D, 0, None) == 1
    assert lib.cpc_mfcc_meldb(None, P(buf), P(buf), P(buf), P(buf), 1, 161, 40, None) == 2
    assert lib.cpc_mfcc_meldb(P(buf), P(buf), P(buf), P(buf), None, 1, 161, 40, None) == 2
    assert lib.cpc_mfcc_dct(P(buf), P(buf), P(buf), None, 1, 2, 40, 0, None) == 2
    assert lib.cpc_mfcc_dct(P(buf), P(buf), P(buf), P(torch.empty(1)), 1, 2, 40, 2, None) == 2
    assert bool((buf == 7.0).all())
