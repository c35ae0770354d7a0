"""The learned-filter-bank kernels (csrc/lfb.hip) on the host SIMT emulator against torch in float64 on the CPU: the fused
conv + squared modulus + Hann pooling (cpc_lfb_energy_forward), its weight and bias gradient (cpc_lfb_energy_backward) and the
log / instance norm (cpc_lfb_lognorm_forward / _backward).  Every output and workspace buffer carries 64 canary floats that
must stay untouched, the inputs keep their bits, and two calls give the same bits (tests/lfb_util.py).

Tolerances are the project's own (tests/test_emu_seqnorm.py, tests/test_gpu_phone_front.py): forward 1e-5, gradients 1e-4 as
norm-relative error.  torch's own fp32 stays below 5e-7 / 2.7e-6 on the energy cases, so the bars separate exact-fp32
arithmetic from anything coarser with a factor of 4 to spare at the least.  The kernels' tiles are 32 conv positions, a hop of
160 and a workgroup of 4 hops: L = 400 is a single position, 1040 and 2000 cross several hops and end in a ragged tile."""
import pytest
import torch

import lfb_util as U
from emu_util import emu


@pytest.mark.parametrize("N,L", U.ENERGY_CASES_D32)
def test_energy_matches_float64_emulated(N, L):
    lib = emu()
    U.check_energy(lib, U.energy_case(N, L, 32, seed=N + L))
    assert lib.cpc_device_error_flags(1) == 0


def test_energy_over_several_channel_blocks_emulated():
    lib = emu()
    U.check_energy(lib, U.energy_case(1, 579, 256, seed=5))
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("variant", U.INPUT_VARIANTS)
def test_energy_input_variants_emulated(variant):
    """Amplitudes 1e-3 and 30, a DC offset of 0.5 and weights times 100: exact-f32 products need no scale, so none may matter."""
    lib = emu()
    U.check_energy(lib, U.energy_case(2, 2000, 32, seed=7, variant=variant), report=variant)
    assert lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset30"])
@pytest.mark.parametrize("normalise", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("N,F,D", U.LOGNORM_CASES)
def test_lognorm_matches_float64_emulated(N, F, D, normalise, offset):
    lib = emu()
    U.check_lognorm(lib, N, F, D, normalise, offset)
    assert lib.cpc_device_error_flags(1) == 0


def test_silence_gives_finite_results_emulated():
    """x = 0: every conv output is its bias, every frame of a filter has the same energy up to the window's overhang, and the
    norm divides by sqrt(var + 1e-5), never by zero.  With zero bias as well the energies are exactly 0 and so is the output."""
    lib = emu()
    x, W, b, han, gs = U.energy_case(2, 1040, 32, seed=9)
    for bias in (b, torch.zeros_like(b)):
        x0 = torch.zeros_like(x)
        s = U.run_energy_forward(lib, x0, W, bias, han)
        n = 2 * 6 * 32
        assert bool(torch.isfinite(s[:n]).all())
        y, stats = U.run_lognorm_forward(lib, s[:n].view(2, 6, 32).contiguous())
        ds = U.run_lognorm_backward(lib, s[:n].view(2, 6, 32).contiguous(), stats, gs)
        dW, db = U.run_energy_backward(lib, x0, W, bias, han, ds[:n].view(2, 6, 32).contiguous())
        assert all(bool(torch.isfinite(t).all()) for t in (y, stats, ds, dW, db))
        assert bool((dW[:64 * 400] == 0).all())                      # dW = sum gy x
    assert bool((s[:n] == 0).all()) and bool((y[:n] == 0).all())
    assert lib.cpc_device_error_flags(1) == 0


def test_arguments_are_checked_before_any_launch_emulated():
    lib = emu()
    buf = torch.full((64,), 7.0)
    P = U.P
    for N, L, D in [(1, 400, 48), (1, 400, 544), (1, 399, 32), (0, 400, 32)]:
        assert lib.cpc_lfb_energy_forward(P(buf), P(buf), P(buf), P(buf), P(buf), None, N, L, D, None) == 1
        assert lib.cpc_lfb_energy_backward(P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), N, L, D, None) == 1
    assert lib.cpc_lfb_energy_forward(None, P(buf), P(buf), P(buf), P(buf), None, 1, 400, 32, None) == 2
    assert lib.cpc_lfb_energy_backward(P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), None, 1, 400, 32, None) == 2
    assert lib.cpc_lfb_lognorm_forward(P(buf), P(buf), None, 1, 2, 32, 1, None) == 2                 # in place
    assert lib.cpc_lfb_lognorm_backward(P(buf), None, P(buf), P(buf), 1, 2, 32, 1, None) == 2
    assert bool((buf == 7.0).all())
