"""The fused probe step and the supervised criteria at any feature width (csrc/probe.hip: cpc_probe_*_d; csrc/supervised.hip:
cpc_classifier_*_d, cpc_ctc_forward_d) on the host SIMT emulator against torch in float64 on the CPU.  Cases, checks and bounds:
tests/probe_widths_util.py (loss within 1e-5 relative, gradients within 1e-5 relative norm, accuracy exact -- no case has a row
whose top-2 margin is under 1e-5 of its scale, which is asserted)."""
import pytest
import torch

import probe_widths_util as U
from emu_util import emu


@pytest.mark.parametrize("D,R,C", U.CASES)
def test_probe_matches_torch_float64_emulated(D, R, C):
    U.check_probe_case(emu(), U.Case(D, R, C, seed=1000 * D + R + C))


@pytest.mark.parametrize("name", sorted(U.LAYOUTS))
def test_probe_reads_x_in_place_emulated(name):
    """The speaker layout (cFeature[:, -1, :]: row pitch 3 D) on the scalar path (D = 13) and on the 16-byte path (D = 40, pitch
    120), and x one float past a 16-byte boundary (scalar loads of x, 16-byte loads of W): the float64 checks, and the bits of the
    same rows read from a dense, aligned copy."""
    lib = emu()
    D, R, C, ldx, off = U.LAYOUTS[name]
    case = U.Case(D, R, C, seed=7 + D + off, ldx=ldx, off=off)
    assert (case.on("cpu")[1] % 16 == 0) == (name == "speaker40")          # the only one of the three that may take 16-byte loads of x
    U.check_probe_case(lib, case)
    dense = U.Case(D, R, C, seed=7 + D + off)
    dense.base, dense.W, dense.b, dense.y, dense.moments = case.x.clone().reshape(-1), case.W, case.b, case.y, case.moments
    a, d = U.train(lib, case), U.train(lib, dense)
    for k in U.BITS:
        assert torch.equal(a[k], d[k]), k


def test_d256_gives_the_bits_of_the_256_entry_points_emulated():
    U.check_d256_gives_the_bits_of_the_256_entry_points(emu())


def test_zero_columns_change_no_bit_emulated():
    """Padding invariance: D = 13 against D = 16 on the same x and W with three zero columns appended -- the same loss, accuracy,
    db and dW[:, :13], bit for bit, and dW[:, 13:] == 0."""
    lib = emu()
    R, C = 33, 41
    a = U.Case(13, R, C, seed=5)
    b = U.Case(16, R, C, seed=6)
    x16, W16 = torch.zeros(R, 16), torch.zeros(C, 16)
    x16[:, :13], W16[:, :13] = a.x, a.W
    b.base, b.W, b.b, b.y = x16.reshape(-1), W16, a.b, a.y
    oa, ob = U.train(lib, a), U.train(lib, b)
    for k in ("loss", "acc", "db"):
        assert torch.equal(oa[k], ob[k]), k
    dWa, dWb = oa["dW"][:C * 13].view(C, 13), ob["dW"][:C * 16].view(C, 16)
    assert torch.equal(dWa, dWb[:, :13]) and bool((dWb[:, 13:] == 0).all())
    ea, eb = U.evaluate(lib, a), U.evaluate(lib, b)
    assert torch.equal(ea["loss"], eb["loss"]) and torch.equal(ea["acc"], eb["acc"])


@pytest.mark.parametrize("D", [13, 40, 512])
def test_classifier_matches_torch_float64_emulated(D):
    U.check_classifier_case(emu(), D)


@pytest.mark.parametrize("D", [13, 40, 512])
def test_ctc_matches_torch_float64_emulated(D):
    U.check_ctc_case(emu(), D)


@pytest.mark.parametrize("C", [41, 70])
def test_label_out_of_range_flags_and_gives_nan_emulated(C):
    lib = emu()
    lib.cpc_device_error_flags(1)
    case = U.Case(40, 40, C, seed=9)
    case.y[7] = C
    out = U.train(lib, case)
    assert torch.isnan(out["loss"][0]) and torch.isnan(out["accum"][0])
    assert lib.cpc_device_error_flags(1) == U.LABEL_RANGE
    U.check_canaries(out, C, 40)
    case.y[7] = -1
    assert torch.isnan(U.evaluate(lib, case)["loss"][0])
    assert lib.cpc_device_error_flags(1) == U.LABEL_RANGE
    assert torch.isnan(U.classifier(lib, case)["loss"][0])
    assert lib.cpc_device_error_flags(1) == U.LABEL_RANGE
    assert lib.cpc_device_error_flags(1) == 0
