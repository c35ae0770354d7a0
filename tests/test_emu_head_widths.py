"""The PER phone classifier's kernels and the phone posteriors at any feature width (cpc_phone_head_*_d, cpc_seqnorm_*_d,
cpc_posterior_forward_d) on the host SIMT emulator, against torch in float64 on the CPU.  The cases, oracles and bounds are
those of tests/head_widths_util.py, which tests/test_gpu_head_widths.py runs on the GPU."""
import itertools

import pytest
import torch

import head_widths_util as U
from emu_util import emu

DEV = torch.device("cpu")


@pytest.mark.parametrize("D,B,S,C", U.HEAD_CASES)
def test_head_matches_conv1d_float64_emulated(D, B, S, C):
    U.check_head(emu(), DEV, D, B, S, C)


@pytest.mark.parametrize("B,S,C", [(2, 11, 7), (2, 37, 41), (1, 77, 65)])
def test_head_d_at_256_is_the_256_head_emulated(B, S, C):
    U.check_head_at_256(emu(), DEV, B, S, C)


@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_head_and_ctc_with_ragged_lengths_emulated(reduction):
    case = U.ragged_ctc_case()
    U.check_ctc_results(U.run_head_ctc(emu(), DEV, *case, reduction), *case, reduction)


@pytest.mark.parametrize("D,shape", list(itertools.product(U.WIDTHS, U.SEQNORM_SHAPES)))
def test_seqnorm_matches_float64_emulated(D, shape):
    lib = emu()
    for with_scale, normalise, scalar in [(True, True, False), (False, True, True), (True, False, False), (True, False, True)]:
        U.check_seqnorm(lib, DEV, D, *shape, with_scale, normalise, scalar)


@pytest.mark.parametrize("D", U.WIDTHS)
@pytest.mark.parametrize("scalar", [False, True])
def test_seqnorm_columns_have_the_bits_of_a_256_wide_call_emulated(D, scalar):
    for shape in ((3, 33), (2, 70)):
        U.check_seqnorm_columns(emu(), DEV, D, *shape, scalar)


@pytest.mark.parametrize("scalar", [False, True])
def test_seqnorm_d_at_256_is_the_256_seqnorm_emulated(scalar):
    for shape in U.SEQNORM_SHAPES:
        U.check_seqnorm_at_256(emu(), DEV, *shape, scalar)


@pytest.mark.parametrize("D", [13, 257, 260])
def test_seqnorm_short_and_overlong_lengths_emulated(D):
    U.check_seqnorm_lengths(emu(), DEV, D)


@pytest.mark.parametrize("D,shape", list(itertools.product(U.WIDTHS, U.POSTERIOR_SHAPES)))
def test_posteriors_and_one_hot_match_torch_float64_emulated(D, shape):
    U.check_posterior(emu(), DEV, D, *shape)


@pytest.mark.parametrize("R,C", [(33, 42), (70, 65), (5, 385)])
def test_posterior_at_13_is_16_with_zero_columns_emulated(R, C):
    U.check_posterior_zero_columns(emu(), DEV, R, C)


@pytest.mark.parametrize("R,C", [(33, 42), (70, 65), (40, 400)])
def test_posterior_d_at_256_is_the_256_posterior_emulated(R, C):
    U.check_posterior_at_256(emu(), DEV, R, C)
