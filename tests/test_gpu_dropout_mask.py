"""The transformer layer's dropout masks on a real MI355X against the independent Philox reference (tests/philox_util.py): the
masks cpc_dropout_keep_mask reports, and the masks every kernel that regenerates them APPLIES -- the layer through the C ABI under
each switch that selects another such kernel, the module path and the group path -- with the oracle fed the reference's masks.

Bounds: 1e-4 absolute on y, 1e-4 relative on dx and on every parameter gradient (those of
tests/test_gpu_transformer.py::test_transformer_layer_trains_with_the_references_dropout).

Input seeds.  A hidden unit whose pre-activation lies within fp32 rounding of zero may fall on the other side of the ReLU on the
device than in the oracle; at these small shapes ONE such unit moves lin1's gradients by ~1 / sqrt(active units) >> 1e-4 (the
ReLU-tie effect described in tests/test_gpu_transformer.py::test_config4_at_its_quoted_batch_...).  The input seed of each case
below was therefore chosen, on the CPU and before any device run, among 0 .. 15 (0 .. 95 for the two largest shapes) as the one whose
float64 oracle keeps its kept hidden units farthest from zero: 2.1e-3, 5.5e-5, 5.0e-5, 9.5e-6 and 9.0e-6 for the five shapes, 2.2e-5
for the group, 1.0e-4 for the module path (dropout_util.oracle_with_reference_masks reports that distance; it is printed with every
case)."""
import functools

import pytest
import torch

import philox_util as PU
from dropout_util import MASK64, assert_layer_matches, group_call, layer_call, library_masks, oracle_with_reference_masks
from oracle import transformer_oracle as T

pytestmark = pytest.mark.gpu

TOL = 1e-4
SEEDS = [0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1]
PS = [0.0, 0.1, 0.2, 0.3, 0.5]
DROP_SEED = 0xC0FFEE123456789A                        # both key words in use
DROP_SEED_S1 = DROP_SEED + 1                          # for (1, 1): DROP_SEED keeps all eight probabilities, this one drops head 1's
GROUP_SEED = 0xFEDCBA9876543210

# (B, S, abspos, p) -> input seed (see the module docstring)
#   (1, 1): one probability per head;  (1, 37): S no multiple of 4 -- a ragged last Philox row block at site 0, and the last row
#   block of the hidden layer holds one row;  (3, 99): M = 297 = one full 256-row tile + a ragged one
CASES = {(1, 1, False, 0.1): 1, (1, 37, False, 0.2): 3, (2, 33, True, 0.3): 9, (3, 99, False, 0.1): 18, (3, 128, False, 0.1): 33}
GROUP_CASE = (1, 37, 3, 0.1)
GROUP_INPUT_SEED = 2
MODULE_INPUT_SEED = 6
MODULE_TORCH_SEED = 321

# the library's defaults, and the settings that select the other kernels which regenerate or apply the mask
DEFAULTS = {"cpc_set_gemm_dma": 1, "cpc_set_gemm_fuse": 1, "cpc_set_attn_fwd": 1, "cpc_set_gemm_split": 1}
SWITCHES = {
    "default": {},
    "dma-fed-epilogue": {"cpc_set_gemm_dma": 2},      # ReLU + dropout + mask bits in lin1's DMA-fed epilogue (gemm_dma.hip)
    "generic-tiles": {"cpc_set_gemm_dma": 0},         # the generic GEMMs with relu_kernel / the ReLU-derivative kernels behind them
    "no-fused-epilogue": {"cpc_set_gemm_fuse": 0},    # the separate ReLU / dropout and ReLU-derivative kernels whatever the size
    "attn-fwd-one-tile": {"cpc_set_attn_fwd": 0},     # the 133 KB attention forward
    # beyond the four switches above: the wide generic tile however small the grid, whose backward epilogue applies the ReLU
    # derivative and the dropout scale from the saved hidden layer (gemm.hip) -- at these sizes the default never takes it
    "wide-tile-epilogue": {"cpc_set_gemm_split": 3},
}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lib():
    from cpc_audio_amd import _lib
    return _lib.get()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _restore(lib):
    for name, value in DEFAULTS.items():
        getattr(lib, name)(value)


def _drop_seed(S):
    return DROP_SEED_S1 if S == 1 else DROP_SEED


def case_inputs(B, S, abspos, input_seed):
    prm = T.make_layer_params(seed=50 + S, size_seq=S, abspos=abspos)
    g = torch.Generator().manual_seed(input_seed)
    return prm, torch.randn(B, S, 256, generator=g), torch.randn(B, S, 256, generator=g)


@functools.lru_cache(maxsize=None)
def _case_reference(B, S, abspos, p):
    """Inputs and the oracle's answer under the reference's masks: computed once per shape, shared by every switch setting."""
    prm, x, dy = case_inputs(B, S, abspos, CASES[(B, S, abspos, p)])
    return prm, x, dy, oracle_with_reference_masks(prm, x, dy, p, _drop_seed(S))


def group_inputs(input_seed):
    B, S, G, _ = GROUP_CASE
    prms = [T.make_layer_params(seed=70 + q, size_seq=S, abspos=False) for q in range(G)]
    g = torch.Generator().manual_seed(input_seed)
    return prms, torch.randn(B, S, 256, generator=g), torch.randn(B * S, G * 256, generator=g)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_reported_mask_equals_the_reference(seed):
    """cpc_dropout_keep_mask == the reference, every bit: mulhi32, the 64-bit counter and key split, the double-precision
    threshold and the element numbering as the hardware computes them."""
    from cpc_audio_amd import ops
    dev, lib = _dev(), _lib()
    try:
        for BH, S in [(8, 1), (8, 37), (24, 128)]:
            bits = PU.attn_bits(BH, S, seed)
            for p in PS:
                got, _ = library_masks(lib, BH, S, 0, p, seed, dev, _stream())
                assert torch.equal(got, PU.attn_keep_ref(BH, S, p, seed, bits)), ("site 0", BH, S, p)
        for rows in [1, 37, 297, 384]:
            bits = PU.ffn_bits(rows, seed)
            for p in PS:
                _, got = library_masks(lib, 0, 1, rows, p, seed, dev, _stream())
                assert torch.equal(got, PU.ffn_keep_ref(rows, p, seed, bits)), ("site 1", rows, p)
    finally:
        _restore(lib)
    ops.check_device_errors()


_APPLIED = [(c, "default") for c in CASES] + [(c, s) for c in CASES if c[:2] in ((1, 37), (3, 99)) for s in SWITCHES if s != "default"]


@pytest.mark.parametrize("case,switch", _APPLIED, ids=lambda v: v if isinstance(v, str) else "B{}-S{}-{}-p{}".format(
    v[0], v[1], "abspos" if v[2] else "relpos", v[3]))
def test_applied_mask_through_the_c_abi(case, switch):
    """cpc_transformer_layer_forward_dropout / _backward_dropout against oracle.transformer_oracle.layer_forward fed the
    reference's masks: the forward kernels and the backward kernels (which regenerate the masks) apply the specification's mask."""
    from cpc_audio_amd import ops
    dev, lib = _dev(), _lib()
    B, S, abspos, p = case
    prm, x, dy, ref = _case_reference(B, S, abspos, p)
    try:
        for name, value in SWITCHES[switch].items():
            assert getattr(lib, name)(value) == 0
        got = layer_call(lib, prm, x.to(dev), dy.to(dev), p, _drop_seed(S), _stream())
    finally:
        _restore(lib)
    assert_layer_matches(got, ref, TOL, f"{case} {switch}")
    ops.check_device_errors()


def test_module_path_draws_its_seed_from_the_cpu_generator_and_applies_the_reference_masks():
    from cpc_audio_amd import ops
    from cpc_audio_amd.transformers import buildTransformerAR
    dev, lib = _dev(), _lib()
    B, S, p = 1, 37, 0.1
    prm, x, dy = case_inputs(B, S, False, MODULE_INPUT_SEED)
    try:
        net = buildTransformerAR(256, 1, S, False).to(dev)          # default dropout: 0.1, as the reference
        net.load_state_dict({"0." + k: v for k, v in prm.items()}, strict=False)
        net.train()
        torch.manual_seed(MODULE_TORCH_SEED)
        seed = int(torch.empty((), dtype=torch.int64).random_().item()) & MASK64     # the next int64 of the CPU generator
        torch.manual_seed(MODULE_TORCH_SEED)
        xd = x.to(dev).requires_grad_(True)
        y1 = net(xd)
        (y1 * dy.to(dev)).sum().backward()
        grads = {k[2:]: v.grad.cpu() for k, v in net.named_parameters()}
        dx = xd.grad.cpu()
        with torch.no_grad():
            y2 = net(x.to(dev))                                      # the generator moved on: other masks
            torch.manual_seed(MODULE_TORCH_SEED)
            y3 = net(x.to(dev))
        torch.cuda.synchronize()
        assert not torch.equal(y1, y2)
        assert torch.equal(y1, y3)                                   # the same manual_seed reproduces the call bit for bit
        ref = oracle_with_reference_masks(prm, x, dy, p, seed)
        assert_layer_matches((y1.detach().cpu(), dx, grads), ref, TOL, f"module path, seed {seed:#x}")
        # eval(): no dropout, no draw from the generator, equal to the p = 0 oracle
        net.eval()
        state = torch.get_rng_state()
        with torch.no_grad():
            e = net(x.to(dev))
        torch.cuda.synchronize()
        assert torch.equal(torch.get_rng_state(), state)
        dev_e = (e.cpu() - T.layer_forward(prm, x)).abs().max().item()
        print(f"module path, eval: max|dy| {dev_e:.2e}")
        assert dev_e < TOL
    finally:
        _restore(lib)
    ops.check_device_errors()


@pytest.mark.parametrize("dma", [1, 2], ids=["default", "dma-fed-epilogue"])
def test_group_path_applies_the_reference_masks_of_seed_plus_layer(dma):
    """cpc_transformer_group_forward / _backward, G = 3: layer g against the oracle under the reference's masks of
    (seed + g) mod 2^64.  dx of the group is the sum of the layers' input gradients."""
    from cpc_audio_amd import ops
    dev, lib = _dev(), _lib()
    B, S, G, p = GROUP_CASE
    prms, x, dy = group_inputs(GROUP_INPUT_SEED)
    try:
        assert lib.cpc_set_gemm_dma(dma) == 0
        out, dx, sgrads = group_call(lib, prms, x.to(dev), dy.to(dev), p, GROUP_SEED, _stream())
    finally:
        _restore(lib)
    dx_sum = torch.zeros(B, S, 256)
    for q in range(G):
        ref = oracle_with_reference_masks(prms[q], x, dy[:, q * 256:(q + 1) * 256].reshape(B, S, 256), p, (GROUP_SEED + q) & MASK64)
        dx_sum += ref[1]
        got = (out[:, q * 256:(q + 1) * 256].reshape(B, S, 256), None, {k: v[q] for k, v in sgrads.items()})
        assert_layer_matches(got, ref, TOL, f"group layer {q}, gemm_dma {dma}")
    dev_dx = ((dx - dx_sum).norm() / dx_sum.norm()).item()
    print(f"group, gemm_dma {dma}: rel dx {dev_dx:.2e}")
    assert dev_dx < TOL
    ops.check_device_errors()
