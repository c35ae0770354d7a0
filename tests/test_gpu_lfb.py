"""The learned-filter-bank encoder on an MI355X (csrc/lfb.hip): the kernels through the C ABI, ops.LfbFunction inside
model.LFBEnconder, the reference's fixture, the encoder inside the train chain and inside harness.build_feature -- always
against torch in float64 on the CPU (tests/lfb_util.py's formula or the module's own torch path) or the reference's stored
results, never against the HIP path itself.

Tolerances are the project's own (tests/test_emu_lfb.py, tests/test_gpu_phone_front.py): forward 1e-5 and gradients 1e-4 as
norm-relative error; the whole chain is compared at L >= 419 only (at two frames the instance norm divides two nearly equal
numbers by their tiny variance and torch's own fp32 reaches the bars), the two-frame shapes stage by stage."""
import functools

import pytest
import torch

import lfb_util as U
from cpc_audio_amd import _lib, harness, model, ops, train
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("N,L,D", [(n, l, 32) for n, l in U.ENERGY_CASES_D32]
                         + [(1, 579, 256), (2, 20480, 256), (1, 64000, 256), (3, 20333, 256)])
def test_energy_matches_float64(N, L, D):
    U.check_energy(_lib.get(), U.energy_case(N, L, D, seed=N + L), device="cuda", stream=_stream())
    ops.check_device_errors()


@pytest.mark.parametrize("variant", U.INPUT_VARIANTS)
def test_energy_input_variants(variant):
    U.check_energy(_lib.get(), U.energy_case(2, 2000, 32, seed=7, variant=variant), device="cuda", stream=_stream(), report=variant)
    ops.check_device_errors()


@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset30"])
@pytest.mark.parametrize("normalise", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("N,F,D", U.LOGNORM_CASES)
def test_lognorm_matches_float64(N, F, D, normalise, offset):
    U.check_lognorm(_lib.get(), N, F, D, normalise, offset, device="cuda", stream=_stream())
    ops.check_device_errors()


def _seeded_encoder(D, normalize=True, seed=31):
    torch.manual_seed(seed)
    return model.LFBEnconder(D, normalize=normalize)


@functools.lru_cache(maxsize=None)
def _float64_reference(N, L, D, normalize=True):
    """The module's own torch path in float64 on the CPU, once per shape: (module, x, y with its graph)."""
    enc = _seeded_encoder(D, normalize)
    g = torch.Generator().manual_seed(N + L + D)
    x = (0.1 * torch.randn(N, 1, L, generator=g)).clamp_(-1, 1)
    ref = _seeded_encoder(D, normalize).double()
    ref.hip = False
    return enc, x, ref, ref(x.double())


def _float64_grads(ref, y64, dy):
    return torch.autograd.grad(y64, [ref.conv.weight, ref.conv.bias], dy.double().cpu(), retain_graph=True)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("N,L,D", [(2, 20480, 256), (3, 1040, 32), (3, 419, 32)])
def test_module_matches_its_float64_torch_path(N, L, D, normalize):
    enc, x, ref, y64 = _float64_reference(N, L, D, normalize)
    enc = enc.cuda()
    assert enc.hip and ops.lfb_supported(N, L, D)
    y = enc(x.cuda())
    F = U.frames(L)
    assert tuple(y.shape) == (N, D, F) and y.permute(0, 2, 1).is_contiguous() and y.grad_fn is not None
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(N, D, F, generator=g)
    (y * dy.cuda()).sum().backward()
    gW, gb = _float64_grads(ref, y64, dy)
    errs = U.rel_err(y.detach(), y64.detach()), U.rel_err(enc.conv.weight.grad, gW), U.rel_err(enc.conv.bias.grad, gb)
    print(f"N={N} L={L} D={D} normalize={normalize}: y {errs[0]:.3g} dW {errs[1]:.3g} db {errs[2]:.3g}")
    assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4
    assert enc.conv.weight.grad.shape == enc.conv.weight.shape
    ops.check_device_errors()


def test_nothing_is_saved_without_grad():
    enc = _seeded_encoder(256).cuda()
    x = (0.1 * torch.randn(2, 1, 20480)).cuda()
    with torch.no_grad():
        enc(x)                                              # warm the allocator and the layout cache
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = enc(x)
        assert y.grad_fn is None and not y.requires_grad
        assert torch.cuda.memory_allocated() - before == y.numel() * 4          # the result alone: no s, no statistics
    for p in enc.parameters():
        p.requires_grad_(False)
    before = torch.cuda.memory_allocated()
    z = enc(x)
    assert not z.requires_grad and torch.cuda.memory_allocated() - before == z.numel() * 4
    assert torch.equal(y, z)
    slow = model.LFBEnconder(256, hip=False).cuda()
    slow.load_state_dict(enc.state_dict())
    with torch.no_grad():
        assert U.rel_err(slow(x), y.double().cpu()) < 1e-4                      # hip=False is the torch path on the same device


@pytest.mark.parametrize("tag", ["small", "wide"])
def test_hip_path_reproduces_the_reference(tag):
    arrays, meta = U.golden()
    enc = model.LFBEnconder(meta["cases"][tag]["D"])
    enc.load_state_dict(U.golden_state(arrays, meta, tag), strict=True)
    U.check_against_golden(enc.cuda(), arrays, meta, tag, "cuda", y_tol=None, grad_tol=1e-4)


@pytest.mark.parametrize("arMode", ["GRU", "no_ar"])
def test_train_chain_with_the_lfb_encoder(arMode):
    """build_model(lfb) + the criterion at B = 2, L = 20480 with fixed negatives: the fused step declines, forward and backward
    run module by module, the loss is that of the same gAR and criterion fed the float64 z, and conv.weight.grad is the
    float64 backward of the encoder fed the dz the GPU chain produced."""
    B, L = 2, 20480
    enc0, x, ref, y64 = _float64_reference(B, L, 256)
    torch.manual_seed(5)
    m = train.build_model(encoder_type="lfb", arMode=arMode, nLevelsGRU=2)
    m.gEncoder.load_state_dict(enc0.state_dict())
    m = m.cuda()
    crit = train.build_criterion().cuda()
    assert type(m.gEncoder) is model.LFBEnconder and type(m.gAR) is (model.NoAr if arMode == "no_ar" else model.CPCAR)
    wave = x.cuda()
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    g = torch.Generator().manual_seed(9)
    bi, si = O.draw_negative_indices(B, 128, 116, 128, generator=g)
    neg = (bi.cuda(), si.cuda())
    c, z, _ = m(wave, None)
    assert z.is_contiguous() and tuple(z.shape) == (B, 128, 256)
    dz = []
    z.register_hook(dz.append)
    losses, _ = crit(c, z, None, negatives=neg)
    with torch.no_grad():
        z_ref = y64.detach().float().cuda().permute(0, 2, 1).contiguous()
        want, _ = crit(m.gAR(z_ref), z_ref, None, negatives=neg)
    assert U.rel_err(z.detach(), y64.detach().permute(0, 2, 1)) < 1e-5
    assert bool(((losses - want).abs() <= 1e-4 * want.abs()).all()), (losses, want)
    if arMode == "GRU":
        losses.sum().backward()
        assert len(dz) == 1 and bool(torch.isfinite(m.gEncoder.conv.weight.grad).all())
        gW, gb = _float64_grads(ref, y64, dz[0].permute(0, 2, 1))
        assert U.rel_err(m.gEncoder.conv.weight.grad, gW) < 1e-4 and U.rel_err(m.gEncoder.conv.bias.grad, gb) < 1e-4
        assert all(p.grad is not None for p in m.gAR.parameters())
    ops.check_device_errors()


def test_build_feature_with_lfb_and_no_ar():
    """150 000 samples in chunks of 64 000: two whole chunks and a rest of 22 000 (no chunk is shorter than the 400 taps):
    400 + 400 + 137 frames."""
    torch.manual_seed(13)
    m = train.build_model(encoder_type="lfb", arMode="no_ar")
    wave = (0.1 * torch.randn(1, 150000)).clamp_(-1, 1)
    assert [e - f for f, e, _ in harness.chunk_plan(150000, 64000, False, 160)] == [64000, 64000, 22000]
    ref = train.build_model(encoder_type="lfb", arMode="no_ar").double()
    ref.load_state_dict(m.state_dict())
    ref.gEncoder.hip = False
    want = harness.build_feature(harness.FeatureModule(ref, False).eval(), wave.double())
    got = harness.build_feature(harness.FeatureModule(m, False).cuda().eval(), wave)
    assert tuple(got.shape) == (1, 937, 256) == tuple(want.shape)
    assert U.rel_err(got, want) < 1e-5
    ops.check_device_errors()
