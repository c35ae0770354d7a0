"""The MFCC encoder on an MI355X (csrc/mfcc.hip): the two kernels through the C ABI, ops.mfcc inside model.MFCCEncoder, the
encoder inside the train chain and inside harness.build_feature -- always against the float64 numpy oracle of
tests/mfcc_util.py on the CPU, never against the HIP path itself and never against the torch.stft path on the device (that
comparison is tools/bench_mfcc.py's business).  Tolerances: tests/mfcc_util.py; the chain's losses at the 1e-4 relative of
tests/test_gpu_lfb.py."""
import functools
import math

import pytest
import torch

import mfcc_util as U
from cpc_audio_amd import _lib, harness, model, ops, train
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("N,L,D", U.CASES_GPU)
def test_stages_match_float64(N, L, D):
    U.check_stages(_lib.get(), U.case(N, L, seed=N + L + D), D, device="cuda", stream=_stream())
    ops.check_device_errors()


@pytest.mark.parametrize("variant", U.VARIANTS)
def test_input_variants(variant):
    N, L, D = U.VARIANT_SHAPE
    db, (y, y_row) = U.check_stages(_lib.get(), U.case(N, L, seed=7, variant=variant), D, device="cuda", stream=_stream(),
                                    variant=variant)
    if variant == "silence":
        assert bool((db == -100.0).all())
        assert U.rel_err(y[:, :, 0], torch.full((N, U.frames(L)), -100.0 * math.sqrt(U.mels(D)))) < 1e-5
        assert float(y[:, :, 1:].abs().max()) <= 1e-3
    if variant == "quiet_row":
        assert not torch.equal(y[1], y_row[1]) and torch.equal(y[0], y_row[0])
    ops.check_device_errors()


@functools.lru_cache(maxsize=None)
def _reference(N, L, D):
    """(x, the oracle's y (N, F, D) in float64), once per shape."""
    x = U.case(N, L, seed=N + L + D)
    return x, U.oracle(x, D)["y"]


@pytest.mark.parametrize("N,L,D", [(2, 20480, 256), (3, 1040, 32), (1, 161, 13)])
def test_module_matches_the_oracle(N, L, D):
    x, want = _reference(N, L, D)
    enc = model.MFCCEncoder(D).cuda()
    assert enc.hip and ops.mfcc_supported(N, L, D)
    wave = x.cuda().unsqueeze(1)
    y = enc(wave)
    F = U.frames(L)
    assert tuple(y.shape) == (N, D, F) and y.permute(0, 2, 1).is_contiguous() and not y.requires_grad and y.grad_fn is None
    assert U.rel_err(y.permute(0, 2, 1), want) < U.BAR
    assert torch.equal(enc(wave.requires_grad_(True)), y)                    # the waveform receives no gradient
    ops.check_device_errors()


def test_only_the_result_stays_allocated():
    enc = model.MFCCEncoder(256).cuda()
    x = (0.1 * torch.randn(2, 1, 20480)).cuda()
    with torch.no_grad():
        enc(x)                                              # warm the allocator and the layout cache
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = enc(x)
        assert torch.cuda.memory_allocated() - before == y.numel() * 4          # db and the workspace are temporaries
    ops.check_device_errors()


def test_train_chain_with_the_mfcc_encoder():
    """build_model(mfcc) + the criterion at B = 2, L = 20480 with fixed negatives: the fused step declines, the chain runs
    module by module, the losses are those of the same gAR and criterion fed the oracle's z, and every parameter of the
    autoregressor and the criterion receives a finite gradient."""
    B, L = 2, 20480
    x, want_z = _reference(B, L, 256)
    torch.manual_seed(5)
    m = train.build_model(encoder_type="mfcc", mfccKernel=True, arMode="GRU", nLevelsGRU=2).cuda()
    crit = train.build_criterion().cuda()
    assert type(m.gEncoder) is model.MFCCEncoder and type(m.gAR) is model.CPCAR
    wave = x.cuda().unsqueeze(1)
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    g = torch.Generator().manual_seed(9)
    bi, si = O.draw_negative_indices(B, 128, 116, 128, generator=g)
    neg = (bi.cuda(), si.cuda())
    c, z, _ = m(wave, None)
    assert z.is_contiguous() and tuple(z.shape) == (B, 128, 256)
    assert U.rel_err(z, want_z) < U.BAR
    losses, _ = crit(c, z, None, negatives=neg)
    with torch.no_grad():
        z_ref = want_z.float().cuda().contiguous()
        want, _ = crit(m.gAR(z_ref), z_ref, None, negatives=neg)
    assert bool(((losses - want).abs() <= 1e-4 * want.abs()).all()), (losses, want)
    losses.sum().backward()
    params = list(m.gAR.parameters()) + list(crit.parameters())
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    ops.check_device_errors()


def test_build_feature_with_mfcc_and_no_ar():
    """150 000 samples in chunks of 64 000, 64 000 and 22 000, the second 80 dB below the first: the batched call floors each
    chunk by its own maximum, as chunk-by-chunk calls do."""
    D = 256
    m = train.build_model(encoder_type="mfcc", mfccKernel=True, arMode="no_ar", hiddenEncoder=D)
    g = torch.Generator().manual_seed(13)
    wave = (0.1 * torch.randn(1, 150000, generator=g)).clamp_(-1, 1)
    wave[:, 64000:128000] *= 1e-4
    got = harness.build_feature(harness.FeatureModule(m, False).cuda().eval(), wave)
    assert m.gEncoder.topPerRow is False
    assert tuple(got.shape) == (1, 938, D)
    assert U.rel_err(got, U.oracle_chunks(wave, D)) < U.BAR
    ops.check_device_errors()
