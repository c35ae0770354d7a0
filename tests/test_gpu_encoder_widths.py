"""The encoder at any hidden width on an MI355X (csrc/enc_wide.hip: cpc_encoder_*_c; ops.EncoderWideFunction; model.CPCEncoder with
encoderKernel=True) against O.encoder_forward in float64 on the CPU (oneDNN off, tests/test_emu_encoder.py says why).
Bar: max |delta| < 1e-4 on y0..y3 and z, norm-wise relative error < 1e-4 on every one of the 20 gradients."""
import copy
import ctypes

import pytest
import torch

from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

BAR = 1e-4
NAMES = [f"gEncoder.{n}{i}.{w}" for i in range(5)
         for n, w in (("conv", "weight"), ("conv", "bias"), ("batchNorm", "weight"), ("batchNorm", "bias"))]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def P(t):
    return None if t is None else t.data_ptr()


def _device_run(C, B, L, dev, seed=0, repeat=1):
    """cpc_encoder_forward_c / _backward_c on NaN-prefilled buffers -> parameters, wave, dz (CPU), then `repeat` results
    (z, [y0..y3], [20 gradients]) on the CPU."""
    from cpc_audio_amd import _lib
    lib = _lib.get()
    p = O.make_params(seed=seed, hidden_encoder=C)
    plist = [p[n].contiguous().to(dev) for n in NAMES]
    wave = O.make_waveform(B, L, seed=5)
    wd = wave.to(dev)
    sizes = (ctypes.c_long * 22)()
    assert lib.cpc_encoder_layout_c(B, L, C, sizes) == 0
    Ls = [sizes[3 + i] for i in range(5)]
    dz = torch.randn(B, Ls[4], C, generator=torch.Generator().manual_seed(11))
    dzd = dz.to(dev)
    parr = (ctypes.c_void_p * 20)(*[P(t) for t in plist])
    stream = torch.cuda.current_stream().cuda_stream
    nan = float("nan")
    out = []
    for _ in range(repeat):
        saved = torch.full((sizes[0],), nan, device=dev)
        fscr = torch.full((max(1, sizes[1]),), nan, device=dev)
        z = torch.full((B, Ls[4], C), nan, device=dev)
        assert lib.cpc_encoder_forward_c(P(wd), parr, P(saved), P(fscr), P(z), B, L, C, stream) == 0
        ys = []
        for i in range(4):
            y = torch.full((B, Ls[i], C), nan, device=dev)
            assert lib.cpc_encoder_saved_activation_c(P(saved), i, P(y), B, L, C, stream) == 0
            ys.append(y.cpu())
        del fscr
        bscr = torch.full((sizes[2],), nan, device=dev)
        grads = [torch.full_like(t, nan) for t in plist]
        garr = (ctypes.c_void_p * 20)(*[P(t) for t in grads])
        assert lib.cpc_encoder_backward_c(P(wd), parr, P(saved), P(z), P(dzd), P(bscr), garr, B, L, C, stream) == 0
        torch.cuda.synchronize()
        out.append((z.cpu(), ys, [g.cpu() for g in grads]))
        del saved, bscr
    return p, wave, dz, out


def _oracle64(p, wave, dz, relu_override):
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in p.items() if k.startswith("gEncoder")}
    acts = []
    with torch.backends.mkldnn.flags(enabled=False):
        z = O.encoder_forward(leaves, wave.double(), collect=acts, relu_override=relu_override).permute(0, 2, 1)
        (z * dz.double()).sum().backward()
    return z.detach(), [a.detach().permute(0, 2, 1) for a in acts], leaves


# one 64-column block, a block edge, a ragged last block, the full eight; the uncovered layer-0 step (978), the one-step window
# (170); (40, 8, 20480) and (512, 4, 20480): several row tiles per layer and several weight-gradient splits at the step's window
CASES = [(3, 2, 1280), (13, 3, 978), (64, 2, 2560), (65, 2, 1370), (130, 2, 1280), (272, 2, 1280), (512, 2, 1280), (512, 1, 170),
         (40, 8, 20480), (512, 4, 20480)]


@pytest.mark.parametrize("C,B,L", CASES)
def test_encoder_widths_match_the_float64_oracle(C, B, L):
    dev = _dev()
    from cpc_audio_amd import ops
    p, wave, dz, [(z, ys, grads)] = _device_run(C, B, L, dev)
    O.tie_report()
    z_ref, acts, leaves = _oracle64(p, wave, dz, [(y > 0).permute(0, 2, 1) for y in ys + [z]])
    ties = O.tie_report()
    print(f"relu ties: {ties}")
    assert O.tie_ok(ties) and ties["disagree_outside"] == 0, ties
    assert z_ref.shape == z.shape
    for i in range(4):
        err = (ys[i].double() - acts[i]).abs().max().item()
        print(f"y{i}: max |delta| = {err:.3g}")
        assert err < BAR, f"layer {i}"
    err = (z.double() - z_ref).abs().max().item()
    print(f"z: max |delta| = {err:.3g}")
    assert err < BAR
    bad = {}
    for n, g in zip(NAMES, grads):
        ref = leaves[n].grad
        assert g.shape == p[n].shape
        e = rel_err(g.view_as(ref), ref) if torch.isfinite(g).all() else float("inf")
        print(f"{n}: {e:.3g}")
        if not e < BAR:
            bad[n] = e
    assert not bad, bad
    ops.check_device_errors(clear=True)


def test_two_runs_give_the_same_bits():
    dev = _dev()
    _, _, _, (a, b) = _device_run(130, 2, 1280, dev, repeat=2)
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0])
    for u, v in zip(a[2], b[2]):
        assert torch.isfinite(u).all() and torch.equal(u, v)


def test_two_channels_run():
    """C = 2 is ill-conditioned (no parity bar): the calls return 0, write every output and leave no NaN."""
    dev = _dev()
    _, _, _, [(z, ys, grads)] = _device_run(2, 2, 1280, dev)
    for t in [z] + ys + grads:
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("C", [40, 512])
def test_the_module_against_a_float64_copy_of_itself(C):
    """CPCEncoder(C, encoderKernel=True) on the device against its own float64 copy on the CPU through autograd, B = 2, L = 1280:
    z over the elements whose float64 pre-activation lies at least 1e-5 from zero (no mask override here), all 20 .grads."""
    dev = _dev()
    from cpc_audio_amd import ops
    from cpc_audio_amd.model import CPCEncoder
    torch.manual_seed(C)
    enc = CPCEncoder(C, "layerNorm", encoderKernel=True)
    with torch.no_grad():                                   # (the default affine is 1 / 0: give the norms something to carry)
        for i in range(5):
            norm = getattr(enc, f"batchNorm{i}")
            norm.weight.add_(0.1 * torch.randn_like(norm.weight))
            norm.bias.add_(0.1 * torch.randn_like(norm.bias))
    ref = copy.deepcopy(enc).double()
    enc = enc.to(dev)
    assert enc.hip_wide and not enc.hip
    wave = O.make_waveform(2, 1280, seed=5)
    z = enc(wave.to(dev))
    assert tuple(z.shape) == (2, C, 8) and z.permute(0, 2, 1).is_contiguous()
    dz = torch.randn(2, C, 8, generator=torch.Generator().manual_seed(3))
    (z * dz.to(dev)).sum().backward()
    pre = []
    hook = ref.batchNorm4.register_forward_hook(lambda mod, inp, out: pre.append(out.detach()))
    with torch.backends.mkldnn.flags(enabled=False):
        z_ref = ref(wave.double())
        (z_ref * dz.double()).sum().backward()
    hook.remove()
    clear = pre[0].abs() >= 1e-5
    err = ((z.detach().double().cpu() - z_ref.detach()).abs() * clear).max().item()
    print(f"z: max |delta| = {err:.3g} over {int(clear.sum())} of {clear.numel()} elements")
    assert err < BAR
    errs = {n: rel_err(q.grad, dict(ref.named_parameters())[n].grad) for n, q in enc.named_parameters()}
    print("gradient errors", errs)
    assert len(errs) == 20 and all(q.grad.shape == q.shape for q in enc.parameters())
    assert all(e < BAR for e in errs.values()), errs
    ops.check_device_errors(clear=True)


def test_the_big_configuration_end_to_end():
    """--hiddenEncoder 512 --hiddenGar 512 --arMode LSTM with every keyword on, B = 4, one window of 20480 samples: the pieces
    meet -- a finite loss, and every parameter of the model and the criterion has a finite gradient of its own shape."""
    dev = _dev()
    from cpc_audio_amd import ops, train
    B, L = 4, 20480
    torch.manual_seed(11)
    m = train.build_model(hiddenEncoder=512, hiddenGar=512, arMode="LSTM", nLevelsGRU=1, lstmKernel=True, hiddenKernel=True,
                          encoderKernel=True).to(dev)
    crit = train.build_criterion(hiddenGar=512, hiddenEncoder=512).to(dev)
    assert m.gEncoder.hip_wide and not m.gEncoder.hip and m.gAR.hip_hidden
    wave = O.make_waveform(B, L, seed=5).to(dev)
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    S = L // 160
    c, z, _ = m(wave, None)
    assert tuple(c.shape) == (B, S, 512) and tuple(z.shape) == (B, S, 512)
    bi, si = O.draw_negative_indices(B, S, S - 12, 128, generator=torch.Generator().manual_seed(9))
    losses, acc = crit(c, z, None, negatives=(bi.to(dev), si.to(dev)))
    losses.sum().backward()
    print("losses", losses.tolist())
    assert bool(torch.isfinite(losses).all())
    params = list(m.named_parameters()) + list(crit.named_parameters())
    assert len(params) >= 20 + 4 + 12
    for n, q in params:
        assert q.grad is not None and q.grad.shape == q.shape and bool(torch.isfinite(q.grad).all()), n
        assert float(q.grad.abs().max()) > 0.0, n
    ops.check_device_errors(clear=True)
