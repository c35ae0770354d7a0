"""The encoder's batchNorm / instanceNorm / ID modes on an MI355X (csrc/enc_wide.hip: cpc_encoder_*_n; ops.EncoderNormFunction;
model.CPCEncoder with encoderKernel=True) against the float64 reference of tests/encoder_norms_util.py on the CPU.
Bar: max |delta| < 1e-4 on y0..y3 and z, norm-wise relative error < 1e-4 on every gradient (encoder_norms_util.compare has the one
exception, the conv bias gradient where the normalisation removes the mean)."""
import copy

import pytest
import torch

import encoder_norms_util as U
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

BAR = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _run(mode, training, C, B, L, dev, bias_offset=0.0, **kw):
    from cpc_audio_amd import _lib
    params, running = U.make_params(C, mode, bias_offset=bias_offset)
    wave = O.make_waveform(B, L, seed=5)
    res = U.run_abi(_lib.get(), mode, training, C, B, L, params, running, wave, dev=dev, stream=torch.cuda.current_stream().cuda_stream,
                    **kw)
    torch.cuda.synchronize()
    return params, running, wave, res


def _check_running(mode, training, res, running, run_ref):
    if mode != "batchNorm":
        return
    for i, (a, b) in enumerate(zip(res["running"], run_ref if training else running)):
        if training:
            assert U.rel_err(a, b) < 1e-5, i                # one training call against torch's
        else:
            assert torch.equal(a, b), i                     # an eval call leaves the buffers bit-unchanged


@pytest.mark.parametrize("C,B,L", U.CASES)
@pytest.mark.parametrize("mode,training", U.VARIANTS)
def test_norm_modes_match_the_float64_reference(mode, training, C, B, L):
    dev = _dev()
    from cpc_audio_amd import ops
    params, running, wave, res = _run(mode, training, C, B, L, dev)
    run_ref = U.compare(mode, training, params, running, wave, res, BAR)
    _check_running(mode, training, res, running, run_ref)
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("mode,training", U.VARIANTS)
def test_a_conv_bias_of_ten_keeps_the_bar(mode, training):
    """The offset case of tests/test_emu_encoder_norms.py.  torch fp32 stays under half of 1e-4 on it, so the bar is the ordinary one."""
    dev = _dev()
    from cpc_audio_amd import ops
    C, B, L, off = U.OFFSET_CASE
    assert U.offset_bars(mode, training, BAR) == (BAR, BAR)
    params, running, wave, res = _run(mode, training, C, B, L, dev, bias_offset=off)
    U.compare(mode, training, params, running, wave, res, BAR)
    ops.check_device_errors(clear=True)


def test_instance_norm_with_two_steps_at_the_last_layer():
    """L_4 = 2: forward only (tests/test_emu_encoder_norms.py says why)."""
    dev = _dev()
    from cpc_audio_amd import ops
    params, running, wave, res = _run("instanceNorm", True, 30, 2, 330, dev, backward=False)
    assert res["sizes"][7] == 2
    U.compare("instanceNorm", True, params, running, wave, res, BAR, check_grads=False)
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("mode,training", [("batchNorm", True), ("instanceNorm", True)])
def test_the_steps_window(mode, training):
    """(64, 4, 20480): 256 statistics partials at layer 0 and several weight-gradient splits."""
    dev = _dev()
    from cpc_audio_amd import ops
    params, running, wave, res = _run(mode, training, 64, 4, 20480, dev)
    run_ref = U.compare(mode, training, params, running, wave, res, BAR)
    _check_running(mode, training, res, running, run_ref)
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("mode,training", [("batchNorm", True), ("instanceNorm", True), ("ID", True)])
def test_two_runs_give_the_same_bits(mode, training):
    dev = _dev()
    from cpc_audio_amd import ops
    _, _, _, a = _run(mode, training, 130, 2, 1280, dev)
    _, _, _, b = _run(mode, training, 130, 2, 1280, dev)
    assert torch.isfinite(a["z"]).all() and torch.equal(a["z"], b["z"])
    for n, g in a["grads"].items():
        assert torch.isfinite(g).all() and torch.equal(g, b["grads"][n]), n
    for u, v in zip(a["running"] or [], b["running"] or []):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    ops.check_device_errors(clear=True)


@pytest.mark.parametrize("mode", ["batchNorm", "instanceNorm", "ID"])
def test_the_module_against_its_torch_path(mode):
    """CPCEncoder(C, mode, encoderKernel=True) against a deep copy without the keyword on the same GPU: two training steps
    (forward, gradients, running buffers, num_batches_tracked), then .eval() and the forward again.  z is held to the bar, the
    gradients norm-wise to twice the bar (two fp32 paths, each within the bar of float64)."""
    dev = _dev()
    from cpc_audio_amd import ops
    from cpc_audio_amd.model import CPCEncoder
    C, B, L = 40, 3, 1290
    torch.manual_seed(C)
    enc = CPCEncoder(C, mode, encoderKernel=True)
    if mode != "ID":
        with torch.no_grad():                               # (the default affine is 1 / 0: give the norms something to carry)
            for i in range(5):
                norm = getattr(enc, f"batchNorm{i}")
                norm.weight.add_(0.1 * torch.randn_like(norm.weight))
                norm.bias.add_(0.1 * torch.randn_like(norm.bias))
    enc = enc.to(dev)
    ref = copy.deepcopy(enc)
    ref.hip_norm = False
    assert enc.hip_norm and not enc.hip and not enc.hip_wide
    zero_bias = mode != "ID"
    for step in range(2):
        wave = O.make_waveform(B, L, seed=5 + step).to(dev)
        dz = torch.randn(B, C, 8, generator=torch.Generator().manual_seed(3 + step)).to(dev)
        for m in (enc, ref):
            m.zero_grad()
        z, z_ref = enc(wave), ref(wave)
        assert tuple(z.shape) == (B, C, 8) and z.permute(0, 2, 1).is_contiguous()
        (z * dz).sum().backward()
        (z_ref * dz).sum().backward()
        err = (z - z_ref).abs().max().item()
        print(f"step {step}: z max |delta| = {err:.3g}")
        assert err < BAR
        for (n, q), (_, r) in zip(enc.named_parameters(), ref.named_parameters()):
            assert q.grad.shape == q.shape
            if zero_bias and n.startswith("conv") and n.endswith("bias"):
                continue                                    # analytically zero: rounding noise on both sides (the ABI tests bound it)
            e = U.rel_err(q.grad, r.grad)
            print(f"step {step} {n}: {e:.3g}")
            assert e < 2 * BAR, n                           # two fp32 paths, each within the bar of float64
        for (k, a), (_, b) in zip(enc.state_dict().items(), ref.state_dict().items()):
            if "running" in k:
                assert U.rel_err(a, b) < 1e-5, k
            elif "num_batches_tracked" in k:
                assert int(a) == int(b) == step + 1, k
    enc.eval()
    ref.eval()
    wave = O.make_waveform(B, L, seed=9).to(dev)
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        z, z_ref = enc(wave), ref(wave)
    err = (z - z_ref).abs().max().item()
    print(f"eval: z max |delta| = {err:.3g}")
    assert err < BAR
    for k, v in enc.state_dict().items():
        assert torch.equal(v, before[k]), k
    ops.check_device_errors(clear=True)
