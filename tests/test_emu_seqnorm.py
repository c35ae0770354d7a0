"""The PER phone classifier's seqNorm / dropout kernels (csrc/seqnorm.hip) on the host SIMT emulator against torch in float64
on the CPU: cpc_seqnorm_forward and cpc_seqnorm_backward on the 16-byte path and on the scalar path (pointers 4 bytes past a
16-byte boundary).  Every output buffer carries spare canary floats that must stay untouched.

Tolerances are the project's own (tests/test_emu_supervised.py, tests/test_emu_phone_head.py): forward 1e-5, gradients 1e-4
as norm-relative error.  fp32 two-pass statistics stay within 2e-6 of float64 on the offset cases; E[x^2] - m^2 is off by
5e-5 .. 2e-3 there, so the forward bar separates the two.  The kernel's time tile is 32 frames (kSnTile): S = 45 and S = 130
both end in a ragged tile, 130 crosses four whole ones."""
import pytest
import torch

from emu_util import emu
from seqnorm_util import BACKWARD_CASES, FORWARD_CASES, H, LENGTH_RANGE, P, case, oracle, rel_err, run_backward, run_forward

CANARY = 64


def _tail_ok(buf, n, fill=7.0):
    tail = buf[n:]
    return tail.numel() == CANARY and bool((tail == fill).all())


@pytest.mark.parametrize("scalar", [False, True], ids=["vec16", "scalar"])
@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_matches_float64_emulated(name, scalar):
    lib = emu()
    B, S, lengths, offset = FORWARD_CASES[name]
    x, lens, _, scale = case(B, S, lengths, offset, seed=B + S)
    x0 = x.clone()
    y, stats = run_forward(lib, x, lens, None, canary=CANARY, scalar=scalar)
    ref = oracle(x, lens)
    n = B * S * H
    err = rel_err(y[:n].double().view(B, S, H), ref["y"])
    print(f"{name} scalar={scalar}: forward error {err:.3g}")
    assert err < 1e-5
    st = stats[:B * 2 * H].double().view(B, 2, H)
    assert rel_err(st[:, 0], ref["m"]) < 1e-5 and rel_err(st[:, 1], ref["r"]) < 1e-5
    assert _tail_ok(y, n) and _tail_ok(stats, B * 2 * H) and torch.equal(x, x0)
    ys, _ = run_forward(lib, x, lens, scale, canary=CANARY, scalar=scalar)       # the dropout's factor: 0 or 2 per (b, c)
    assert rel_err(ys[:n].double().view(B, S, H), oracle(x, lens, scale)["y"]) < 1e-5
    assert bool((ys[:n].view(B, S, H)[:, :, 0] == 0).all()) and _tail_ok(ys, n)
    assert lib.cpc_device_error_flags(1) == 0


def test_forward_variants_share_their_bits_emulated():
    """lengths NULL against all-S lengths, stats NULL against given, the scalar path against the 16-byte path."""
    lib = emu()
    x, lens, _, scale = case(2, 130, [130, 67], 30.0, seed=3)
    full = torch.tensor([130, 130])
    y_null, st_null = run_forward(lib, x, None, scale, canary=CANARY)
    y_full, st_full = run_forward(lib, x, full, scale, canary=CANARY)
    assert torch.equal(y_null, y_full) and torch.equal(st_null, st_full)
    assert rel_err(y_null[:2 * 130 * H].double().view(2, 130, H), oracle(x, None, scale)["y"]) < 1e-5
    y, st = run_forward(lib, x, lens, scale, canary=CANARY)
    y_nostats, none = run_forward(lib, x, lens, scale, want_stats=False, canary=CANARY)
    assert none is None and torch.equal(y, y_nostats)
    y_scalar, st_scalar = run_forward(lib, x, lens, scale, canary=CANARY, scalar=True)
    assert torch.equal(y, y_scalar) and torch.equal(st, st_scalar)
    mixed = torch.full((2 * 130 * H + 5,), 7.0)                    # only the output misaligned: the scalar path again
    off = (1 - mixed.data_ptr() // 4) % 4
    assert lib.cpc_seqnorm_forward(P(x), P(lens), P(scale), mixed[off:].data_ptr(), None, 2, 130, 1, None) == 0
    assert torch.equal(mixed[off:off + 2 * 130 * H], y[:2 * 130 * H]) and bool((mixed[off + 2 * 130 * H:] == 7.0).all())


@pytest.mark.parametrize("scalar", [False, True], ids=["vec16", "scalar"])
def test_scale_only_is_exact_emulated(scalar):
    """normalise off: y = x * scale and dx = dy * scale, to the bit; lengths, stats and the backward's x are not read."""
    lib = emu()
    x, _, dy, scale = case(3, 45, [45, 38, 3], 0.0, seed=4)
    y, none = run_forward(lib, x, None, scale, normalise=False, want_stats=False, canary=CANARY, scalar=scalar)
    n = 3 * 45 * H
    assert torch.equal(y[:n].view(3, 45, H), x * scale[:, None, :]) and _tail_ok(y, n)
    dx = run_backward(lib, None, dy, None, scale, None, normalise=False, canary=CANARY, scalar=scalar)
    assert torch.equal(dx[:n].view(3, 45, H), dy * scale[:, None, :]) and _tail_ok(dx, n)
    y1, _ = run_forward(lib, x, None, None, normalise=False, want_stats=False, scalar=scalar)
    assert torch.equal(y1[:n].view(3, 45, H), x)


@pytest.mark.parametrize("scalar", [False, True], ids=["vec16", "scalar"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward_matches_autograd_float64_emulated(name, with_scale, scalar):
    lib = emu()
    B, S, lengths, offset = BACKWARD_CASES[name]
    x, lens, dy, scale = case(B, S, lengths, offset, seed=B + S + 1)
    scale = scale if with_scale else None
    _, stats = run_forward(lib, x, lens, scale, scalar=scalar)
    dx = run_backward(lib, x, dy, lens, scale, stats, canary=CANARY, scalar=scalar)
    ref = oracle(x, lens, scale, dy=dy)
    n = B * S * H
    err = rel_err(dx[:n].double().view(B, S, H), ref["dx"])
    print(f"{name} scale={with_scale} scalar={scalar}: backward error {err:.3g}")
    assert err < 1e-4
    assert _tail_ok(dx, n)
    if with_scale:
        assert bool((dx[:n].view(B, S, H)[:, :, 0] == 0).all())
    if not scalar:
        assert torch.equal(dx, run_backward(lib, x, dy, lens, scale, stats, canary=CANARY, scalar=True))


def test_backward_formula_agrees_with_autograd_in_float64():
    """dx_t = r (g_t - [t < n] (G1 / n + xh_t G2 / (n - 1))) with the sums over all S frames: the cross-check of the derivation."""
    x, lens, dy, scale = case(3, 45, [45, 38, 3], 30.0, seed=9)
    ref = oracle(x, lens, scale, dy=dy)
    xd, g = x.double(), dy.double() * scale.double()[:, None, :]
    m, r = ref["m"][:, None, :], ref["r"][:, None, :]
    xh = (xd - m) * r
    n = lens.double()[:, None, None]
    valid = (torch.arange(45)[None, :, None] < lens[:, None, None]).double()
    dx = r * (g - valid * (g.sum(1, keepdim=True) / n + xh * (g * xh).sum(1, keepdim=True) / (n - 1)))
    assert rel_err(dx, ref["dx"]) < 1e-12


def test_an_utterance_has_the_same_bits_alone_and_in_a_batch_emulated():
    lib = emu()
    x, lens, dy, scale = case(3, 45, [45, 38, 3], 30.0, seed=5)
    y, st = run_forward(lib, x, lens, scale)
    dx = run_backward(lib, x, dy, lens, scale, st)
    y2, st2 = run_forward(lib, x, lens, scale)
    assert torch.equal(y, y2) and torch.equal(st, st2) and torch.equal(dx, run_backward(lib, x, dy, lens, scale, st))
    n = 45 * H
    for i in range(3):
        xi, li, si, di = x[i:i + 1].contiguous(), lens[i:i + 1].clone(), scale[i:i + 1].contiguous(), dy[i:i + 1].contiguous()
        yi, sti = run_forward(lib, xi, li, si)
        assert torch.equal(yi, y[i * n:(i + 1) * n]) and torch.equal(sti, st[i * 2 * H:(i + 1) * 2 * H]), i
        assert torch.equal(run_backward(lib, xi, di, li, si, sti), dx[i * n:(i + 1) * n]), i


def test_a_single_frame_gives_nan_for_that_utterance_only_emulated():
    """n = 1: the unbiased variance is 0 / 0, as torch.var's; the other rows keep their bits and no error is flagged."""
    lib = emu()
    x, lens, dy, scale = case(3, 45, [45, 38, 3], 0.0, seed=6)
    good_y, good_st = run_forward(lib, x, lens, scale)
    good_dx = run_backward(lib, x, dy, lens, scale, good_st)
    one = torch.tensor([45, 1, 3])
    assert bool(torch.isnan(oracle(x, one)["y"][1]).all())
    y, st = run_forward(lib, x, one, None, canary=CANARY)
    dx = run_backward(lib, x, dy, one, None, st, canary=CANARY)
    n = 45 * H
    assert bool(torch.isnan(y[n:2 * n]).all()) and bool(torch.isnan(dx[n:2 * n]).all())
    assert bool(torch.isnan(st[3 * H:4 * H]).all())
    y, st = run_forward(lib, x, one, scale, canary=CANARY)
    dx = run_backward(lib, x, dy, one, scale, st, canary=CANARY)
    for i in (0, 2):
        assert torch.equal(y[i * n:(i + 1) * n], good_y[i * n:(i + 1) * n]), i
        assert torch.equal(dx[i * n:(i + 1) * n], good_dx[i * n:(i + 1) * n]), i
    assert _tail_ok(y, 3 * n) and _tail_ok(dx, 3 * n) and _tail_ok(st, 3 * 2 * H)
    assert lib.cpc_device_error_flags(1) == 0


def test_no_frame_at_all_gives_nan_forward_and_backward_emulated():
    """n = 0: mean and variance of nothing; y, r and dx of that utterance are NaN (torch autograd's answer), no error."""
    lib = emu()
    x, lens, dy, scale = case(3, 45, [45, 38, 3], 0.0, seed=8)
    good_y, good_st = run_forward(lib, x, lens, scale)
    good_dx = run_backward(lib, x, dy, lens, scale, good_st)
    none = torch.tensor([45, 0, 3])
    y, st = run_forward(lib, x, none, None, canary=CANARY)
    dx = run_backward(lib, x, dy, none, None, st, canary=CANARY)
    n = 45 * H
    assert bool(torch.isnan(y[n:2 * n]).all()) and bool(torch.isnan(dx[n:2 * n]).all()) and bool(torch.isnan(st[3 * H:4 * H]).all())
    y, st = run_forward(lib, x, none, scale, canary=CANARY)
    dx = run_backward(lib, x, dy, none, scale, st, canary=CANARY)
    for i in (0, 2):
        assert torch.equal(y[i * n:(i + 1) * n], good_y[i * n:(i + 1) * n]), i
        assert torch.equal(dx[i * n:(i + 1) * n], good_dx[i * n:(i + 1) * n]), i
    assert _tail_ok(y, 3 * n) and _tail_ok(dx, 3 * n) and lib.cpc_device_error_flags(1) == 0


@pytest.mark.parametrize("bad", [46, -1])
def test_a_length_out_of_range_is_flagged_and_clamped_emulated(bad):
    lib = emu()
    lib.cpc_device_error_flags(1)
    x, lens, dy, scale = case(3, 45, [45, 38, 3], 0.0, seed=7)
    clamped = torch.tensor([45 if bad > 0 else 0, 38, 3])
    want_y, want_st = run_forward(lib, x, clamped, scale)
    assert lib.cpc_device_error_flags(1) == 0
    y, st = run_forward(lib, x, torch.tensor([bad, 38, 3]), scale, canary=CANARY)
    assert lib.cpc_device_error_flags(1) == LENGTH_RANGE
    n = 3 * 45 * H
    assert torch.equal(y[45 * H:n], want_y[45 * H:n]) and _tail_ok(y, n) and _tail_ok(st, 3 * 2 * H)
    if bad > 0:
        assert torch.equal(y[:n], want_y[:n])
    dx = run_backward(lib, x, dy, torch.tensor([bad, 38, 3]), scale, st, canary=CANARY)
    assert lib.cpc_device_error_flags(1) == LENGTH_RANGE and _tail_ok(dx, n)
    assert lib.cpc_device_error_flags(1) == 0


def test_arguments_are_checked_before_any_launch_emulated():
    lib = emu()
    buf = torch.full((2 * H,), 7.0)
    out = torch.full((2 * H,), 7.0)
    lens = torch.ones(1, dtype=torch.long)
    fwd, bwd = lib.cpc_seqnorm_forward, lib.cpc_seqnorm_backward
    assert fwd(P(buf), P(lens), None, P(out), None, 0, 1, 1, None) == 1
    assert fwd(P(buf), P(lens), None, P(out), None, 1, 0, 1, None) == 1
    assert fwd(P(buf), P(lens), None, P(out), None, 1 << 15, 1 << 8, 1, None) == 1        # B S 256 = 2^31
    assert fwd(None, P(lens), None, P(out), None, 1, 1, 1, None) == 2
    assert fwd(P(buf), P(lens), None, None, None, 1, 1, 1, None) == 2
    assert fwd(P(buf), P(lens), None, P(buf), None, 1, 1, 1, None) == 2                   # in place
    assert fwd(P(buf), P(lens), None, P(out), None, 1, 1, 2, None) == 2
    assert bwd(P(buf), P(buf), P(lens), None, P(buf), P(out), 0, 1, 1, None) == 1
    assert bwd(P(buf), P(buf), P(lens), None, P(buf), P(out), 1 << 15, 1 << 8, 1, None) == 1
    assert bwd(P(buf), None, P(lens), None, P(buf), P(out), 1, 1, 1, None) == 2
    assert bwd(P(buf), P(buf), P(lens), None, P(buf), None, 1, 1, 1, None) == 2
    assert bwd(None, P(buf), P(lens), None, P(buf), P(out), 1, 1, 1, None) == 2           # normalise needs x ...
    assert bwd(P(buf), P(buf), P(lens), None, None, P(out), 1, 1, 1, None) == 2           # ... and the statistics
    assert bwd(P(buf), P(buf), P(lens), None, P(buf), P(out), 1, 1, -1, None) == 2
    assert bool((buf == 7.0).all()) and bool((out == 7.0).all())
    assert bwd(None, P(buf), None, None, None, P(out), 1, 1, 0, None) == 0                # scale-only: neither is read
    assert torch.equal(out[:H], buf[:H]) and bool((out[H:] == 7.0).all())
