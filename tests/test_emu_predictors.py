"""The feed-forward prediction networks' kernels (csrc/pred_conv.hip: --rnnMode ffd / conv4 / conv8 / conv12) on the host SIMT
emulator against this package's torch modules in float64 on the CPU: cpc_pred_conv_forward and _backward through the C ABI.
Every output buffer carries spare canary floats that must stay untouched.

Bars are the project's emulator bars (tests/test_emu_phone_head.py): rel_err < 1e-5 for outputs and for gradients."""
import pytest
import torch

from emu_util import emu
from pred_conv_util import (CASES, H, canaries_ok, check_against_oracle, conv_case, rel_err, run, scale_of,
                            without_relu_ties)

CANARY = 64
BAR = 1e-5


@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_causal_conv_matches_shifted_conv_float64_emulated(name):
    """Cases a, b, c, e: the shared-input form without ReLU, i.e. K ShiftedConv heads."""
    lib = emu()
    B, W, G, ks = CASES[name]
    x, w, b, dy = conv_case(B, W, G, ks)
    out = run(lib, x, w, b, True, False, dy=dy, canary=CANARY)
    check_against_oracle(out, x, w, b, dy, True, False, BAR, BAR, show=name)
    canaries_ok(out, CANARY)


@pytest.mark.parametrize("name", ["a_window_shorter_than_taps", "c_ragged_row_tiles"])
def test_exact_f32_mfma_mode_emulated(name):
    """cpc_set_mfma_mode(0): the same calls on the exact-f32 MFMA tiles (the default runs three bf16 pieces per operand)."""
    lib = emu()
    B, W, G, ks = CASES[name]
    x, w, b, dy = conv_case(B, W, G, ks)
    mode = lib.cpc_get_mfma_mode()
    assert mode != 0
    try:
        assert lib.cpc_set_mfma_mode(0) == 0
        out = run(lib, x, w, b, True, False, dy=dy, canary=CANARY)
        again = run(lib, x, w, b, True, False, dy=dy)
    finally:
        assert lib.cpc_set_mfma_mode(mode) == 0
    check_against_oracle(out, x, w, b, dy, True, False, BAR, BAR, show=name + " exact")
    canaries_ok(out, CANARY)
    for k in ("y", "dw", "db", "dx"):
        assert torch.equal(out[k][:out["n"][k]], again[k]), k


def test_batch_items_do_not_read_each_other_emulated():
    """Case b: three batch items inside one row tile.  Changing item 0's input must not move one output bit of items 1 and 2,
    nor one bit of their input gradient."""
    lib = emu()
    B, W, G, ks = CASES["b_three_items_in_one_tile"]
    x, w, b, dy = conv_case(B, W, G, ks)
    base = run(lib, x, w, b, True, False, dy=dy)
    x2 = x.clone()
    x2[0] = torch.randn(W, H, generator=torch.Generator().manual_seed(77)) * 50.0
    moved = run(lib, x2, w, b, True, False, dy=dy)
    y0, y1 = base["y"].view(B, W, G * H), moved["y"].view(B, W, G * H)
    assert torch.equal(y0[1:], y1[1:]) and not torch.equal(y0[0], y1[0])
    dy2 = dy.clone()
    dy2[0] *= 3.0
    moved = run(lib, x, w, b, True, False, dy=dy2)
    d0, d1 = base["dx"].view(B, W, H), moved["dx"].view(B, W, H)
    assert torch.equal(d0[1:], d1[1:]) and not torch.equal(d0[0], d1[0])
    # ... and an item alone gives the bits it gives inside the batch
    alone = run(lib, x[1:2].contiguous(), w, b, True, False, dy=dy[1:2].contiguous())
    assert torch.equal(alone["y"], base["y"][W * G * H:2 * W * G * H])
    assert torch.equal(alone["dx"], base["dx"][W * H:2 * W * H])


@pytest.mark.parametrize("B,W,G", [(2, 6, 3), (2, 70, 2)])
def test_ffd_layers_relu_shared_then_per_head_emulated(B, W, G):
    """Case d, ks = 1: lin1 (shared input, ReLU epilogue, masked backward), then lin2 on lin1's output (per-head input).  Each
    call against the oracle, and the chain against FFNetwork.double() itself."""
    lib = emu()
    x, w1, b1, dh = conv_case(B, W, G, 1, seed=1)
    _, w2, b2, dy = conv_case(B, W, G, 1, seed=2)
    dh, _ = without_relu_ties(x, w1, b1, True, dh)
    o1 = run(lib, x, w1, b1, True, True, dy=dh, canary=CANARY)
    check_against_oracle(o1, x, w1, b1, dh, True, True, BAR, BAR, show="lin1")
    canaries_ok(o1, CANARY)
    h = o1["y"][:B * W * G * H].view(B, W, G * H).clone()
    assert bool((h == 0).any()) and bool((h > 0).any())            # the ReLU did something
    o2 = run(lib, h, w2, b2, False, False, dy=dy, canary=CANARY)
    check_against_oracle(o2, h, w2, b2, dy, False, False, BAR, BAR, show="lin2")
    canaries_ok(o2, CANARY)
    # the two calls chained = K FFNetworks (criterion.py:11-20), forward and every gradient
    from cpc_audio_amd.criterion import FFNetwork
    xr = x.double().clone().requires_grad_(True)
    nets = []
    for g in range(G):
        net = FFNetwork(H, H, H, 0).double()
        with torch.no_grad():
            net.lin1.module.weight.copy_(w1[g, :, :, 0]); net.lin1.module.bias.copy_(b1[g])
            net.lin2.module.weight.copy_(w2[g, :, :, 0]); net.lin2.module.bias.copy_(b2[g])
        nets.append(net)
    ref = torch.cat([net(xr) for net in nets], dim=2)
    (ref * dy.double()).sum().backward()
    assert rel_err(o2["y"][:ref.numel()].double().view_as(ref), ref.detach()) < BAR
    dh_chain = o2["dx"][:B * W * G * H].view(B, W, G * H).clone()
    back = run(lib, x, w1, b1, True, True, dy=dh_chain)
    assert rel_err(back["dx"].double().view_as(xr.grad), xr.grad) < BAR
    dw1 = torch.stack([n.lin1.module.weight.grad for n in nets])
    assert rel_err(back["dw"].double().view(G, H, H), dw1) < BAR
    assert rel_err(back["db"].double().view(G, H), torch.stack([n.lin1.module.bias.grad for n in nets])) < BAR
    assert scale_of(1) == nets[0].lin1.weight


def test_per_head_input_with_several_taps_emulated():
    """The per-head input form is not only for ks = 1: a window over a (B, W, G*256) tensor walks rows G*256 apart."""
    lib = emu()
    x, w, b, dy = conv_case(2, 6, 3, 4, shared=False)
    dy, _ = without_relu_ties(x, w, b, False, dy)
    for relu in (False, True):
        out = run(lib, x, w, b, False, relu, dy=dy, canary=CANARY)
        check_against_oracle(out, x, w, b, dy, False, relu, BAR, BAR, show=f"per-head relu={relu}")
        canaries_ok(out, CANARY)


def test_identical_calls_give_identical_bits_and_null_dx_emulated():
    """Case f (on case c: several row slabs and row tiles): two backward calls give bit-identical dw, db and dx; dx = NULL
    (a frozen context) leaves dw and db as they are."""
    lib = emu()
    B, W, G, ks = CASES["c_ragged_row_tiles"]
    x, w, b, dy = conv_case(B, W, G, ks)
    a1, a2 = run(lib, x, w, b, True, False, dy=dy), run(lib, x, w, b, True, False, dy=dy)
    for k in ("y", "dw", "db", "dx"):
        assert torch.equal(a1[k], a2[k]), k
    none = run(lib, x, w, b, True, False, dy=dy, need_dx=False, canary=CANARY)
    assert none["dx"] is None
    assert torch.equal(none["dw"][:w.numel()], a1["dw"]) and torch.equal(none["db"][:b.numel()], a1["db"])
    canaries_ok(none, CANARY)


def test_arguments_are_checked_before_any_launch_emulated():
    lib = emu()
    x, w, b, dy = conv_case(1, 2, 1, 1)
    buf = torch.zeros(1 << 17)
    p = lambda t: t.data_ptr()
    s = scale_of(1)
    assert lib.cpc_pred_conv_forward(p(x), p(w), p(b), p(buf), p(buf), 1, 2, 0, 1, 1, s, 0, None) == 1        # G = 0
    assert lib.cpc_pred_conv_forward(p(x), p(w), p(b), p(buf), p(buf), 1, 2, 1, 17, 1, s, 0, None) == 1       # ks = 17
    assert lib.cpc_pred_conv_forward(p(x), p(w), p(b), None, p(buf), 1, 2, 1, 1, 1, s, 0, None) == 2
    assert lib.cpc_pred_conv_backward(p(x), p(w), None, p(dy), p(buf), p(buf), p(buf), None, 0, 2, 1, 1, 1, s, 0, None) == 1
    assert lib.cpc_pred_conv_backward(p(x), p(w), None, p(dy), p(buf), p(buf), p(buf), None, 1, 2, 1, 1, 1, s, 1, None) == 2   # relu, no y
    assert lib.cpc_pred_conv_backward(p(x), p(w), None, None, p(buf), p(buf), p(buf), None, 1, 2, 1, 1, 1, s, 0, None) == 2
