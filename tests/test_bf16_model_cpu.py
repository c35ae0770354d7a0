"""tests/bf16_model.py before it is trusted anywhere (pure CPU, no kernel):
 * with every rounding switched off, its stages chained in float64 ARE the encoder: they reproduce oracle.cpc_oracle.encoder_forward
   plus autograd to 1e-10 on every activation and every gradient;
 * its comparison rules reject the ways a kernel of the bf16-storage variant goes wrong without moving a norm -- one element two
   bf16 ulps off, a swapped channel pair, a zeroed last row of a ragged tile, a dropped row split of a weight gradient, a
   non-zero value where no window reaches -- and accept an honest float32 run."""
import pytest
import torch

import bf16_model as M
from oracle import cpc_oracle as O


@pytest.mark.parametrize("B,L", [(2, 978), (1, 1370)])
def test_model_without_rounding_is_the_oracle_encoder_in_float64(B, L):
    p = O.make_params(seed=0)
    plist = [p[n].double() for n in M.NAMES]
    wave = O.make_waveform(B, L, seed=5).double()
    leaves = {n: t.clone().requires_grad_(True) for n, t in zip(M.NAMES, plist)}
    acts = []
    with torch.backends.mkldnn.flags(enabled=False):
        z = O.encoder_forward(leaves, wave, collect=acts)
        dz = torch.randn(z.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        (z * dz).sum().backward()
        m_acts, m_grads = M.chain(plist, wave, dz.permute(0, 2, 1), torch.float64, rnd=False)
    for i in range(5):
        ref = acts[i].detach().permute(0, 2, 1)
        assert (m_acts[i] - ref).abs().max().item() <= 1e-10 * ref.abs().max().item(), f"activation {i}"
    for n, g in zip(M.NAMES, m_grads):
        ref = leaves[n].grad
        assert (g.reshape(ref.shape) - ref).abs().max().item() <= 1e-10 * ref.abs().max().item(), n


def test_bf16_round_and_ulp():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.75, 3.0e-5, 0.0], dtype=torch.float64)
    # ties to even: 1 + 2^-8 is half-way between 1 and 1 + 2^-7 -> 1; 1 + 3 2^-8 -> 1 + 2^-6
    assert M.bf16_round(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -0.75, float(torch.tensor(3.0e-5).bfloat16()), 0.0]
    assert M.bf16_ulp(torch.tensor([1.0, 1.99, 2.0, -0.75, 0.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133]
    # the float32 value is what gets rounded: a float64 a hair above a tie that float32 cannot hold goes to the tie's even side
    assert M.bf16_round(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)).item() == 1.0
    buf = torch.zeros(8)
    buf[2:4].view(torch.bfloat16)[:] = torch.tensor([1.5, -2.0, 0.25, 3.0], dtype=torch.bfloat16)
    assert M.read_bf16(buf, 2, (3,)).float().tolist() == [1.5, -2.0, 0.25]


@pytest.fixture(scope="module")
def stage():
    """One forward stage (layer 2, 75 output rows: a 64-row tile and a ragged one of 11), one data gradient with an uncovered
    input step (layer 1, 195 = 4 48 + 3 steps) and one weight gradient (200 rows = 128 + 72), each as float64 / float32 pair on
    bf16-valued inputs; the 'device' is the honest float32 run."""
    g = torch.Generator().manual_seed(3)
    p = O.make_params(seed=0)
    plist = [p[n] for n in M.NAMES]
    x = M.bf16_round(torch.randn(1, 150, M.C, generator=g).relu())
    fwd = M._pair(lambda dt: M.layer_forward(2, x, *plist[8:12], dt)["y"])
    dx1 = M.bf16_round(torch.randn(1, 48, M.C, generator=g))
    dg = M._pair(lambda dt: M.dgrad(1, dx1, plist[4], 195, dt))
    zero = torch.zeros(1, 195, 1, dtype=torch.bool)
    zero[:, M.uncovered_steps(195, 1)] = True
    assert M.uncovered_steps(195, 1) == [194] and M.uncovered_steps(192, 1) == [] and M.uncovered_steps(511, 2) == []
    dx2 = M.bf16_round(torch.randn(1, 200, M.C, generator=g))
    xin = M.bf16_round(torch.randn(1, 400, M.C, generator=g).relu())
    wg = M._pair(lambda dt: M.wgrad(2, dx2, xin, dt))
    cut = dx2.clone()
    cut[:, 128:] = 0                                             # the second row split never summed
    wg_cut = M.wgrad(2, cut, xin, torch.float32)
    return {"fwd": fwd, "dg": dg, "zero": zero, "wg": wg, "wg_cut": wg_cut}


def _bf16_ok(m64, m32, dev, zero=None):
    rep = M.Report("self-test")
    rep.bf16("t", dev, m64, m32, zero=zero)
    return rep.ok


def test_checker_accepts_an_honest_float32_run(stage):
    m64, m32 = stage["fwd"]
    assert _bf16_ok(m64, m32, M.bf16_round(m32))
    m64, m32 = stage["dg"]
    assert _bf16_ok(m64, m32, M.bf16_round(m32), stage["zero"])
    rep = M.Report("self-test")
    rep.f32("dw", stage["wg"][1], *stage["wg"])
    assert rep.ok


def test_checker_rejects_one_element_two_ulps_off(stage):
    m64, m32 = stage["fwd"]
    dev = M.bf16_round(m32)
    r, c = 70, int(dev[0, 70].argmax())
    for sign in (1, -1):
        bad = dev.clone()
        bad[0, r, c] += sign * 2 * float(M.bf16_ulp(dev[0, r, c]))
        assert bad[0, r, c] == M.bf16_round(bad[0, r, c])        # still a bf16 value
        assert not _bf16_ok(m64, m32, bad)


def test_checker_rejects_a_swapped_channel_pair(stage):
    m64, m32 = stage["fwd"]
    dev = M.bf16_round(m32)
    r = 33
    c = 2 * int((dev[0, r, 0::2] - dev[0, r, 1::2]).abs().argmax())          # the lane pair (c, c + 1) packs one dword
    bad = dev.clone()
    bad[0, r, c], bad[0, r, c + 1] = dev[0, r, c + 1], dev[0, r, c]
    assert not _bf16_ok(m64, m32, bad)


def test_checker_rejects_a_zeroed_last_row_of_a_ragged_tile(stage):
    m64, m32 = stage["fwd"]
    bad = M.bf16_round(m32)
    assert bad.shape[1] == 75 and (bad[0, 74] > 0).any()
    bad[0, 74] = 0
    assert not _bf16_ok(m64, m32, bad)


def test_checker_rejects_a_dropped_row_split_of_a_weight_gradient(stage):
    rep = M.Report("self-test")
    rep.f32("dw", stage["wg_cut"], *stage["wg"])
    assert not rep.ok


def test_checker_rejects_a_nonzero_value_in_an_uncovered_row(stage):
    m64, m32 = stage["dg"]
    bad = M.bf16_round(m32)
    assert (bad[0, 194] == 0).all()
    bad[0, 194, 7] = 2.0 ** -100                                 # far inside any tolerance: only the structural rule sees it
    assert not _bf16_ok(m64, m32, bad, stage["zero"])
    assert _bf16_ok(m64, m32, bad)                               # (without the rule it passes: the rule is what rejects it)
