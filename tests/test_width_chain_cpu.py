"""tests/width_chain_util.py -- the float64 model tests/test_gpu_width_chain.py holds the HIP chain to -- is itself pinned here, on
the CPU: against O.train_step where that exists (256 / 256, GRU x 2), its LSTM and RNN against torch.nn.LSTM / nn.RNN in double,
every row of the case table against the three well-posedness conditions, and the GPU test's checks against planted errors: each
must move a checked quantity by at least 100 x its bar, so that the GPU test could not pass with that bug."""
from unittest import mock

import pytest
import torch

import width_chain_util as U
from oracle import cpc_oracle as O

BAR = 1e-4                      # the GPU test's bars: max |delta| on z and c, per loss relative to max(1, |loss|), per gradient by norm
PLANT_FACTOR = 100.0


def _maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item()


# --------------------------------------------------------------------------- the model against what exists already
def test_parameters_follow_the_oracle_s_recipe():
    mine = U.make_params(256, 256, "GRU", 2, K=4, seed=1, head_scale=64.0)
    theirs = O.make_params(seed=1, head_scale=64.0, n_predicts=4)
    assert list(mine) == list(theirs)
    assert all(torch.equal(mine[k], theirs[k]) for k in mine)
    lstm = U.param_shapes(65, 100, "LSTM", 1, 4)
    assert lstm["gAR.baseNet.weight_ih_l0"] == (400, 65) and lstm["gAR.baseNet.weight_hh_l0"] == (400, 100)
    assert U.param_shapes(130, 256, "RNN", 2, 4)["gAR.baseNet.weight_ih_l1"] == (256, 256)


def test_the_chain_at_256_is_the_oracle_s_train_step():
    B, L, K, N = 2, 2560, 4, 16
    p = {k: v.double() for k, v in U.make_params(256, 256, "GRU", 2, K=K).items()}
    wave = O.make_waveform(B, L, seed=2).double()
    S = L // 160
    bi, si = O.draw_negative_indices(B, S, S - K, N, generator=torch.Generator().manual_seed(3))
    h0 = 0.3 * torch.randn(2, B, 256, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    got = U.Chain("GRU", 2, K, N).step(p, wave, bi, si, state=h0)
    with torch.backends.mkldnn.flags(enabled=False):
        want = O.train_step(p, wave, bi, si, n_predicts=K, n_neg=N, h0=h0)
    for key, ref in (("z", want["z"]), ("c", want["c"]), ("state", want["hN"]), ("losses", want["losses"])):
        assert _maxdiff(got[key], ref) <= 1e-12 * max(1.0, ref.abs().max().item()), key
    assert torch.equal(got["counts"], torch.round(want["acc"][0] * (B * (S - K))).long())
    assert set(got["grads"]) == set(want["grads"])
    for k, g in want["grads"].items():
        assert _maxdiff(got["grads"][k], g) <= 1e-12 * max(1.0, g.abs().max().item()), k
    # ... and the tail the planted criteria below score with is O.criterion_forward's
    chain = U.Chain("GRU", 2, K, N)
    losses, counts = U.losses_from_logits(chain.logits(p, want["c"], want["z"], want["ext"]))
    assert _maxdiff(losses, want["losses"]) <= 1e-12 and torch.equal(counts, got["counts"])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("given_state", [False, True])
@pytest.mark.parametrize("cell,layers", [("LSTM", 1), ("LSTM", 2), ("RNN", 1), ("RNN", 2), ("GRU", 2)])
def test_recurrences_equal_torch_s_modules_in_double(cell, layers, given_state, reverse):
    B, S, D, H = 3, 9, 13, 11
    torch.manual_seed(5)
    net = {"LSTM": torch.nn.LSTM, "RNN": torch.nn.RNN, "GRU": torch.nn.GRU}[cell](D, H, layers, batch_first=True).double()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, S, D, generator=g, dtype=torch.float64)
    dy = torch.randn(B, S, H, generator=g, dtype=torch.float64)
    n_state = 2 if cell == "LSTM" else 1
    ds = [torch.randn(layers, B, H, generator=g, dtype=torch.float64) for _ in range(n_state)]
    s0 = [0.5 * torch.randn(layers, B, H, generator=g, dtype=torch.float64) for _ in range(n_state)] if given_state else None

    def pack(ts):
        return None if ts is None else (tuple(ts) if cell == "LSTM" else ts[0])

    def objective(y, st):
        st = st if isinstance(st, tuple) else (st,)
        return (y * dy).sum() + sum((a * b).sum() for a, b in zip(st, ds))

    xr = x.clone().requires_grad_(True)
    yr, sr = net(torch.flip(xr, [1]) if reverse else xr, pack(s0))
    yr = torch.flip(yr, [1]) if reverse else yr
    objective(yr, sr).backward()
    p = {"gAR.baseNet." + n: q.detach().clone().requires_grad_(True) for n, q in net.named_parameters()}
    xm = x.clone().requires_grad_(True)
    y, st = U.recurrence(p, xm, cell, layers, pack(s0), reverse)
    objective(y, st).backward()
    assert _maxdiff(y, yr) <= 1e-10
    for a, b in zip(st if isinstance(st, tuple) else (st,), sr if isinstance(sr, tuple) else (sr,)):
        assert a.shape == b.shape and _maxdiff(a, b) <= 1e-10
    assert _maxdiff(xm.grad, xr.grad) <= 1e-10
    for n, q in net.named_parameters():
        assert _maxdiff(p["gAR.baseNet." + n].grad, q.grad) <= 1e-10, n


# --------------------------------------------------------------------------- the case table is well-posed
@pytest.fixture(scope="module")
def clean():
    """Every row's float64 step, computed once: {name: (case, parameters, wave, bi, si, result)}."""
    out = {}
    for name in U.CASES:
        cs, p, w, bi, si = U.case_inputs(name)
        out[name] = (cs, p, w, bi, si, U.Chain(**cs).step(p, w, bi, si))
    return out


def _assert_well_posed(rep, tag, allow_near_zero=False):
    print(f"{tag}: {rep['near_zero']} of {rep['preactivations']} pre-activations within {U.TIE_EPS:g} of zero; distinct-candidate "
          f"margin {min(rep['margin']):.3g}; |loss - ln(N+1)| >= {min(rep['ln_gap']):.3g}; first-index rows {rep['first_index_rows']}")
    assert allow_near_zero or rep["near_zero"] == 0, tag                                  # (a)
    assert min(rep["margin"]) >= U.MARGIN_MIN, tag                                        # (b)
    assert min(rep["ln_gap"]) >= U.LN_GAP_MIN, tag                                        # (c)
    assert rep["tie_gap"] == 0.0, tag                  # a negative that is the positive's own z row ties with it exactly


@pytest.mark.parametrize("name", list(U.CASES))
def test_every_case_is_well_posed(clean, name):
    cs, _, _, _, _, r = clean[name]
    S = cs["L"] // 160
    assert r["z"].shape == (cs["B"], S, cs["C"]) and r["c"].shape == (cs["B"], S, cs["H"])
    assert r["report"]["preactivations"] == cs["B"] * cs["C"] * sum(cs["L"] // d for d in (5, 20, 40, 80, 160))
    assert 0 <= cs["wave"] <= 15
    _assert_well_posed(r["report"], name, allow_near_zero=cs.get("device_relu", False))
    # rows where the positive wins only by arg-max's first-index rule: equal counts on the device pin that rule
    assert sum(r["report"]["first_index_rows"]) >= 1
    assert all(g is not None and g.abs().max() > 0 for g in r["grads"].values())


def test_the_carried_window_and_the_trainer_s_steps_are_well_posed(clean):
    cs, p, _, bi, si, first = clean[U.CARRY_CASE]
    w2 = O.make_waveform(cs["B"], cs["L"], seed=U.CARRY_WAVE2)
    _assert_well_posed(U.Chain(**cs).step(p, w2, bi, si, state=first["state"], backward=False)["report"], "carried window")
    cs, p, w, bi, si, _ = clean[U.TRAINER_CASE]
    results, _ = U.adam_trajectory(U.Chain(**cs), p, w, bi, si, U.TRAINER_STEPS)
    for i, r in enumerate(results):
        _assert_well_posed(r["report"], f"trainer step {i}")


# --------------------------------------------------------------------------- planted errors
def _ratios(got, want):
    """Every quantity the GPU test checks, as error / bar."""
    out = {"z": _maxdiff(got["z"], want["z"]) / BAR, "c": _maxdiff(got["c"], want["c"]) / BAR,
           "losses": ((got["losses"] - want["losses"]).abs() / (BAR * want["losses"].abs().clamp_min(1.0))).max().item(),
           "counts": 0.0 if torch.equal(got["counts"], want["counts"]) else float("inf")}
    for k, g in want["grads"].items():
        out[k] = U.rel_err(got["grads"][k], g) / BAR
    return out


class _FromLogits(U.Chain):
    def score(self, p, c, z, ext):
        return U.losses_from_logits(self.logits(p, c, z, ext))


class BiasedVariance(U.Chain):
    """ChannelNorm with the biased variance (divisor C)."""

    def encode(self, p, wave, relu_override=None):
        def biased(x, weight, bias, eps=O.CHANNEL_NORM_EPS):
            d = x - x.mean(dim=1, keepdim=True)
            return d * torch.rsqrt((d * d).mean(dim=1, keepdim=True) + eps) * weight + bias
        with mock.patch.object(O, "channel_norm", biased):
            return super().encode(p, wave, relu_override)


class PositiveOneStepEarly(_FromLogits):
    """The positive taken at t + k - 1."""

    def logits(self, p, c, z, ext):
        if self.reverse:
            c, z = torch.flip(c, [1]), torch.flip(z, [1])
        right = O.criterion_logits(p, c, z, ext, self.K)
        early = O.criterion_logits(p, c, torch.roll(z, 1, dims=1), ext, self.K)
        return [torch.cat([e[:, :1], r[:, 1:]], dim=1) for e, r in zip(early, right)]


class SummedScores(_FromLogits):
    """The score summed, not averaged, over the C channels."""

    def logits(self, p, c, z, ext):
        return [lg * z.shape[2] for lg in super().logits(p, c, z, ext)]


class NoRecurrenceTermInDz(U.Chain):
    """The recurrence's dz dropped: the encoder's input gradient is the criterion's alone."""

    def recur(self, p, z, state):
        return super().recur(p, z.detach(), state)


class FlipOfCOnly(_FromLogits):
    """Criterion mode "reverse" flipping c but not z."""

    def logits(self, p, c, z, ext):
        return O.criterion_logits(p, torch.flip(c, [1]) if self.reverse else c, z, ext, self.K)


class PadColumnRead(_FromLogits):
    """The pad of z, modelled explicitly: z stored at 64 ceil(C / 64) columns, the first pad column set to 1.  Where its counterpart
    is the zero F.pad gives the predictions such a column is inert (it adds to no score; F.pad's backward cuts its gradient), so
    the plant models the way it does reach a result: the criterion reading that storage as a contiguous (B S, C) z."""

    def logits(self, p, c, z, ext):
        B, S, C = z.shape
        Cp = 64 * ((C + 63) // 64)
        stored = torch.nn.functional.pad(z, (0, Cp - C)).clone()
        stored[:, :, C] = 1.0
        return super().logits(p, c, stored.reshape(-1)[:B * S * C].view(B, S, C), ext)


PLANTS = [(BiasedVariance, lambda cs: True), (PositiveOneStepEarly, lambda cs: True), (SummedScores, lambda cs: True),
          (NoRecurrenceTermInDz, lambda cs: True), (FlipOfCOnly, lambda cs: cs["reverse"]),
          (PadColumnRead, lambda cs: cs["C"] % 64 != 0)]


@pytest.mark.parametrize("plant,applies", PLANTS, ids=[p.__name__ for p, _ in PLANTS])
def test_planted_errors_would_fail_the_gpu_test(clean, plant, applies):
    names = [n for n in U.CASES if applies(U.CASES[n])]
    assert names
    for name in names:
        cs, p, w, bi, si, want = clean[name]
        ratios = _ratios(plant(**cs).step(p, w, bi, si), want)
        counts = ratios.pop("counts")                      # (any change of a count fails the GPU test; not relied on here)
        worst = max(ratios, key=ratios.get)
        print(f"{plant.__name__} at {name}: {worst} moves by {ratios[worst]:.3g} x its bar; counts {'differ' if counts else 'equal'}")
        assert ratios[worst] >= PLANT_FACTOR, (name, ratios)


def test_a_state_that_is_not_carried_would_fail_the_gpu_test(clean):
    cs, p, _, bi, si, first = clean[U.CARRY_CASE]
    w2 = O.make_waveform(cs["B"], cs["L"], seed=U.CARRY_WAVE2)
    chain = U.Chain(**cs)
    want = chain.step(p, w2, bi, si, state=first["state"])
    ratios = _ratios(chain.step(p, w2, bi, si, state=None), want)
    print({k: f"{v:.3g}" for k, v in ratios.items()})
    assert ratios["z"] == 0.0 and ratios["c"] >= PLANT_FACTOR and ratios["losses"] >= PLANT_FACTOR, ratios
    assert _maxdiff(first["state"][0], torch.zeros(())) > 100 * BAR
