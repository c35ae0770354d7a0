"""The float64 model of the whole train step at any encoder / context width: encoder -> recurrence -> criterion joined, so that
z feeds both the recurrence and the criterion and every parameter gradient of ``losses.sum()`` carries both terms.

Built from oracle.cpc_oracle (O.encoder_forward, O.gru_forward, O.negative_rows, O.criterion_forward) plus the LSTM and the tanh
RNN written the same way as O.gru_forward: the input projection of all steps up front, then S dependent steps.  Everything runs
in float64 (or, for the float32 error estimate, in ``dtype``) with oneDNN off (tests/test_gpu_encoder_widths.py says why).

tests/test_width_chain_cpu.py pins this model (against O.train_step at 256 / 256, against torch.nn.LSTM / nn.RNN in double),
checks that every row of CASES is well-posed and that planted errors move what tests/test_gpu_width_chain.py checks.
"""
import math

import torch

from oracle import cpc_oracle as O

GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}          # rows of weight_ih / weight_hh per hidden unit (LSTM: gate order i, f, g, o)
PARAM_SEED = 1
NEG_SEED = 9
TIE_EPS = 1e-5                                    # condition (a): no encoder pre-activation closer to zero than this
MARGIN_MIN = 1e-5                                 # condition (b): top-two score margin over distinct candidate rows
LN_GAP_MIN = 0.05                                 # condition (c): every head's loss this far from ln(N + 1)

# The case table: the smallest shapes at which the pieces still meet non-trivially.  ``wave`` is the seed of O.make_waveform and
# ``head_scale`` the factor on the heads, both chosen on the CPU before any device run (wave among 0..15) so that the float64 model
# meets (a), (b) and (c) -- tests/test_width_chain_cpu.py::test_every_case_is_well_posed; parameters are make_params(PARAM_SEED,
# head_scale), negatives O.draw_negative_indices under NEG_SEED.  The LSTM's |c| is small, so its heads need a larger factor to
# leave ln(N + 1).  At C = 256 no seed in 0..15 meets (a) (1 to 9 of 577,536 pre-activations within 1e-5 of zero; seed 4 has one):
# ``device_relu`` hands the device's ReLU decisions to the model inside that window, as tests/test_gpu_train_step.py does.
CASES = {
    # one ragged 64-column block; in_proj; the pad in nce_wide_scores.  (Seed 3 meets (a) too, but not on the Trainer's third step.)
    "c40_gru2_h256": dict(C=40, cell="GRU", layers=2, H=256, B=3, L=2560, K=4, N=16, reverse=False, wave=11, head_scale=64.0),
    # block edge + 1; H padded to 128; C < H
    "c65_lstm1_h100": dict(C=65, cell="LSTM", layers=1, H=100, B=3, L=2560, K=4, N=16, reverse=False, wave=0, head_scale=64.0),
    # reverse mode in both the model and the criterion
    "c130_rnn2_h256_reverse": dict(C=130, cell="RNN", layers=2, H=256, B=3, L=2560, K=4, N=16, reverse=True, wave=10,
                                   head_scale=64.0),
    # the default fp16-piece encoder feeding the wide criterion; heads with C > H
    "c256_lstm1_h64": dict(C=256, cell="LSTM", layers=1, H=64, B=3, L=2560, K=4, N=16, reverse=False, wave=4, head_scale=256.0,
                           device_relu=True),
    # the "big" configuration
    "c512_lstm2_h512": dict(C=512, cell="LSTM", layers=2, H=512, B=2, L=1280, K=3, N=8, reverse=False, wave=1, head_scale=1024.0),
}
# the second window of the state-carry check (the C = 65 row; the first window is the row's own) and the Trainer row, whose three
# Adam steps on one wave are well-posed one by one
CARRY_CASE, CARRY_WAVE2 = "c65_lstm1_h100", 5
TRAINER_CASE, TRAINER_STEPS, TRAINER_LR = "c40_gru2_h256", 3, 2e-4


def param_shapes(C, H, cell="GRU", layers=2, K=12):
    """The reference's state-dict keys and shapes in its key order (model, then criterion): O.param_shapes with the
    autoregressor's 3H rows replaced by GATES[cell] * H."""
    shapes = dict(O.param_shapes(hidden_encoder=C, hidden_gar=H, n_levels_gru=0, n_predicts=0))
    g = GATES[cell]
    for l in range(layers):
        din = C if l == 0 else H
        shapes[f"gAR.baseNet.weight_ih_l{l}"] = (g * H, din)
        shapes[f"gAR.baseNet.weight_hh_l{l}"] = (g * H, H)
        shapes[f"gAR.baseNet.bias_ih_l{l}"] = (g * H,)
        shapes[f"gAR.baseNet.bias_hh_l{l}"] = (g * H,)
    for k in range(K):
        shapes[f"wPrediction.predictors.{k}.weight"] = (C, H)
    return shapes


def make_params(C, H, cell="GRU", layers=2, K=12, seed=PARAM_SEED, head_scale=64.0):
    """The recipe of O.make_params on param_shapes above: every tensor from ONE cpu generator in key order, weights
    randn / sqrt(fan_in), biases 0.1 randn, norm weights 1 + 0.1 randn, heads times ``head_scale``.  float32, as loaded."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = {}
    for name, shape in param_shapes(C, H, cell, layers, K).items():
        r = torch.randn(shape, generator=g, dtype=torch.float32)
        if "batchNorm" in name:
            t = 1.0 + 0.1 * r if name.endswith("weight") else 0.1 * r
        elif name.endswith("bias") or ".bias_" in name:
            t = 0.1 * r
        else:
            t = r / math.sqrt(math.prod(shape[1:]))
            if name.startswith("wPrediction"):
                t = t * head_scale
        out[name] = t.contiguous()
    return out


def case_inputs(name, wave=None):
    """-> (case, parameters, wave (B,1,L), batchIdx, seqIdx) of a row of CASES (``wave``: another waveform seed)."""
    cs = CASES[name]
    p = make_params(cs["C"], cs["H"], cs["cell"], cs["layers"], cs["K"], head_scale=cs["head_scale"])
    w = O.make_waveform(cs["B"], cs["L"], seed=cs["wave"] if wave is None else wave)
    S = cs["L"] // O.DOWNSAMPLING
    bi, si = O.draw_negative_indices(cs["B"], S, S - cs["K"], cs["N"], generator=torch.Generator().manual_seed(NEG_SEED))
    return cs, p, w, bi, si


# --------------------------------------------------------------------------- the recurrences, step by step
def _layer_params(p, l, prefix):
    return (p[f"{prefix}weight_ih_l{l}"], p[f"{prefix}weight_hh_l{l}"], p[f"{prefix}bias_ih_l{l}"], p[f"{prefix}bias_hh_l{l}"])


def lstm_forward(p, x, n_levels=1, state=None, prefix="gAR.baseNet."):
    """x (B,S,Din) -> (y (B,S,H), (hN, cN) each (n_levels,B,H)); torch.nn.LSTM semantics, gate order i, f, g, o:
      c' = sigmoid(f) c + sigmoid(i) tanh(g),  h' = sigmoid(o) tanh(c')."""
    B, S, _ = x.shape
    inp, hs, cs = x, [], []
    for l in range(n_levels):
        w_ih, w_hh, b_ih, b_hh = _layer_params(p, l, prefix)
        H = w_hh.shape[1]
        gi = (inp.reshape(B * S, -1) @ w_ih.t() + b_ih).view(B, S, 4 * H)
        h = inp.new_zeros(B, H) if state is None else state[0][l]
        c = inp.new_zeros(B, H) if state is None else state[1][l]
        outs = []
        for t in range(S):
            i, f, g, o = (gi[:, t] + h @ w_hh.t() + b_hh).split(H, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        inp = torch.stack(outs, dim=1)
        hs.append(h)
        cs.append(c)
    return inp, (torch.stack(hs, dim=0), torch.stack(cs, dim=0))


def rnn_forward(p, x, n_levels=1, state=None, prefix="gAR.baseNet."):
    """x (B,S,Din) -> (y (B,S,H), hN (n_levels,B,H)); torch.nn.RNN(nonlinearity="tanh"): h' = tanh(W_ih x + b_ih + W_hh h + b_hh)."""
    B, S, _ = x.shape
    inp, hs = x, []
    for l in range(n_levels):
        w_ih, w_hh, b_ih, b_hh = _layer_params(p, l, prefix)
        H = w_hh.shape[1]
        gi = (inp.reshape(B * S, -1) @ w_ih.t() + b_ih).view(B, S, H)
        h = inp.new_zeros(B, H) if state is None else state[l]
        outs = []
        for t in range(S):
            h = torch.tanh(gi[:, t] + h @ w_hh.t() + b_hh)
            outs.append(h)
        inp = torch.stack(outs, dim=1)
        hs.append(h)
    return inp, torch.stack(hs, dim=0)


def recurrence(p, x, cell, n_levels, state=None, reverse=False):
    """CPCAR.forward: in reverse mode the sequence runs back to front and comes back in its original order; the final state is
    that of the run as it was made."""
    if reverse:
        x = torch.flip(x, [1])
    if cell == "GRU":
        y, st = O.gru_forward(p, x, n_levels=n_levels, h0=state)
    elif cell == "LSTM":
        y, st = lstm_forward(p, x, n_levels, state)
    else:
        y, st = rnn_forward(p, x, n_levels, state)
    return (torch.flip(y, [1]) if reverse else y), st


def losses_from_logits(logits):
    """The tail of O.criterion_forward on the K (B, 1+N, W) score tensors -> (losses (1,K), counts (K,) of rows whose arg-max is
    the positive)."""
    losses, counts = [], []
    for lg in logits:
        rows = lg.permute(0, 2, 1).reshape(lg.shape[0] * lg.shape[2], -1)
        losses.append((torch.logsumexp(rows, dim=1) - rows[:, 0]).mean().view(1, 1))
        counts.append((rows.argmax(dim=1) == 0).sum())
    return torch.cat(losses, dim=1), torch.stack(counts)


def score_report(logits, ext, S):
    """What makes the arg-max and the loss of a case decidable.  Per head: ``margin`` -- the smallest gap between the best score
    and the best score of a DIFFERENT z row (a negative that is the positive's own z row ties with it exactly and is legitimate:
    the arg-max then goes to the first index, the positive) --, ``first_index_rows`` -- the rows where exactly that happens at
    the top, which pin the first-index rule --, and ``tie_gap`` -- the largest score difference between two candidates that are
    the same z row (0 in float64: same operands, same reduction)."""
    B, N, W = ext.shape
    neg_ids = ext.permute(0, 2, 1).reshape(B * W, N)
    base = (torch.arange(B).view(B, 1) * S + torch.arange(W).view(1, W)).reshape(B * W, 1)
    margins, first, gap = [], [], 0.0
    for k, lg in enumerate(logits, start=1):
        rows = lg.detach().permute(0, 2, 1).reshape(B * W, -1)
        ids = torch.cat([base + k, neg_ids], dim=1)
        top = rows.argmax(dim=1, keepdim=True)
        top_id = ids.gather(1, top)
        others = rows.masked_fill(ids == top_id, float("-inf"))
        margins.append((rows.gather(1, top)[:, 0] - others.max(dim=1).values).min().item())
        dup = ids[:, 1:] == ids[:, :1]
        first.append(int((dup.any(dim=1) & (top_id[:, 0] == ids[:, 0])).sum()))
        if dup.any():
            gap = max(gap, ((rows[:, 1:] - rows[:, :1]).abs() * dup).max().item())
    return {"margin": margins, "first_index_rows": first, "tie_gap": gap}


class Chain:
    """One train step of encoder C -> ``cell`` x ``layers`` of width H -> K linear heads on N negatives, forward and
    ``losses.sum().backward()``.  The three stages are methods so that tests/test_width_chain_cpu.py can plant an error in one."""

    def __init__(self, cell, layers, K, N, reverse=False, dtype=torch.float64, **_unused):
        self.cell, self.layers, self.K, self.N, self.reverse, self.dtype = cell, layers, K, N, reverse, dtype

    # -- stages ---------------------------------------------------------------------------------------------------------------
    def encode(self, p, wave, relu_override=None):
        """-> z (B,S,C).  Leaves in ``self.ties`` O.tie_report() of the five layers: ``eligible`` counts the pre-activations
        (post-ChannelNorm, pre-ReLU) with |x| < TIE_EPS.  ``relu_override``: the device's ReLU decisions, per layer (B,C,L_i)
        (O._ReluTieAware); default: the model's own."""
        if relu_override is None:
            acts = []
            with torch.no_grad():
                O.encoder_forward(p, wave, collect=acts)
            relu_override = [a > 0 for a in acts]
        O.tie_report()
        z = O.encoder_forward(p, wave, relu_override=relu_override, tie_eps=TIE_EPS)
        self.ties = O.tie_report()
        return z.permute(0, 2, 1)

    def recur(self, p, z, state):
        return recurrence(p, z, self.cell, self.layers, state, self.reverse)

    def logits(self, p, c, z, ext):
        """The K (B, 1+N, W) score tensors; criterion mode "reverse" flips c and z along time first."""
        if self.reverse:
            c, z = torch.flip(c, [1]), torch.flip(z, [1])
        return O.criterion_logits(p, c, z, ext, self.K)

    def score(self, p, c, z, ext):
        if self.reverse:
            c, z = torch.flip(c, [1]), torch.flip(z, [1])
        losses, acc = O.criterion_forward(p, c, z, ext, self.K)
        B, S, _ = z.shape
        return losses, torch.round(acc[0] * (B * (S - self.K))).long()

    def features(self, params, wave, state=None):
        """Forward only, no gradient: -> (z (B,S,C), c (B,S,H), final state)."""
        dt = self.dtype
        p = {k: v.detach().to(dt) for k, v in params.items()}
        if state is not None:
            state = tuple(s.detach().to(dt) for s in state) if isinstance(state, tuple) else state.detach().to(dt)
        with torch.no_grad(), torch.backends.mkldnn.flags(enabled=False):
            z = O.encoder_forward(p, wave.to(dt)).permute(0, 2, 1)
            c, last = self.recur(p, z, state)
        return z, c, last

    # -- the step -------------------------------------------------------------------------------------------------------------
    def step(self, params, wave, bi, si, state=None, relu_override=None, backward=True):
        """-> dict(z, c, state, losses (1,K), counts (K,), grads {key: d losses.sum() / d parameter}, report).  ``params``: a flat
        dict under the reference's keys (cast to ``dtype``, treated as leaves); ``state``: h0 / (h0, c0), no gradient."""
        dt = self.dtype
        leaves = {k: v.detach().to(dt).clone().requires_grad_(backward) for k, v in params.items()}
        if state is not None:
            state = tuple(s.detach().to(dt) for s in state) if isinstance(state, tuple) else state.detach().to(dt)
        with torch.backends.mkldnn.flags(enabled=False):
            z = self.encode(leaves, wave.to(dt), relu_override)
            c, last = self.recur(leaves, z, state)
            B, S, _ = z.shape
            ext = O.negative_rows(bi, si, B, S, S - self.K, self.N)
            losses, counts = self.score(leaves, c, z, ext)
            if backward:
                losses.sum().backward()
            with torch.no_grad():
                rep = score_report(self.logits(leaves, c, z, ext), ext, S)
        rep["near_zero"], rep["preactivations"] = self.ties["eligible"], self.ties["numel"]
        rep["ln_gap"] = [abs(l - math.log(self.N + 1)) for l in losses.detach()[0].tolist()]
        last = tuple(s.detach() for s in last) if isinstance(last, tuple) else last.detach()
        return {"z": z.detach(), "c": c.detach(), "state": last, "losses": losses.detach(), "counts": counts, "ext": ext,
                "grads": {k: v.grad for k, v in leaves.items()} if backward else None, "report": rep}


def well_posed(rep, allow_near_zero=False):
    """Conditions (a), (b), (c) on a Chain.step report (``allow_near_zero``: a ``device_relu`` row, which is held to O.tie_ok and
    ``disagree_outside == 0`` on the device instead of to (a))."""
    return (allow_near_zero or rep["near_zero"] == 0) and min(rep["margin"]) >= MARGIN_MIN and min(rep["ln_gap"]) >= LN_GAP_MIN


def adam_trajectory(chain, params, wave, bi, si, steps, lr=TRAINER_LR):
    """``steps`` float64 train steps with torch.optim.Adam(lr, (0.9, 0.999), 1e-8) on the chain's own gradients (the same wave and
    negatives every step) -> ([result of every step], parameters afterwards)."""
    cur = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(cur.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    results = []
    for _ in range(steps):
        r = chain.step({k: v.detach() for k, v in cur.items()}, wave, bi, si)
        for k, v in cur.items():
            v.grad = r["grads"][k]
        opt.step()
        results.append(r)
    return results, {k: v.detach() for k, v in cur.items()}


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()
