"""Inputs of the supervised-criterion fixture (tests/golden/supervised.npz, written by tools/make_golden_supervised.py from the
reference's classes) -- seeded, so the fixture holds outputs only."""
import torch

B, S, N_PHONES, N_SPEAKERS = 4, 128, 41, 12

# name -> (class name, constructor args, feature width)
CASES = {
    "speaker": ("SpeakerCriterion", (256, N_SPEAKERS), 256),
    "phone": ("PhoneCriterion", (256, N_PHONES, False), 256),
    "phone_enc": ("PhoneCriterion", (256, N_PHONES, True), 256),
    "phone_nl2": ("PhoneCriterion", (256, N_PHONES, False, 2), 256),
    "phone_w128": ("PhoneCriterion", (128, N_PHONES, False), 128),
    "ctc": ("CTCPhoneCriterion", (256, N_PHONES, False), 256),
    "ctc_w128": ("CTCPhoneCriterion", (128, N_PHONES, False), 128),
}


FULL_GRADS = ("speaker", "phone", "ctc")
FLOAT64_CASES = ("ctc",)                       # run by the reference in float64 for the fixture (its fp32 CTC rounds ~1e-4)        # cases whose weight gradients the fixture holds in full (the rest: projected)


def frame_labels(n_phones=N_PHONES, b=B, s=S, seed=5):
    """(b, s) int64 phone labels: runs of varied length (single frames and long runs), long runs only, every frame different
    from the one before (nothing collapses: L = s), random runs."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(b, s, dtype=torch.int64)
    for i in range(b):
        kind = i % 4
        t, row = 0, []
        while len(row) < s:
            if kind == 0:
                n = [1, 1, 7, 1, 23, 2, 1, 3][t % 8]
            elif kind == 1:
                n = 20 + int(torch.randint(0, 20, (1,), generator=g))
            elif kind == 2:
                n = 1
            else:
                n = 1 + int(torch.randint(0, 6, (1,), generator=g))
            v = (t * 7 + i) % n_phones if kind == 2 else int(torch.randint(0, n_phones, (1,), generator=g))
            if row and v == row[-1]:
                v = (v + 1) % n_phones
            row += [v] * n
            t += 1
        out[i] = torch.tensor(row[:s])
    return out


def speaker_labels(n_speakers=N_SPEAKERS, b=B, seed=6):
    return torch.randint(0, n_speakers, (b,), generator=torch.Generator().manual_seed(seed))


def features(dim, seed):
    """(cFeature, encodedData), each (B, S, dim)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, dim, generator=g), torch.randn(B, S, dim, generator=g)


def seeded_state(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: 0.1 * torch.randn(*s, generator=g) for k, s in shapes.items()}


def projection(dim, k=4):
    """Seeded (dim, k) directions: the fixture stores feature gradients projected on them (B * S * k floats, not B * S * dim)
    and the weight gradients of the cases outside FULL_GRADS likewise."""
    return torch.randn(dim, k, generator=torch.Generator().manual_seed(1000 + dim))


def run(crit, name, c, enc, plabels, slabels):
    """Loss, accuracy and gradients of one criterion (its parameters already loaded)."""
    cr, er = c.clone().requires_grad_(True), enc.clone().requires_grad_(True)
    label = slabels if name == "speaker" else plabels
    loss, acc = crit(cr, er, label)
    loss.sum().backward()
    grads = {k: p.grad for k, p in crit.named_parameters()}
    return loss.detach(), acc.detach(), grads, cr.grad, er.grad
