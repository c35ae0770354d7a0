"""The CPC criterion at encoder / context widths other than 256 and with a speaker embedding, on an MI355X (csrc/nce_wide.hip
through ops.nce_wide_scores and criterion.CPCUnsupersivedCriterion): the reference's stored results
(tests/golden/criterion_widths.npz), the module against oracle.cpc_oracle.criterion_forward in float64 on the CPU, the other
prediction networks and options at a non-256 width, and the MFCC / filter-bank encoders trained end to end.

Bar (tests/test_gpu_predictors.py, tests/test_gpu_recurrent_predictors.py): relative error below 1e-4 against float64 on the CPU;
accuracies are counts and must agree."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4


@pytest.fixture(autouse=True)
def _no_device_errors():
    yield
    if torch.cuda.is_available():
        from cpc_audio_amd import ops
        ops.check_device_errors()                       # raises on any flagged device error


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _oracle(crit, c, z, label, negatives, gl):
    """The criterion module's own prediction networks (a float64 copy on the CPU) scored by oracle.cpc_oracle.criterion_forward on
    the given draws -> losses (1, K), acc (1, K), d c, d z, {parameter name: gradient} of (losses * gl).sum().  ``c is z`` (no
    autoregressive network): one leaf, whose gradient is returned twice."""
    ref = copy.deepcopy(crit).cpu().double().eval()
    ref.zero_grad()
    zr = z.detach().cpu().double().requires_grad_(True)
    cr = zr if c is z else c.detach().cpu().double().requires_grad_(True)
    cc, zz = cr, zr
    if crit.mode == "reverse":
        cc, zz = torch.flip(cc, [1]), torch.flip(zz, [1])
    B, S, _ = zz.shape
    K, N = crit.nPredicts, crit.negativeSamplingExt
    W = S - K
    if ref.speakerEmb is not None:
        cc = torch.cat([cc, ref.speakerEmb(label.cpu().view(B, 1).expand(B, S))], dim=2)
    rows = O.negative_rows(negatives[0].cpu(), negatives[1].cpu(), B, S, W, N)

    def predict(k, cw):
        out = ref.wPrediction.predictors[k](cw)
        return out[0] if isinstance(out, tuple) else out

    losses, acc = O.criterion_forward({}, cc, zz, rows, K, predict)
    (losses * gl.detach().cpu().double()).sum().backward()
    return losses.detach(), acc.detach(), cr.grad, zr.grad, {n: p.grad for n, p in ref.named_parameters()}


def _check(crit, c, z, label, negatives, gl, twice=False):
    """One forward + backward of ``crit`` on the device against _oracle; c and z are leaves here."""
    c = c.detach().clone().requires_grad_(True)
    z = z.detach().clone().requires_grad_(True)
    crit.zero_grad()
    losses, acc = crit(c, z, label, negatives=negatives)
    K = crit.nPredicts
    assert tuple(losses.shape) == (1, K) and tuple(acc.shape) == (1, K)
    (losses * gl).sum().backward()
    want = _oracle(crit, c, z, label, negatives, gl)
    assert bool(((losses.detach().cpu().double() - want[0]).abs() <= BAR * want[0].abs().clamp_min(1.0)).all()), (losses, want[0])
    assert (acc.cpu().double() - want[1].double()).abs().max().item() < 1e-6, (acc, want[1])
    assert rel_err(c.grad, want[2]) < BAR and rel_err(z.grad, want[3]) < BAR
    grads = {n: p.grad.detach().clone() for n, p in crit.named_parameters()}
    assert set(grads) == set(want[4])
    for n, g in grads.items():
        assert rel_err(g, want[4][n]) < BAR, n
    if twice:                                           # bit-reproducible: no float atomics anywhere on the way
        c2, z2 = c.detach().clone().requires_grad_(True), z.detach().clone().requires_grad_(True)
        crit.zero_grad()
        l2, a2 = crit(c2, z2, label, negatives=negatives)
        (l2 * gl).sum().backward()
        assert torch.equal(l2, losses) and torch.equal(a2, acc) and torch.equal(c2.grad, c.grad) and torch.equal(z2.grad, z.grad)
        for n, p in crit.named_parameters():
            assert torch.equal(p.grad, grads[n]), n
    return losses, acc


def _case(dev, B, S, H, C, K, N, seed, speakers=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.tanh(torch.randn(B, S, H, generator=g)).to(dev)
    z = torch.relu(torch.randn(B, S, C, generator=g)).to(dev)
    label = torch.randint(0, max(speakers, 1), (B,), generator=g).to(dev)
    bi, si = O.draw_negative_indices(B, S, S - K, N, generator=g)
    gl = torch.randn(1, K, generator=g).to(dev)
    return c, z, label, (bi.to(dev), si.to(dev)), gl


@pytest.mark.parametrize("tag", ["h24c40", "h32c72", "spk"])
def test_the_reference_s_stored_results(tag):
    """tools/make_golden_criterion_widths.py: the reference's CPCUnsupersivedCriterion at (H, C, E) = (24, 40, 0), (32, 72, 0)
    and (16, 16, 8) with its own negative draws."""
    dev = _dev()
    from cpc_audio_amd.criterion import CPCUnsupersivedCriterion
    with open(os.path.join(GOLDEN, "criterion_widths_meta.json")) as f:
        meta = json.load(f)
    cs = meta["cases"][tag]
    with np.load(os.path.join(GOLDEN, "criterion_widths.npz")) as f:
        a = {k[len(tag) + 1:]: torch.from_numpy(f[k]) for k in f.files if k.startswith(tag + "_")}
    crit = CPCUnsupersivedCriterion(meta["K"], cs["H"], cs["C"], meta["N"], speakerEmbedding=cs["E"], nSpeakers=cs["speakers"],
                                    sizeInputSeq=meta["S"])
    crit.load_state_dict({k: a["param_" + k] for k in cs["keys"]}, strict=True)
    crit = crit.to(dev)
    c = a["c"].to(dev).requires_grad_(True)
    z = a["z"].to(dev).requires_grad_(True)
    losses, acc = crit(c, z, a["label"].to(dev), negatives=(a["batchIdx"].to(dev), a["seqIdx"].to(dev)))
    (losses * a["gloss"].to(dev)).sum().backward()
    assert bool(((losses.cpu() - a["losses"]).abs() <= BAR * a["losses"].abs().clamp_min(1.0)).all()), (losses, a["losses"])
    assert (acc.cpu() - a["acc"]).abs().max().item() < 1e-6
    assert rel_err(c.grad, a["dc"]) < BAR and rel_err(z.grad, a["dz"]) < BAR
    for k in cs["keys"]:
        assert rel_err(dict(crit.named_parameters())[k].grad, a["grad_" + k]) < BAR, k


@pytest.mark.parametrize("H,C,E", [(256, 40, 0), (64, 128, 0), (512, 512, 0), (256, 256, 16)])
def test_module_against_the_oracle_in_float64(H, C, E):
    dev = _dev()
    from cpc_audio_amd.criterion import CPCUnsupersivedCriterion
    B, S, K, N = 3, 24, 12, 24
    torch.manual_seed(H + C + E)
    crit = CPCUnsupersivedCriterion(K, H, C, N, speakerEmbedding=E, nSpeakers=4 if E else 0, sizeInputSeq=S).to(dev)
    assert crit.wPrediction.scores_apart
    c, z, label, neg, gl = _case(dev, B, S, H, C, K, N, seed=H + C, speakers=4 if E else 0)
    _check(crit, c, z, label, neg, gl, twice=True)


@pytest.mark.parametrize("kw", [dict(mode="reverse"), dict(dropout=True), dict(rnnMode="ffd"), dict(nPredicts=18)],
                         ids=["reverse", "dropout_eval", "ffd", "18_heads"])
def test_options_at_64_to_128(kw):
    """mode="reverse", the reference's dropout in eval mode (the identity), the ffd prediction networks on their torch modules,
    and more than 16 heads walked in groups -- the same module's predictions scored by the oracle."""
    dev = _dev()
    from cpc_audio_amd.train import build_criterion
    H, C, B, N = 64, 128, 3, 24
    K = kw.get("nPredicts", 12)
    S = 24 if K == 12 else 28
    torch.manual_seed(3)
    crit = build_criterion(hiddenGar=H, hiddenEncoder=C, negativeSamplingExt=N, sizeWindow=S * 160, **{"nPredicts": K, **kw}).to(dev)
    crit.eval()
    c, z, label, neg, gl = _case(dev, B, S, H, C, K, N, seed=17)
    _check(crit, c, z, label, neg, gl)


@pytest.mark.parametrize("enc", ["mfcc", "lfb"])
def test_encoders_of_other_widths_train_end_to_end(enc):
    """build_model + build_criterion at the encoder's width, one forward and backward at B = 2, L = 4000, against the oracle
    criterion evaluated on that model's own c and z."""
    dev = _dev()
    from cpc_audio_amd import ops, train
    torch.manual_seed(11)
    K, N, B, L = 5, 16, 2, 4000
    if enc == "mfcc":
        m = train.build_model(encoder_type="mfcc", hiddenEncoder=40, mfccKernel=True).to(dev)
        crit = train.build_criterion(hiddenEncoder=40, nPredicts=K, negativeSamplingExt=N, sizeWindow=L).to(dev)
    else:
        m = train.build_model(encoder_type="lfb", hiddenEncoder=64, arMode="no_ar").to(dev)
        crit = train.build_criterion(hiddenGar=64, hiddenEncoder=64, nPredicts=K, negativeSamplingExt=N, sizeWindow=L).to(dev)
    wave = (0.1 * torch.randn(B, 1, L, generator=torch.Generator().manual_seed(5))).clamp_(-1, 1).to(dev)
    assert train.CompositeStep(m, crit, ops.StepContext(), None).ok(wave) is False
    c, z, _ = m(wave, None)
    S = z.shape[1]
    assert S > K and z.shape[2] == crit.wPrediction.dimOutputEncoder
    bi, si = O.draw_negative_indices(B, S, S - K, N, generator=torch.Generator().manual_seed(9))
    neg = (bi.to(dev), si.to(dev))
    gl = torch.ones(1, K, device=dev)
    for t in {id(c): c, id(z): z}.values():
        if t.requires_grad:
            t.retain_grad()
    losses, acc = crit(c, z, None, negatives=neg)
    losses.sum().backward()
    want = _oracle(crit, c, z, None, neg, gl)
    assert bool(((losses.detach().cpu().double() - want[0]).abs() <= BAR * want[0].abs().clamp_min(1.0)).all()), (losses, want[0])
    assert (acc.cpu().double() - want[1].double()).abs().max().item() < 1e-6
    for n, p in crit.named_parameters():
        assert rel_err(p.grad, want[4][n]) < BAR, n
    if c.requires_grad:
        assert rel_err(c.grad, want[2]) < BAR                     # (no_ar: c is z, the one leaf carries both gradients)
    params = list(m.parameters()) + list(crit.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)


def test_train_epoch_with_the_mfcc_configuration():
    """Two steps of harness.train_epoch: CompositeStep.ok() is False for these widths, so this is the autograd path."""
    dev = _dev()
    from cpc_audio_amd import harness as H, train
    torch.manual_seed(2)
    K = 5
    m = train.build_model(encoder_type="mfcc", hiddenEncoder=40, mfccKernel=True).to(dev)
    crit = train.build_criterion(hiddenEncoder=40, nPredicts=K, negativeSamplingExt=16, sizeWindow=4000).to(dev)
    opt = torch.optim.Adam(list(crit.parameters()) + list(m.parameters()), lr=2e-4)
    before = [p.detach().clone() for p in crit.parameters()]
    logs = H.train_epoch(H.SyntheticLoader(2, 2, 4000, seed=3, device=dev), m, crit, opt)
    assert logs["iter"] == 2
    for key in ("locLoss_train", "locAcc_train"):
        v = np.asarray(logs[key]).reshape(1, -1)
        assert v.shape == (1, K) and np.isfinite(v).all()
    assert any(not torch.equal(p.detach(), q) for p, q in zip(crit.parameters(), before))
