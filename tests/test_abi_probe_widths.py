"""The feature-width option of the supervised criteria and of the fused probe step -- module surface, the C ABI's new symbols and
their argument checks (which return before any launch; run on the host emulator's build of the same sources) and the command
line.  No GPU needed."""
import ctypes

import pytest
import torch
import torch.nn as nn

import probe_widths_util as U
from emu_util import P, emu

NEW_SYMBOLS = ("cpc_probe_layout_d", "cpc_probe_train_step_d", "cpc_probe_eval_d", "cpc_supervised_layout_d",
               "cpc_classifier_forward_d", "cpc_classifier_backward_d", "cpc_ctc_forward_d")


def _criteria(dim, **kw):
    from cpc_audio_amd.criterion import CTCPhoneCriterion, PhoneCriterion, SpeakerCriterion
    return SpeakerCriterion(dim, 12, **kw), PhoneCriterion(dim, 41, False, **kw), CTCPhoneCriterion(dim, 41, False, **kw)


def test_keyword_and_attributes():
    from cpc_audio_amd.criterion import PhoneCriterion
    for dim in (13, 40, 512):
        for crit in _criteria(dim, wideKernel=True):
            assert crit.hip_wide is True and crit.hip_path is False, (dim, type(crit).__name__)
    for crit in _criteria(513, wideKernel=True):
        assert crit.hip_wide is False and crit.hip_path is False
    for crit in _criteria(256, wideKernel=True):                      # 256 stays on the existing path, with or without the keyword
        assert crit.hip_wide is False and crit.hip_path is True
    nl2 = PhoneCriterion(40, 41, False, nLayers=2, wideKernel=True)
    assert nl2.hip_wide is False and nl2.hip_path is False
    nl2 = PhoneCriterion(40, 41, False, 2, True)                      # positional: behind nLayers
    assert nl2.hip_wide is False and isinstance(nl2.PhoneCriterionClassifier, nn.Sequential)


def test_defaults_are_unchanged():
    for dim in (13, 40, 512, 513):
        for crit in _criteria(dim):
            assert crit.hip_wide is False and crit.hip_path is False
    for crit in _criteria(256):
        assert crit.hip_wide is False and crit.hip_path is True
    plain, wide = _criteria(40), _criteria(40, wideKernel=True)
    for a, b in zip(plain, wide):                                     # state-dict keys and shapes do not depend on the keyword
        assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}
        assert list(a.state_dict()) == list(b.state_dict())


@pytest.mark.parametrize("dim", [13, 40, 512])
def test_cpu_input_runs_the_modules_torch_ops(dim):
    """As CPCAR(inputKernel=True) does for CPU input: torch.equal to plain nn.Linear + nn.CrossEntropyLoss / nn.CTCLoss."""
    from cpc_audio_amd.criterion import collapse_label_chain
    torch.manual_seed(dim)
    spk, phone, ctc = _criteria(dim, wideKernel=True)
    B, S = 3, 8
    c = torch.randn(B, S, dim)
    y_spk = torch.randint(0, 12, (B,))
    y_ph = torch.randint(0, 41, (B, S // 2)).repeat_interleave(2, dim=1)
    loss, acc = spk(c, c, y_spk)
    logits = spk.linearSpeakerClassifier(c[:, -1, :])
    assert torch.equal(loss, nn.CrossEntropyLoss()(logits, y_spk).view(1, 1))
    assert torch.equal(acc, (logits.max(1)[1] == y_spk).double().mean().view(1, 1))
    loss, acc = phone(c, c, y_ph)
    logits = phone.PhoneCriterionClassifier(c.reshape(B * S, dim))
    assert torch.equal(loss, nn.CrossEntropyLoss()(logits, y_ph.reshape(-1)).view(1, 1))
    assert torch.equal(acc, (logits.max(1)[1] == y_ph.reshape(-1)).double().mean().view(1, 1))
    loss, zero = ctc(c, c, y_ph)
    lp = torch.nn.functional.log_softmax(ctc.PhoneCriterionClassifier(c.reshape(B * S, dim)).view(B, S, -1), dim=2).permute(1, 0, 2)
    targets, sizes = collapse_label_chain(y_ph)
    ref = nn.CTCLoss(blank=41, zero_infinity=True)(lp, targets, torch.full((B,), S, dtype=torch.int64), sizes)
    assert torch.equal(loss, ref.view(1, 1)) and float(zero) == 0
    assert loss.requires_grad


def test_new_symbols_are_bound_at_abi_version_16():
    from cpc_audio_amd import _lib
    assert _lib.EXPECTED_ABI == 16
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
    assert "cpc_ctc_backward_d" not in _lib.SIGNATURES                # what it reads of ``saved`` does not depend on D
    lib = emu()
    assert lib.cpc_abi_version() == 16
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name


def test_layouts_at_256_are_the_existing_ones():
    lib = emu()
    a, b = (ctypes.c_long * 3)(), (ctypes.c_long * 3)()
    for R, C in [(1, 2), (33, 41), (70, 65), (8, 251), (1024, 41), (200, 4100), (8300, 5), (262143, 8192)]:
        assert lib.cpc_probe_layout_d(R, C, 256, a) == 0 and lib.cpc_probe_layout(R, C, b) == 0
        assert tuple(a) == tuple(b), (R, C)
    for Bq, S, C, ctc in [(8, 1, 12, 0), (8, 128, 41, 0), (4, 128, 42, 1), (4, 512, 42, 1), (64, 128, 8192, 0), (700, 1, 300, 0)]:
        assert lib.cpc_supervised_layout_d(Bq, S, C, 256, ctc, a) == 0 and lib.cpc_supervised_layout(Bq, S, C, ctc, b) == 0
        assert tuple(a) == tuple(b), (Bq, S, C, ctc)
    # the shape limits of the 256 calls are those of the _d calls
    for bad in [(0, 41), (4, 1), (4, 8193), (1 << 20, 4096)]:
        assert lib.cpc_probe_layout_d(*bad, 40, a) == 1, bad
    assert lib.cpc_supervised_layout_d(4, 513, 42, 40, 1, a) == 1 and lib.cpc_supervised_layout_d(4, 512, 42, 40, 1, a) == 0
    # the partials follow D: narrower rows, a smaller workspace
    assert lib.cpc_probe_layout_d(70, 65, 40, a) == 0 and lib.cpc_probe_layout(70, 65, b) == 0 and a[0] < b[0]
    assert lib.cpc_probe_layout_d(100000, 8192, 512, a) == 0 and 1 <= a[1] <= 256


def test_arguments_are_checked_before_any_launch():
    lib = emu()
    sizes = (ctypes.c_long * 3)()
    for D in (0, 513, -1):
        assert lib.cpc_probe_layout_d(4, 41, D, sizes) == 1 and lib.cpc_supervised_layout_d(4, 1, 41, D, 0, sizes) == 1, D
    assert lib.cpc_probe_layout_d(4, 41, 40, None) == 2 and lib.cpc_supervised_layout_d(4, 1, 41, 40, 0, None) == 2
    assert lib.cpc_supervised_layout_d(4, 1, 41, 40, 2, sizes) == 2
    assert lib.cpc_probe_layout_d(4, 41, 512, sizes) == 0 and lib.cpc_probe_layout_d(4, 41, 1, sizes) == 0
    D = 40
    case = U.Case(D, 4, 41, seed=1)
    W, b = case.W.clone(), case.b.clone()
    m = [t.clone() for t in case.moments]
    ws, loss = torch.full((8192,), 7.0), torch.full((1,), 7.0)
    acc = torch.zeros(1, dtype=torch.float64)
    bc1, bc2s = U.bias_corrections(1)

    def train(x_=P(case.base), ldx=D, y_=P(case.y), R=4, C=41, D_=D, W_=P(W), b_=P(b), m_=P(m[0]), ws_=P(ws), loss_=P(loss), acc_=P(acc),
              bc1_=bc1):
        return lib.cpc_probe_train_step_d(x_, ldx, y_, R, C, D_, W_, b_, m_, P(m[1]), P(m[2]), P(m[3]), U.LR, U.BETA1, U.BETA2, U.EPS,
                                          bc1_, bc2s, ws_, loss_, acc_, None, None, None, None)

    def evaluate(x_=P(case.base), ldx=D, y_=P(case.y), R=4, C=41, D_=D, W_=P(W), b_=P(b), ws_=P(ws), loss_=P(loss), acc_=P(acc)):
        return lib.cpc_probe_eval_d(x_, ldx, y_, R, C, D_, W_, b_, ws_, loss_, acc_, None, None)

    for call in (train, evaluate):
        assert call(D_=0) == 1 and call(D_=513) == 1 and call(C=1) == 1 and call(C=8193) == 1 and call(R=0) == 1
        assert call(D_=513, x_=None) == 1                            # the width is checked first
        assert call(ldx=D - 1) == 2
        for null in ("x_", "y_", "W_", "b_", "ws_", "loss_", "acc_"):
            assert call(**{null: None}) == 2, null
        assert call(ws_=P(ws) + 4) == 2                              # a workspace that is not 16-byte aligned
    assert train(m_=None) == 2 and train(bc1_=0.0) == 2
    # the classifier and the CTC criterion
    saved, dW = torch.full((8192,), 7.0), torch.full((41 * D,), 7.0)

    def forward(x_=P(case.base), ldx=D, W_=P(W), b_=P(b), y_=P(case.y), saved_=P(saved), loss_=P(loss), acc_=P(acc), D_=D):
        return lib.cpc_classifier_forward_d(x_, ldx, W_, b_, y_, saved_, loss_, acc_, 4, 41, D_, None)

    assert forward(D_=0) == 1 and forward(D_=513) == 1 and forward(ldx=D - 1) == 2
    for null in ("x_", "W_", "b_", "y_", "saved_", "loss_", "acc_"):
        assert forward(**{null: None}) == 2, null

    def backward(x_=P(case.base), ldx=D, W_=P(W), dl_=P(saved), scr_=P(ws), dW_=P(dW), db_=P(loss), D_=D):
        return lib.cpc_classifier_backward_d(x_, ldx, W_, None, None, None, dl_, scr_, dW_, db_, None, 4, 41, D_, None)

    assert backward(D_=0) == 1 and backward(D_=513) == 1 and backward(ldx=D - 1) == 2
    for null in ("x_", "W_", "dl_", "scr_", "dW_", "db_"):               # (dl_: neither dlogits nor what makes them)
        assert backward(**{null: None}) == 2, null

    def ctc(x_=P(case.base), W_=P(W), b_=P(b), y_=P(case.y), saved_=P(saved), loss_=P(loss), S=4, D_=D):
        return lib.cpc_ctc_forward_d(x_, W_, b_, y_, saved_, loss_, 1, S, 41, D_, None)

    assert ctc(D_=0) == 1 and ctc(D_=513) == 1 and ctc(S=513) == 1
    for null in ("x_", "W_", "b_", "y_", "saved_", "loss_"):
        assert ctc(**{null: None}) == 2, null
    # nothing was launched: no buffer was written
    for t, v in ((ws, 7.0), (loss, 7.0), (saved, 7.0), (dW, 7.0)):
        assert bool((t == v).all())
    assert torch.equal(W, case.W) and torch.equal(b, case.b) and all(torch.equal(a, c) for a, c in zip(m, case.moments))
    # a D = 512 call with valid sizes passes the layout and runs
    wide = U.Case(512, 4, 41, seed=2)
    out = U.train(lib, wide)
    assert torch.isfinite(out["loss"][0]) and not torch.equal(out["W"][:41 * 512], wide.W.reshape(-1))
    U.check_canaries(out, 41, 512)


def test_ops_refuse_a_width_mismatch_and_posterior_stays_at_256():
    from cpc_audio_amd import ops
    x, y = torch.zeros(4, 40), torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError, match="weight"):
        ops.ClassifierXentFunction.apply(x, y, torch.zeros(41, 64), torch.zeros(41))
    with pytest.raises(ValueError, match="weight"):
        ops.CtcXentFunction.apply(torch.zeros(1, 4, 40), torch.zeros(1, 4, dtype=torch.long), torch.zeros(42, 64), torch.zeros(42))
    with pytest.raises(ValueError, match="weight"):
        ops.probe_eval(x, y, torch.zeros(41, 64), torch.zeros(41))
    with pytest.raises(ValueError, match="weight"):
        ops.probe_train_step(x, y, torch.zeros(41, 64), torch.zeros(41), None)
    with pytest.raises((NotImplementedError, RuntimeError), match="256|no CPU path"):
        ops.posterior(torch.zeros(4, 128), torch.zeros(41, 128), torch.zeros(41))
    assert ops.CLASSIFIER_MAX_DIM == 512


def test_command_line_option():
    from cpc_audio_amd import linear_separability as LS
    argv = ["/data/db", "/data/train.txt", "/data/val.txt", "/ckpt/checkpoint_30.pt"]
    # off by default -- and then not in the namespace at all, so that the reference's argument lists still parse to the
    # reference's namespace (tests/test_linsep_cpu.py), which is what main() writes to checkpoint_args.json
    assert getattr(LS.parse_args(argv), "wideKernel", False) is False and "wideKernel" not in vars(LS.parse_args(argv))
    assert LS.parse_args(argv + ["--wideKernel"]).wideKernel is True
    # the fused step takes a wide criterion on a frozen feature maker, and only with the option
    import linsep_util as LU
    from cpc_audio_amd.criterion import CTCPhoneCriterion, PhoneCriterion, SpeakerCriterion
    fm = LU.PassThrough()
    assert LS._probe_of(fm, PhoneCriterion(40, 41, False, wideKernel=True))[1] == "phone"
    assert LS._probe_of(fm, SpeakerCriterion(13, 12, wideKernel=True))[1] == "speaker"
    assert LS._probe_of(fm, PhoneCriterion(40, 41, False)) is None and LS._probe_of(fm, SpeakerCriterion(13, 12)) is None
    assert LS._probe_of(fm, CTCPhoneCriterion(40, 41, False, wideKernel=True)) is None
    assert LS._probe_of(fm, PhoneCriterion(256, 41, False))[1] == "phone"
