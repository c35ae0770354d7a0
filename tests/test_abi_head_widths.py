"""The feature-width option of the PER phone classifier and of the phone posteriors -- the C ABI's six new symbols and their
argument checks (which return before any launch; run on the host emulator's build of the same sources), the module surface and
the command lines.  No GPU needed."""
import ctypes

import pytest
import torch

import head_widths_util as U
import zerospeech_util as ZU
from emu_util import P, emu

NEW_SYMBOLS = ("cpc_phone_head_layout_d", "cpc_phone_head_forward_d", "cpc_phone_head_backward_d", "cpc_seqnorm_forward_d",
               "cpc_seqnorm_backward_d", "cpc_posterior_forward_d")
SHAPE, ARG = 1, 2            # CPC_ERR_SHAPE, CPC_ERR_ARG


def test_new_symbols_are_declared_and_the_abi_version_stays():
    from cpc_audio_amd import _lib
    lib = emu()
    assert lib.cpc_abi_version() == _lib.EXPECTED_ABI == 16
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    # the existing argument lists plus int D
    for name in NEW_SYMBOLS:
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-2]][1]) + 1, name


def test_widths_outside_1_to_512_are_refused_before_anything_else():
    lib = emu()
    sizes = (ctypes.c_long * 5)()
    x, W, b = torch.full((2 * 16 * 512,), 7.0), torch.full((7 * 512 * 8,), 7.0), torch.full((7,), 7.0)
    out = [torch.full((1 << 16,), 7.0) for _ in range(6)]
    hot = torch.full((64,), 7, dtype=torch.int64)
    lens = torch.tensor([16, 16])
    for D in (0, 513, -1):
        assert lib.cpc_phone_head_layout_d(2, 16, 7, 0, D, sizes) == SHAPE
        assert lib.cpc_phone_head_layout_d(2, 16, 7, 0, D, None) == SHAPE                       # the width is checked first
        assert lib.cpc_phone_head_forward_d(P(x), P(W), P(b), P(out[0]), P(out[1]), P(out[2]), 2, 16, 7, D, None) == SHAPE
        assert lib.cpc_phone_head_forward_d(None, P(W), P(b), P(out[0]), P(out[1]), P(out[2]), 2, 16, 7, D, None) == SHAPE
        assert lib.cpc_phone_head_backward_d(P(x), P(W), P(out[2]), P(out[1]), P(out[3]), P(out[4]), P(out[5]), 2, 16, 7, D,
                                             None) == SHAPE
        assert lib.cpc_seqnorm_forward_d(P(x), P(lens), None, P(out[0]), P(out[1]), 2, 16, D, 1, None) == SHAPE
        assert lib.cpc_seqnorm_forward_d(None, P(lens), None, P(out[0]), P(out[1]), 2, 16, D, 1, None) == SHAPE
        assert lib.cpc_seqnorm_backward_d(P(x), P(W), P(lens), None, P(out[1]), P(out[0]), 2, 16, D, 1, None) == SHAPE
        for mode, o in ((0, out[0]), (1, hot)):
            assert lib.cpc_posterior_forward_d(P(x), 512, P(W), P(b), 4, 7, D, mode, P(o), None, None) == SHAPE
        assert lib.cpc_posterior_forward_d(None, 512, P(W), P(b), 4, 7, D, 0, P(out[0]), None, None) == SHAPE
    # the other checks are those of the 256 calls
    assert lib.cpc_phone_head_layout_d(2, 7, 7, 0, 40, sizes) == SHAPE and lib.cpc_phone_head_layout_d(2, 16, 1, 0, 40, sizes) == SHAPE
    assert lib.cpc_phone_head_layout_d(2, 16, 7, 0, 40, None) == ARG
    assert lib.cpc_phone_head_forward_d(P(x), P(W), P(b), None, P(out[1]), P(out[2]), 2, 16, 7, 40, None) == ARG
    assert lib.cpc_seqnorm_forward_d(P(x), P(lens), None, P(x), P(out[1]), 2, 16, 40, 1, None) == ARG       # in place
    assert lib.cpc_seqnorm_forward_d(P(x), P(lens), None, P(out[0]), P(out[1]), 2, 16, 40, 2, None) == ARG
    assert lib.cpc_seqnorm_forward_d(P(x), P(lens), None, P(out[0]), P(out[1]), 1 << 12, 1 << 12, 512, 1, None) == SHAPE
    assert lib.cpc_posterior_forward_d(P(x), 39, P(W), P(b), 4, 7, 40, 0, P(out[0]), None, None) == ARG     # ldx < D
    assert lib.cpc_posterior_forward_d(P(x), 40, P(W), P(b), 4, 1, 40, 0, P(out[0]), None, None) == SHAPE
    # nothing was launched: no buffer was written
    for t in (x, W, b, hot, *out):
        assert bool((t == 7).all())
    assert lib.cpc_phone_head_layout_d(2, 16, 7, 0, 1, sizes) == 0 and lib.cpc_phone_head_layout_d(2, 16, 7, 0, 512, sizes) == 0


def test_head_layout_at_256_is_the_existing_one_and_follows_the_width():
    lib = emu()
    a, b = (ctypes.c_long * 5)(), (ctypes.c_long * 5)()
    for B, S, C, Lmax in [(1, 8, 2, 0), (2, 11, 7, 3), (8, 1500, 42, 40), (64, 128, 256, 512), (300, 8196, 42, 10)]:
        assert lib.cpc_phone_head_layout_d(B, S, C, Lmax, 256, a) == 0 and lib.cpc_phone_head_layout(B, S, C, Lmax, b) == 0
        assert tuple(a) == tuple(b), (B, S, C, Lmax)
    for bad in [(0, 8, 2, 0), (1, 7, 2, 0), (1, 8, 257, 0), (1, 8200, 2, 0), (1, 8, 2, 513), (1 << 13, 8196, 256, 0)]:
        assert lib.cpc_phone_head_layout_d(*bad, 256, a) == lib.cpc_phone_head_layout(*bad, b) != 0, bad
        assert lib.cpc_phone_head_layout_d(*bad, 40, a) != 0, bad
    assert lib.cpc_phone_head_layout_d(2, 37, 41, 0, 40, a) == 0 and lib.cpc_phone_head_layout(2, 37, 41, 0, b) == 0
    assert a[0] == b[0] and a[1] == 41 * 8 * 40 and a[3] == b[3] and a[4] == b[4] and a[2] <= b[2]
    assert lib.cpc_phone_head_layout_d(2, 37, 41, 0, 512, a) == 0 and a[1] == 41 * 8 * 512


def test_keyword_defaults_attributes_and_state_dict():
    from cpc_audio_amd import common_voices_eval as CV
    from cpc_audio_amd.harness import ModelPhoneCombined
    plain, wide = CV.CTCphone_criterion(40, 6, True), CV.CTCphone_criterion(40, 6, True, wideKernel=True)
    assert plain.wideKernel is False and wide.wideKernel is True
    assert plain._hipConfig is False and plain._hipFrontConfig is False and wide._hipConfig is True and wide._hipFrontConfig is True
    assert wide.hipHead is None and wide.hipFront is None
    assert wide.last_path is None and wide.last_front is None and wide.last_lstm is None and plain.last_lstm is None
    assert list(plain.state_dict()) == list(wide.state_dict())
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == {k: tuple(v.shape) for k, v in wide.state_dict().items()}
    wide.load_state_dict(plain.state_dict(), strict=True)
    for dim in (1, 13, 512):
        c = CV.CTCphone_criterion(dim, 6, hipHead=True, hipFront=True, wideKernel=True)
        assert c._hipConfig and c._hipFrontConfig
    at256 = CV.CTCphone_criterion(256, 6, wideKernel=True)
    assert at256._hipConfig and at256._hipFrontConfig
    assert CV.CTCphone_criterion(40, 6, sizeKernel=4, wideKernel=True)._hipConfig is False      # sizeKernel must still be 8
    m = ModelPhoneCombined(ZU.Features(), torch.nn.Identity(), False)
    assert m.wideKernel is False and ModelPhoneCombined(ZU.Features(), torch.nn.Identity(), False, None, True).wideKernel is True


def test_refusals_stay_and_name_the_new_range():
    from cpc_audio_amd import common_voices_eval as CV
    with pytest.raises(NotImplementedError, match="dimEncoder 256"):
        CV.CTCphone_criterion(16, 6, hipHead=True)
    with pytest.raises(NotImplementedError, match="dimEncoder 256"):
        CV.CTCphone_criterion(16, 6, hipFront=True)
    CV.CTCphone_criterion(16, 6, hipHead=True, hipFront=True, wideKernel=True)
    for kw in (dict(hipHead=True), dict(hipFront=True)):
        with pytest.raises(NotImplementedError, match="1 <= dimEncoder <= 512"):
            CV.CTCphone_criterion(513, 6, wideKernel=True, **kw)
        with pytest.raises(NotImplementedError, match="1 <= dimEncoder <= 512"):
            CV.CTCphone_criterion(0, 6, wideKernel=True, **kw)
    with pytest.raises(NotImplementedError, match="sizeKernel 8"):
        CV.CTCphone_criterion(40, 6, sizeKernel=4, hipHead=True, wideKernel=True)


@pytest.mark.parametrize("lstm", [False, True])
def test_cpu_input_runs_the_torch_path(lstm):
    from cpc_audio_amd import common_voices_eval as CV
    torch.manual_seed(3)
    off = CV.CTCphone_criterion(40, 6, lstm, seqNorm=True, hipHead=False, hipFront=False).eval()
    auto = CV.CTCphone_criterion(40, 6, lstm, seqNorm=True, wideKernel=True).eval()
    auto.load_state_dict(off.state_dict())
    x = torch.randn(2, 24, 40)
    sizes, label, label_size = torch.tensor([24, 17]), torch.tensor([[1, 2, 3], [4, 0, 0]]), torch.tensor([3, 1])
    assert torch.equal(auto(x, sizes, label, label_size), off(x, sizes, label, label_size))
    assert auto.last_path == "torch" and auto.last_front == "torch" and auto.last_lstm == ("torch" if lstm else None)
    assert torch.equal(auto.getPrediction(x, sizes), off.getPrediction(x, sizes))
    for kw in (dict(hipHead=True), dict(hipFront=True)):
        hip = CV.CTCphone_criterion(40, 6, lstm, seqNorm=True, wideKernel=True, **kw)
        with pytest.raises(NotImplementedError):
            hip(x, sizes, label, label_size)
        with pytest.raises(NotImplementedError):
            hip.getPrediction(x, sizes)


def test_ops_check_widths():
    from cpc_audio_amd import ops
    with pytest.raises((NotImplementedError, RuntimeError), match="256|no CPU path"):
        ops.posterior(torch.zeros(4, 128), torch.zeros(41, 128), torch.zeros(41))
    with pytest.raises(ValueError, match="weight"):
        ops.posterior(torch.zeros(4, 40), torch.zeros(41, 64), torch.zeros(41), wide=True)
    with pytest.raises(ValueError, match="weight"):
        ops.phone_head_logits(torch.zeros(1, 8, 40), torch.zeros(7, 64, 8), torch.zeros(7))
    with pytest.raises(ValueError, match="weight"):
        ops.PhoneHeadCtcFunction.apply(torch.zeros(1, 8, 40), torch.zeros(7, 64, 8), torch.zeros(7), torch.ones(1, dtype=torch.long),
                                       torch.zeros(1, 1, dtype=torch.long), torch.ones(1, dtype=torch.long), 6, "sum")
    with pytest.raises(NotImplementedError, match="512"):
        ops.phone_head_logits(torch.zeros(1, 8, 513), torch.zeros(7, 513, 8), torch.zeros(7))
    with pytest.raises(ValueError, match="scale"):
        ops.SeqNormFunction.apply(torch.zeros(1, 8, 40), None, torch.zeros(1, 64), True)
    with pytest.raises(NotImplementedError, match="512"):
        ops.SeqNormFunction.apply(torch.zeros(1, 8, 513), None, None, True)
    with pytest.raises(NotImplementedError, match="512"):
        ops.phone_head_layout(1, 8, 7, 0, 513)
    assert ops.phone_head_supported(1, 8, 7, 0, 513) is False and ops.phone_head_supported(1, 8, 7, 0, 0) is False
    assert ops.seqnorm_supported(2, 8, 40) and ops.seqnorm_supported(2, 8) and not ops.seqnorm_supported(2, 8, 513)
    assert not ops.seqnorm_supported(2, 8, 0) and not ops.seqnorm_supported(1 << 12, 1 << 12, 512)
    assert ops.PHONE_HEAD_MAX_DIM == 512


def test_command_line_options():
    from cpc_audio_amd import build_zeroSpeech_features as BZ, common_voices_eval as CV
    argv = ["train", "/data/db", "/data/phones.txt", "/ckpt/checkpoint_30.pt"]
    assert "wideKernel" not in vars(CV.parse_args(argv)) and CV.parse_args(argv + ["--wideKernel"]).wideKernel is True
    assert "wideKernel" not in vars(CV.parse_args(["per", "/out"]))
    base = ZU.ARGV["defaults"]
    assert "wideKernel" not in vars(BZ.parse_args(base)) and BZ.parse_args(base + ["--wideKernel"]).wideKernel is True


def test_per_reads_the_option_back(tmp_path):
    import json
    from cpc_audio_amd import common_voices_eval as CV
    saved = dict(pathDB="/db", file_extension=".wav", pathPhone="/p", pathVal="/v", pathCheckpoint="ID", no_pretraining=False)
    for extra, want in (({}, False), ({"wideKernel": True}, True)):
        with open(tmp_path / "args_training.json", "w") as f:
            json.dump({**saved, **extra}, f)
        args = CV.get_PER_args(CV.parse_args(["per", str(tmp_path)]))
        assert getattr(args, "wideKernel", False) is want and ("wideKernel" in vars(args)) is want
