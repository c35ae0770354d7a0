"""CPCUnsupersivedCriterion / PredictionNetwork at encoder and context widths other than 256 and with a speaker embedding
(cpc/criterion/criterion.py:89-95, 154-160): construction, state-dict layout, the reference's initialisation of heads wider than
the context, which path the module takes.  No GPU: the forward itself is covered by tests/test_gpu_criterion_widths.py."""
import json
import os

import pytest
import torch

from cpc_audio_amd import ops
from cpc_audio_amd.criterion import CPCUnsupersivedCriterion, PredictionNetwork
from cpc_audio_amd.train import build_criterion

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("H,C", [(256, 40), (64, 128), (512, 512), (256, 13)])
def test_construction_at_other_widths(H, C):
    crit = build_criterion(nPredicts=5, hiddenGar=H, hiddenEncoder=C, negativeSamplingExt=16)
    sd = crit.state_dict()
    assert list(sd.keys()) == [f"wPrediction.predictors.{k}.weight" for k in range(5)]
    assert all(tuple(v.shape) == (C, H) for v in sd.values())
    assert crit.wPrediction.scores_apart and crit.speakerEmb is None
    assert tuple(crit.wPrediction.stacked_weight().shape) == (5 * C, H)


def test_state_dict_layout_equals_the_fixture_meta():
    with open(os.path.join(GOLDEN, "criterion_widths_meta.json")) as f:
        meta = json.load(f)
    assert len(meta["cases"]) == 3
    for tag, cs in meta["cases"].items():
        crit = CPCUnsupersivedCriterion(meta["K"], cs["H"], cs["C"], meta["N"], speakerEmbedding=cs["E"], nSpeakers=cs["speakers"],
                                        sizeInputSeq=meta["S"])
        sd = crit.state_dict()
        assert list(sd.keys()) == cs["keys"], tag
        assert {k: list(v.shape) for k, v in sd.items()} == cs["shapes"], tag


def test_wider_encoders_raise_with_the_limit_named():
    with pytest.raises(NotImplementedError, match="512"):
        PredictionNetwork(3, 256, 513)
    with pytest.raises(NotImplementedError, match="512"):
        build_criterion(hiddenEncoder=1024)
    assert ops.nce_wide_supported(512) and ops.nce_wide_supported(1) and not ops.nce_wide_supported(513)
    assert not ops.nce_wide_supported(0)
    assert ops.nce_wide_padded_width(13) == 64 and ops.nce_wide_padded_width(320) == 320


def test_heads_wider_than_the_context_start_as_the_reference_initialises_them():
    """criterion.py:92-95: rows 0 .. H-1 of every head N(0, 1), rows H .. C-1 RESIDUAL_STD * N(0, 1)."""
    torch.manual_seed(0)
    H, C = 64, 128
    net = PredictionNetwork(4, H, C)
    assert net.RESIDUAL_STD == 0.01
    for p in net.predictors:
        assert tuple(p.weight.shape) == (C, H)
        assert p.weight[H:].std().item() < 0.05 and p.weight[:H].std().item() > 0.5
    # ... and no re-initialisation where the context is at least as wide: nn.Linear's own (uniform within 1 / sqrt(H))
    net = PredictionNetwork(2, 128, 64)
    assert all(p.weight.abs().max().item() <= 1.0 / 128 ** 0.5 + 1e-6 for p in net.predictors)


def test_speaker_embedding_widens_the_context():
    crit = CPCUnsupersivedCriterion(5, 16, 16, 16, speakerEmbedding=8, nSpeakers=5, sizeInputSeq=20)
    sd = crit.state_dict()
    assert tuple(sd["speakerEmb.weight"].shape) == (5, 8)
    assert all(p.in_features == 16 + 8 and p.out_features == 16 for p in crit.wPrediction.predictors)
    assert crit.wPrediction.scores_apart
    # 256 / 256 with an embedding is not the fused path either: the context is 256 + E wide
    crit = CPCUnsupersivedCriterion(3, 256, 256, 16, speakerEmbedding=16, nSpeakers=4)
    assert crit.wPrediction.predictors[0].in_features == 272 and crit.wPrediction.scores_apart


def test_the_default_widths_keep_the_fused_path():
    crit = build_criterion().eval()
    assert not crit.wPrediction.scores_apart and not crit.wPrediction.wide and crit.speakerEmb is None
    assert not build_criterion(dropout=True).eval().wPrediction.scores_apart
    assert build_criterion(dropout=True).train().wPrediction.scores_apart


@pytest.mark.parametrize("kw", [dict(hiddenGar=24, hiddenEncoder=40), dict(hiddenGar=16, hiddenEncoder=16, speakerEmbedding=8, nSpeakers=5)])
def test_cpu_input_raises_the_no_cpu_path_error(kw):
    crit = build_criterion(nPredicts=5, negativeSamplingExt=16, **kw)
    c, z = torch.randn(2, 20, kw["hiddenGar"]), torch.randn(2, 20, kw["hiddenEncoder"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(c, z, torch.zeros(2, dtype=torch.long))
