"""The MFCC encoder without a GPU: model.MFCCEncoder's torch path, ops.mfcc_tables, train.build_model(encoder_type="mfcc",
mfccKernel=True), harness.loadModel and harness.build_feature against the float64 numpy oracle of tests/mfcc_util.py (explicit
DFT matrices; neither torch.stft nor the package's tables).  Tolerances: tests/mfcc_util.py."""
import json
import math

import pytest
import torch

import mfcc_util as U
from cpc_audio_amd import harness, model, ops, train


@pytest.mark.parametrize("N,L,D", U.CASES_CPU)
def test_torch_path_matches_the_oracle(N, L, D):
    x = U.case(N, L, seed=N + L + D)
    enc = model.MFCCEncoder(D)
    for rowwise in (False, True):
        enc.topPerRow = rowwise
        want = U.oracle(x, D, rowwise)["y"].permute(0, 2, 1)
        y64 = enc.double()(x.double().unsqueeze(1))
        assert tuple(y64.shape) == (N, D, U.frames(L)) and y64.dtype == torch.float64
        assert U.rel_err(y64, want) < 1e-12
        y32 = enc.float()(x.unsqueeze(1))
        assert y32.dtype == torch.float32 and U.rel_err(y32, want) < U.BAR
        assert not y32.requires_grad and y32.grad_fn is None


@pytest.mark.parametrize("variant", U.VARIANTS)
def test_torch_fp32_stays_below_the_bars(variant):
    N, L, D = U.VARIANT_SHAPE
    x = U.case(N, L, seed=7, variant=variant)
    bar_db, bar_y = U.bars(variant)
    for rowwise in (False, True):
        ref = U.oracle(x, D, rowwise)
        db, y = U.torch_stages(x, D, torch.float32, rowwise)
        e = U.rel_err(db, ref["db"]), U.rel_err(y, ref["y"])
        print(f"{variant} rowwise={rowwise}: db {e[0]:.3g} y {e[1]:.3g}")
        assert e[0] < bar_db and e[1] < bar_y


def test_frame_counts_and_the_shortest_window():
    for L, F in [(161, 2), (320, 2), (321, 3), (20480, 128), (64000, 400)]:
        assert ops.mfcc_frames(L) == F == (L - 1) // 160 + 1
    enc = model.MFCCEncoder(13)
    assert tuple(enc(torch.zeros(1, 1, 161)).shape) == (1, 13, 2)
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 1, 160))
    assert ops.mfcc_supported(1, 161, 13) and ops.mfcc_supported(64, 20480, 512)
    assert not ops.mfcc_supported(1, 160, 13) and not ops.mfcc_supported(1, 161, 0) and not ops.mfcc_supported(1, 161, 513)
    assert not ops.mfcc_supported(1 << 20, 64000, 40)


@pytest.mark.parametrize("D", [40, 256, 512])
def test_tables_match_the_oracle_and_pin_the_empty_filters(D):
    basis, fb, dct = ops.mfcc_tables(D)
    M = max(128, D)
    assert basis.dtype == fb.dtype == dct.dtype == torch.float32
    assert tuple(basis.shape) == (321, 322) and tuple(fb.shape) == (161, M) and tuple(dct.shape) == (M, D)
    wc, wsn, fb64, dct64 = (torch.from_numpy(t) for t in U.oracle_tables(D))
    assert torch.equal(basis, torch.cat([wc, -wsn], dim=1).float())
    assert torch.equal(fb, fb64.float()) and U.rel_err(dct, dct64.t()) < 1e-7
    assert int((fb == 0).all(dim=0).sum()) == U.EMPTY_FILTERS[M]


def test_silence():
    N, L, D = U.VARIANT_SHAPE
    y = model.MFCCEncoder(D)(torch.zeros(N, 1, L))
    M = max(128, D)
    assert U.rel_err(y[:, 0, :], torch.full((N, U.frames(L)), -100.0 * math.sqrt(M))) < 1e-5
    assert float(y[:, 1:, :].abs().max()) <= 1e-3


def test_the_floor_of_the_whole_call_and_of_one_row():
    N, L, D = U.VARIANT_SHAPE
    x = U.case(N, L, seed=7, variant="quiet_row").unsqueeze(1)
    enc = model.MFCCEncoder(D)
    both, alone = enc(x), enc(x[1:])
    assert not torch.allclose(both[1], alone[0])                            # row 1 is floored by row 0's maximum
    assert U.rel_err(both, U.oracle(x[:, 0], D)["y"].permute(0, 2, 1)) < U.BAR
    assert U.rel_err(alone, U.oracle(x[1:, 0], D)["y"].permute(0, 2, 1)) < U.BAR
    enc.topPerRow = True
    assert torch.equal(enc(x), torch.cat([enc(x[:1]), enc(x[1:])]))


def test_state_dict_keys_shapes_and_reload():
    enc = model.MFCCEncoder(40)
    state = enc.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == {"MFCC.MelSpectrogram.spectrogram.window": (321,),
                                                             "MFCC.MelSpectrogram.mel_scale.fb": (161, 128),
                                                             "MFCC.dct_mat": (128, 40)}
    assert list(enc.parameters()) == [] and enc.DOWNSAMPLING == 160 and enc.getDimOutput() == 40
    assert torch.allclose(state["MFCC.MelSpectrogram.spectrogram.window"], torch.hann_window(321), rtol=0, atol=1e-6)
    # a loaded window is the truth from then on: the kernel's basis and the torch path follow it
    other = model.MFCCEncoder(40)
    state["MFCC.MelSpectrogram.spectrogram.window"] = torch.ones(321)
    other.load_state_dict(state, strict=True)
    assert torch.equal(other.basis, ops.mfcc_basis(torch.ones(321))) and not torch.equal(other.basis, enc.basis)
    x = U.case(1, 1040, seed=1).unsqueeze(1)
    assert not torch.allclose(other(x), enc(x))


def test_build_model_with_the_keyword():
    m = train.build_model(encoder_type="mfcc", mfccKernel=True, arMode="no_ar", hiddenEncoder=40)
    assert type(m.gEncoder) is model.MFCCEncoder and type(m.gAR) is model.NoAr
    c, z, _ = m(U.case(2, 1040, seed=2).unsqueeze(1), None)
    assert c is z and tuple(z.shape) == (2, 7, 40) and not z.requires_grad
    g = train.build_model(encoder_type="mfcc", mfccKernel=True, arMode="GRU", hiddenEncoder=40, hiddenGar=48, nLevelsGRU=1)
    assert type(g.gAR) is model.CPCAR and tuple(g(U.case(2, 1040, seed=2).unsqueeze(1), None)[0].shape) == (2, 7, 48)
    with pytest.raises(NotImplementedError, match="mfccKernel"):
        train.build_model(encoder_type="mfcc")


def test_load_model_rebuilds_an_mfcc_checkpoint(tmp_path):
    src = train.build_model(hiddenEncoder=40, arMode="no_ar", encoder_type="mfcc", mfccKernel=True)
    with open(tmp_path / "checkpoint_args.json", "w") as f:
        json.dump({"encoder_type": "mfcc", "arMode": "no_ar", "hiddenEncoder": 40}, f)
    torch.save({"gEncoder": src.state_dict()}, tmp_path / "checkpoint_0.pt")
    m, hidden_gar, hidden_enc = harness.loadModel([str(tmp_path / "checkpoint_0.pt")])
    assert type(m.gEncoder) is model.MFCCEncoder and type(m.gAR) is model.NoAr and (hidden_gar, hidden_enc) == (40, 40)
    x = U.case(1, 1040, seed=4).unsqueeze(1)
    assert torch.equal(m(x, None)[1], src(x, None)[1])


def test_build_feature_equals_the_oracle_chunk_by_chunk():
    D = 40
    m = train.build_model(encoder_type="mfcc", mfccKernel=True, arMode="no_ar", hiddenEncoder=D)
    g = torch.Generator().manual_seed(13)
    wave = (0.1 * torch.randn(1, 150000, generator=g)).clamp_(-1, 1)
    wave[:, 64000:128000] *= 1e-4                                  # the second chunk 80 dB below the first
    assert [e - f for f, e, _ in harness.chunk_plan(150000, 64000, False, 160)] == [64000, 64000, 22000]
    got = harness.build_feature(harness.FeatureModule(m, False).eval(), wave)
    assert m.gEncoder.topPerRow is False                          # (set for the duration of the call only)
    assert tuple(got.shape) == (1, 400 + 400 + 138, D)
    assert U.rel_err(got, U.oracle_chunks(wave, D)) < U.BAR
