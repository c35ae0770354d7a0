"""The surface of the LSTM at any hidden width (no GPU): the cpc_lstm_*_h symbols and their argument checks, which return
before any launch, and the hiddenKernel keyword of model.CPCAR / train.build_model / common_voices_eval."""
import ctypes
import os
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cpc_lstm_layout_h", "cpc_lstm_forward_h", "cpc_lstm_backward_h"]
SHAPE, ARG = 1, 2            # CPC_ERR_SHAPE, CPC_ERR_ARG


def _library():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    return _lib.bind(build.build())


def test_header_and_signature_table_carry_the_new_entries():
    from cpc_audio_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and f"{name}(" in text, name
    assert _lib.EXPECTED_ABI == 16
    i, p = ctypes.c_int, ctypes.c_void_p
    # symbols were added, none changed
    assert _lib.SIGNATURES["cpc_lstm_forward_in"] == (i, [p] * 9 + [i] * 5 + [p])
    assert _lib.SIGNATURES["cpc_lstm_forward_h"] == (i, [p] * 9 + [i] * 6 + [p])
    assert _lib.SIGNATURES["cpc_lstm_backward_h"] == (i, [p] * 10 + [i] * 6 + [p])


def test_library_exports_the_symbols_and_layout_checks_its_ranges():
    lib = _library()
    assert lib.cpc_abi_version() == 16
    for name in NEW:
        assert hasattr(lib, name)
    sizes = (ctypes.c_long * 3)()
    B, S, nl, D, H = 2, 33, 2, 40, 130
    for bad in [dict(H=0), dict(H=513), dict(D=0), dict(D=513), dict(nl=0), dict(nl=9), dict(B=0), dict(B=1 << 11, S=(1 << 10) + 1)]:
        a = dict(B=B, S=S, nl=nl, D=D, H=H)
        a.update(bad)
        assert lib.cpc_lstm_layout_h(*a.values(), sizes) == SHAPE, bad
    assert lib.cpc_lstm_layout_h(B, S, nl, D, H, None) == ARG
    assert lib.cpc_lstm_layout_h(B, S, nl, D, H, sizes) == 0
    assert all(v > 0 for v in sizes)
    # H == 256 is the input-width entry
    old = (ctypes.c_long * 3)()
    assert lib.cpc_lstm_layout_h(B, S, nl, D, 256, sizes) == 0 and lib.cpc_lstm_layout_in(B, S, nl, D, old) == 0
    assert tuple(sizes) == tuple(old)


def test_forward_and_backward_check_their_arguments_before_any_launch():
    lib = _library()
    B, S, nl, D, H = 2, 5, 1, 40, 130
    ref = torch.nn.LSTM(D, H, nl, batch_first=True)
    plist = [p.detach().clone() for p in ref.parameters()]
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    parr = (ctypes.c_void_p * 4)(*[P(t) for t in plist])
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_lstm_layout_h(B, S, nl, D, H, sizes) == 0
    x = torch.randn(B, S, D)
    h0 = torch.zeros(nl, B, H)
    saved, fscr, bscr = (torch.full((sizes[k],), 7.0) for k in range(3))
    y = torch.full((B, S, H), 7.0)
    hN, cN = torch.full((nl, B, H), 7.0), torch.full((nl, B, H), 7.0)
    dx = torch.full((B, S, D), 7.0)
    grads = [torch.full_like(t, 7.0) for t in plist]
    garr = (ctypes.c_void_p * 4)(*[P(t) for t in grads])

    def fwd(**kw):
        a = dict(x=P(x), h0=None, c0=None, params=parr, saved=P(saved), scratch=P(fscr), y=P(y), hN=P(hN), cN=P(cN), B=B, S=S,
                 nl=nl, D=D, H=H, flags=0)
        a.update(kw)
        return lib.cpc_lstm_forward_h(*a.values(), None)

    def bwd(**kw):
        a = dict(x=P(x), h0=None, c0=None, params=parr, saved=P(saved), y=P(y), dy=P(y), scratch=P(bscr), dx=P(dx),
                 grads=garr, B=B, S=S, nl=nl, D=D, H=H, flags=0)
        a.update(kw)
        return lib.cpc_lstm_backward_h(*a.values(), None)

    for call in (fwd, bwd):
        assert call(params=None) == ARG
        assert call(h0=P(h0)) == ARG                       # h0 without c0
        assert call(flags=2) == ARG                        # unknown flag bit
        assert call(H=513) == SHAPE and call(H=0) == SHAPE and call(D=513) == SHAPE and call(nl=9) == SHAPE
        assert call(x=None) == ARG
    assert fwd(y=None) == ARG and fwd(hN=None) == ARG and bwd(dx=None) == ARG and bwd(grads=None) == ARG
    for t in [saved, fscr, bscr, y, hN, cN, dx] + grads:   # nothing was launched: every buffer still holds its fill
        assert bool((t == 7.0).all())


def test_the_keyword_sets_an_attribute_of_its_own():
    from cpc_audio_amd.model import CPCAR
    ar = CPCAR(256, 512, False, 1, mode="LSTM", lstmKernel=True, hiddenKernel=True)
    assert ar.hip_hidden is True and ar.hip_lstm is False and ar.hip_in is False and ar.hip is False and ar.hip_rnn is False
    assert CPCAR(256, 512, False, 1, mode="LSTM", lstmKernel=True).hip_hidden is False             # off by default
    assert CPCAR(256, 512, False, 1, mode="LSTM", hiddenKernel=True).hip_hidden is False            # needs lstmKernel too
    assert CPCAR(256, 512, False, 1, mode="GRU", lstmKernel=True, hiddenKernel=True).hip_hidden is False
    assert CPCAR(256, 512, False, 1, mode="RNN", lstmKernel=True, rnnKernel=True, hiddenKernel=True).hip_hidden is False
    assert CPCAR(40, 130, False, 8, mode="LSTM", lstmKernel=True, hiddenKernel=True).hip_hidden is True
    assert CPCAR(40, 513, False, 1, mode="LSTM", lstmKernel=True, hiddenKernel=True).hip_hidden is False
    assert CPCAR(40, 130, False, 9, mode="LSTM", lstmKernel=True, hiddenKernel=True).hip_hidden is False
    same = CPCAR(256, 256, False, 1, mode="LSTM", lstmKernel=True, hiddenKernel=True)             # 256 stays what it was
    assert same.hip_lstm is True and same.hip_hidden is False
    keys = list(ar.state_dict())
    assert keys == ["baseNet." + k for k in torch.nn.LSTM(256, 512, 1, batch_first=True).state_dict()]


def test_cpu_input_runs_the_torch_module():
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(0)
    ar = CPCAR(40, 130, True, 2, mode="LSTM", lstmKernel=True, hiddenKernel=True)
    assert ar.hip_hidden
    x = torch.randn(2, 5, 40)
    y = ar(x)
    want, h = ar.baseNet(x)
    assert torch.equal(y, want)
    for a, b in zip(ar.hidden, h):
        assert torch.equal(a, b)
    assert not hasattr(y, "_cpc_abs_bound")


def test_build_model_passes_the_keyword():
    from cpc_audio_amd import train
    m = train.build_model(hiddenGar=512, arMode="LSTM", nLevelsGRU=1, lstmKernel=True, hiddenKernel=True)
    assert m.gAR.hip_hidden is True and m.gAR.hip_lstm is False
    assert train.build_model(hiddenGar=512, arMode="LSTM", nLevelsGRU=1, lstmKernel=True).gAR.hip_hidden is False
    assert train.build_model().gAR.hip_hidden is False and train.build_model(hiddenKernel=True).gAR.hip is True


def test_the_per_classifier_and_its_command_line_take_the_keyword():
    from cpc_audio_amd import common_voices_eval as cv
    crit = cv.CTCphone_criterion(40, 41, LSTM=True, hipFront=True, wideKernel=True, hiddenKernel=True)
    assert crit.hiddenKernel is True
    assert cv.CTCphone_criterion(40, 41, LSTM=True, hipFront=True, wideKernel=True).hiddenKernel is False
    args = cv.parse_args(["train", "db", "phones.txt", "ckpt.pt", "--LSTM", "--hipFront", "--wideKernel", "--hiddenKernel"])
    assert args.hiddenKernel is True
    assert not hasattr(cv.parse_args(["train", "db", "phones.txt", "ckpt.pt"]), "hiddenKernel")
