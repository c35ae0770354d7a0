"""The surface of the GRU at any hidden width (no GPU): the cpc_gru_*_h symbols and their argument checks, which return before
any launch, and the hiddenKernel keyword of model.CPCAR / train.build_model / harness.loadModel for mode GRU."""
import ctypes
import json
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cpc_gru_layout_h", "cpc_gru_paths_h", "cpc_gru_forward_h", "cpc_gru_backward_h"]
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
    assert re.search(r"#define CPC_GRU_PER_STEP 1\b", text)
    assert _lib.EXPECTED_ABI == 16
    i, p = ctypes.c_int, ctypes.c_void_p
    # symbols were added, none changed
    assert _lib.SIGNATURES["cpc_gru_forward_in"] == (i, [p] * 7 + [i] * 4 + [p])
    assert _lib.SIGNATURES["cpc_gru_backward_in"] == (i, [p] * 9 + [i] * 4 + [p])
    assert _lib.SIGNATURES["cpc_gru_layout_h"] == (i, [i] * 5 + [p])
    assert _lib.SIGNATURES["cpc_gru_paths_h"] == (i, [i])
    assert _lib.SIGNATURES["cpc_gru_forward_h"] == (i, [p] * 7 + [i] * 6 + [p])
    assert _lib.SIGNATURES["cpc_gru_backward_h"] == (i, [p] * 9 + [i] * 6 + [p])


def test_library_exports_the_symbols_and_layout_checks_its_ranges():
    lib = _library()
    assert lib.cpc_abi_version() == 16
    for name in NEW:
        assert hasattr(lib, name)
    sizes = (ctypes.c_long * 3)()
    B, S, nl, D, H = 2, 33, 2, 40, 130
    # (the last three: B*S > 2^21 rows; B*S*3Hp > 2^31 at Hp = 512, where B*S = 2^20.5 rows alone would pass)
    for bad in [dict(H=0), dict(H=513), dict(D=0), dict(D=513), dict(nl=0), dict(nl=9), dict(B=0), dict(S=0),
                dict(B=1 << 11, S=(1 << 10) + 1), dict(B=1 << 10, S=1449, H=512), dict(B=1 << 10, S=1821, H=300)]:
        a = dict(B=B, S=S, nl=nl, D=D, H=H)
        a.update(bad)
        assert lib.cpc_gru_layout_h(*a.values(), sizes) == SHAPE, bad
    assert lib.cpc_gru_layout_h(1 << 10, 1365, nl, D, 512, sizes) == 0          # 1365 * 2^10 * 1536 <= 2^31
    assert lib.cpc_gru_layout_h(1 << 11, 1 << 10, nl, D, 130, sizes) == 0        # 2^21 rows at Hp = 256
    assert lib.cpc_gru_layout_h(B, S, nl, D, H, None) == ARG
    assert lib.cpc_gru_layout_h(B, S, nl, D, H, sizes) == 0
    assert all(v > 0 for v in sizes)
    # H == 256 is the input-width entry
    old = (ctypes.c_long * 3)()
    assert lib.cpc_gru_layout_h(B, S, nl, D, 256, sizes) == 0 and lib.cpc_gru_layout_in(B, S, nl, D, old) == 0
    assert tuple(sizes) == tuple(old)
    assert lib.cpc_gru_paths_h(1) == 0 and lib.cpc_gru_paths_h(0) == 0           # nothing was launched


def test_forward_and_backward_check_their_arguments_before_any_launch():
    lib = _library()
    B, S, nl, D, H = 2, 5, 1, 40, 130
    ref = torch.nn.GRU(D, H, nl, batch_first=True)
    plist = [p.detach().clone() for p in ref.parameters()]
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    parr = (ctypes.c_void_p * 4)(*[P(t) for t in plist])
    hole = (ctypes.c_void_p * 4)(P(plist[0]), None, P(plist[2]), P(plist[3]))
    sizes = (ctypes.c_long * 3)()
    assert lib.cpc_gru_layout_h(B, S, nl, D, H, sizes) == 0
    x = torch.randn(B, S, D)
    saved, fscr, bscr = (torch.full((sizes[k],), 7.0) for k in range(3))
    y = torch.full((B, S, H), 7.0)
    hN = torch.full((nl, B, H), 7.0)
    dx = torch.full((B, S, D), 7.0)
    grads = [torch.full_like(t, 7.0) for t in plist]
    garr = (ctypes.c_void_p * 4)(*[P(t) for t in grads])

    def fwd(**kw):
        a = dict(x=P(x), h0=None, params=parr, saved=P(saved), scratch=P(fscr), y=P(y), hN=P(hN), B=B, S=S, nl=nl, D=D, H=H,
                 flags=0)
        a.update(kw)
        return lib.cpc_gru_forward_h(*a.values(), None)

    def bwd(**kw):
        a = dict(x=P(x), h0=None, params=parr, saved=P(saved), y=P(y), dy=P(y), scratch=P(bscr), dx=P(dx), grads=garr, B=B, S=S,
                 nl=nl, D=D, H=H, flags=0)
        a.update(kw)
        return lib.cpc_gru_backward_h(*a.values(), None)

    for call in (fwd, bwd):
        assert call(params=None) == ARG and call(params=hole) == ARG
        assert call(flags=2) == ARG and call(flags=3) == ARG       # unknown flag bits
        assert call(H=256, flags=1) == ARG                         # the 256 path's choice is cpc_set_gru_mode's
        assert call(H=513) == SHAPE and call(H=0) == SHAPE and call(D=513) == SHAPE and call(D=0) == SHAPE
        assert call(nl=9) == SHAPE and call(nl=0) == SHAPE and call(B=0) == SHAPE
        assert call(x=None) == ARG and call(saved=None) == ARG and call(scratch=None) == ARG and call(y=None) == ARG
    assert fwd(hN=None) == ARG and bwd(dx=None) == ARG and bwd(grads=None) == ARG and bwd(dy=None) == ARG and bwd(grads=hole) == ARG
    for t in [saved, fscr, bscr, y, hN, dx] + grads:       # nothing was launched: every buffer still holds its fill
        assert bool((t == 7.0).all())
    assert lib.cpc_gru_paths_h(1) == 0


def test_the_keyword_sets_an_attribute_of_its_own():
    from cpc_audio_amd.model import CPCAR
    ar = CPCAR(256, 512, False, 2, mode="GRU", hiddenKernel=True)
    assert ar.hip_gru_hidden is True
    assert ar.hip_hidden is False and ar.hip is False and ar.hip_in is False and ar.hip_lstm is False and ar.hip_rnn is False
    assert CPCAR(256, 512, False, 2, mode="GRU").hip_gru_hidden is False                             # off by default
    assert CPCAR(256, 512, False, 2, mode="GRU", inputKernel=True).hip_gru_hidden is False           # another keyword
    same = CPCAR(256, 256, False, 2, mode="GRU", hiddenKernel=True)                                  # 256 stays what it was
    assert same.hip is True and same.hip_gru_hidden is False
    narrow = CPCAR(40, 256, False, 2, mode="GRU", inputKernel=True, hiddenKernel=True)
    assert narrow.hip_in is True and narrow.hip_gru_hidden is False
    assert CPCAR(40, 130, False, 8, mode="GRU", hiddenKernel=True).hip_gru_hidden is True
    assert CPCAR(1, 1, False, 1, mode="GRU", hiddenKernel=True).hip_gru_hidden is True
    assert CPCAR(40, 513, False, 1, mode="GRU", hiddenKernel=True).hip_gru_hidden is False
    assert CPCAR(513, 130, False, 1, mode="GRU", hiddenKernel=True).hip_gru_hidden is False
    assert CPCAR(40, 130, False, 9, mode="GRU", hiddenKernel=True).hip_gru_hidden is False
    # the LSTM keeps its own attribute and rule, the RNN stays on torch
    lstm = CPCAR(256, 512, False, 1, mode="LSTM", lstmKernel=True, hiddenKernel=True)
    assert lstm.hip_hidden is True and lstm.hip_gru_hidden is False
    assert CPCAR(256, 512, False, 1, mode="LSTM", hiddenKernel=True).hip_gru_hidden is False
    rnn = CPCAR(256, 512, False, 1, mode="RNN", rnnKernel=True, hiddenKernel=True)
    assert rnn.hip_gru_hidden is False and rnn.hip_hidden is False and rnn.hip_rnn is False
    keys = list(ar.state_dict())
    assert keys == ["baseNet." + k for k in torch.nn.GRU(256, 512, 2, batch_first=True).state_dict()]


def test_cpu_input_runs_the_torch_module():
    from cpc_audio_amd.model import CPCAR
    torch.manual_seed(0)
    ar = CPCAR(40, 130, True, 2, mode="GRU", hiddenKernel=True)
    assert ar.hip_gru_hidden
    x = torch.randn(2, 5, 40)
    y = ar(x)
    want, h = ar.baseNet(x)
    assert torch.equal(y, want) and torch.equal(ar.hidden, h)
    assert not hasattr(y, "_cpc_abs_bound")
    y2 = ar(x)                                              # the carried state goes into the second call
    assert torch.equal(y2, ar.baseNet(x, h)[0])


def test_the_function_refuses_what_it_does_not_take():
    """ops.GruHiddenFunction has no CPU path: a CPU tensor is an error, not a quiet torch forward."""
    from cpc_audio_amd import ops
    net = torch.nn.GRU(40, 130, 1, batch_first=True)
    with pytest.raises(RuntimeError, match="GruHiddenFunction"):
        ops.GruHiddenFunction.apply(torch.randn(2, 5, 40), None, False, *net.parameters())
    assert ops.GRU_HIDDEN_MAX == 512


def test_build_model_passes_the_keyword():
    from cpc_audio_amd import train
    m = train.build_model(hiddenGar=512, hiddenKernel=True)                    # the package's default: GRU, two layers
    assert m.gAR.hip_gru_hidden is True and m.gAR.hip is False and m.gAR.hip_hidden is False
    assert train.build_model(hiddenGar=512).gAR.hip_gru_hidden is False
    plain = train.build_model(hiddenKernel=True).gAR
    assert plain.hip is True and plain.hip_gru_hidden is False
    lstm = train.build_model(hiddenGar=512, arMode="LSTM", nLevelsGRU=1, lstmKernel=True, hiddenKernel=True).gAR
    assert lstm.hip_hidden is True and lstm.hip_gru_hidden is False


def test_load_model_passes_the_keyword(tmp_path):
    from cpc_audio_amd import harness, train
    src = train.build_model(hiddenGar=128, arMode="GRU", nLevelsGRU=1)
    with open(tmp_path / "checkpoint_args.json", "w") as f:
        json.dump({"arMode": "GRU", "hiddenGar": 128, "hiddenEncoder": 256, "nLevelsGRU": 1}, f)
    path = str(tmp_path / "checkpoint_5.pt")
    torch.save({"gEncoder": src.state_dict()}, path)
    m, hidden_gar, hidden_encoder = harness.loadModel([path], hiddenKernel=True)
    assert (hidden_gar, hidden_encoder) == (128, 256)
    assert m.gAR.hip_gru_hidden is True and m.gAR.hip is False
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in m.state_dict().items())
    assert harness.loadModel([path])[0].gAR.hip_gru_hidden is False            # off by default
    with open(tmp_path / "checkpoint_args.json", "w") as f:                    # an LSTM checkpoint is not this keyword's
        json.dump({"arMode": "LSTM", "hiddenGar": 128, "hiddenEncoder": 256, "nLevelsGRU": 1}, f)
    torch.save({"gEncoder": train.build_model(hiddenGar=128, arMode="LSTM", nLevelsGRU=1).state_dict()}, path)
    lstm = harness.loadModel([path], hiddenKernel=True)[0].gAR
    assert lstm.hip_gru_hidden is False and lstm.hip_hidden is False
