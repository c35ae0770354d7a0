"""The C ABI and the module surface of the HIP prediction networks (csrc/pred_conv.hip; ``hipPredictors``) -- no GPU needed."""
import ctypes
import json
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpc_pred_conv_layout", "cpc_pred_conv_forward", "cpc_pred_conv_backward")


def _built():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from cpc_audio_amd import _lib, build
    return _lib.bind(build.build())


def test_symbols_are_declared_bound_and_exported():
    from cpc_audio_amd import _lib
    header = open(os.path.join(ROOT, "include", "cpc_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\(", header, re.M), name
        assert name in _lib.SIGNATURES, name
    # the argument counts of the header and the table agree
    for name in SYMBOLS:
        decl = re.search(r"^int\s+" + name + r"\(([^;]*)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    bound = _built()                        # raises if a declared symbol is missing from the gfx950 build
    for name in SYMBOLS:
        assert hasattr(bound, name)
    assert bound.cpc_abi_version() == 16 and _lib.EXPECTED_ABI == 16      # symbols were added, none changed


def test_layout_limits():
    bound = _built()
    sizes = (ctypes.c_long * 3)()
    assert bound.cpc_pred_conv_layout(2, 116, 12, 12, sizes) == 0
    assert sizes[0] == 12 * 12 * 65536 and sizes[2] == 2 * 116 * 12 * 256 and sizes[1] > sizes[0] + sizes[2]
    assert bound.cpc_pred_conv_layout(1, 1, 64, 16, sizes) == 0               # the stated limits
    for bad in ((2, 116, 0, 4), (2, 116, 65, 4), (2, 116, 12, 0), (2, 116, 12, 17), (0, 116, 12, 4), (2, 0, 12, 4),
                (1 << 15, 256, 1, 1),                  # B W G 256 = 2^31
                (1 << 20, 1 << 20, 12, 4)):            # B W alone overflows an int
        assert bound.cpc_pred_conv_layout(*bad, sizes) == 1, bad              # CPC_ERR_SHAPE
    assert bound.cpc_pred_conv_layout((1 << 15) - 1, 256, 1, 1, sizes) == 0
    assert bound.cpc_pred_conv_layout(2, 116, 12, 4, None) == 2               # CPC_ERR_ARG
    p = ctypes.c_void_p(8)
    s = 0.1
    assert bound.cpc_pred_conv_forward(p, p, p, p, p, 2, 116, 12, 17, 1, s, 0, None) == 1
    assert bound.cpc_pred_conv_forward(p, p, p, p, None, 2, 116, 12, 4, 1, s, 0, None) == 2
    assert bound.cpc_pred_conv_backward(p, p, p, p, p, p, p, p, 2, 116, 0, 4, 1, s, 0, None) == 1
    assert bound.cpc_pred_conv_backward(p, p, None, p, p, p, p, p, 2, 116, 12, 4, 1, s, 1, None) == 2


@pytest.mark.parametrize("mode", ["conv8", "ffd"])
def test_flag_keeps_the_state_dict_and_the_cpu_path(mode):
    """hipPredictors=True: the reference's state-dict keys and shapes; CPU input takes the torch modules, bit-equal to the
    flag off."""
    import torch
    from cpc_audio_amd.criterion import CPCUnsupersivedCriterion, PredictionNetwork
    from cpc_audio_amd.train import build_criterion
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "predictors_meta.json")))
    shapes = {k: tuple(v) for k, v in meta["modes"][mode]["keys"].items()}
    torch.manual_seed(5)
    on = PredictionNetwork(3, 256, 256, mode, hipPredictors=True)
    off = PredictionNetwork(3, 256, 256, mode)
    assert on.hipPredictors and not off.hipPredictors and on.scores_apart and on.last_path is None
    assert {k: tuple(v.shape) for k, v in on.state_dict().items()} == shapes
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    off.load_state_dict(on.state_dict(), strict=True)
    c = torch.randn(2, 6, 256)
    a, b = on.predictions(c), off.predictions(c)
    assert on.last_path == "torch" and off.last_path == "torch"
    assert a.shape == (2, 6, 3 * 256) and torch.equal(a, b)
    assert CPCUnsupersivedCriterion(3, 256, 256, 8, rnnMode=mode, hipPredictors=True).wPrediction.hipPredictors
    assert build_criterion(rnnMode=mode, hipPredictors=True).wPrediction.hipPredictors
    assert not build_criterion(rnnMode=mode).wPrediction.hipPredictors        # off by default
