"""Phone posteriors on an MI355X: ops.posterior (cpc_posterior_forward) against torch in float64 on the CPU, with the bounds of
tests/test_emu_posterior.py -- softmax within 4 x f32_dev of tests/golden/zerospeech_meta.json (what the reference's own float32
run deviates from its float64 run on inputs of this scale) and rows that sum to 1 within 1e-6; one-hot exact, after the test has
made sure in float64 that no row's top-2 margin is under 1e-4 of its scale."""
import itertools
import json
import os

import pytest
import torch
import torch.nn.functional as F

import zerospeech_util as U
from cpc_audio_amd import ops

pytestmark = pytest.mark.gpu

H = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ref = {}


def _f32_dev():
    with open(os.path.join(ROOT, "tests", "golden", "zerospeech_meta.json")) as f:
        return json.load(f)["f32_dev"]


def _case(R, C):
    """Seeded inputs and their float64 logits, computed once per shape and left unchanged."""
    if (R, C) not in _ref:
        g = torch.Generator().manual_seed(3000 * R + C)      # (a rule under which no case has a close top-2 margin)
        x = torch.randn(R, H, generator=g)
        W = (2 * torch.rand(C, H, generator=g) - 1) / 16
        b = (2 * torch.rand(C, generator=g) - 1) / 16
        _ref[(R, C)] = (x, W, b, F.linear(x.double(), W.double(), b.double()))
    return _ref[(R, C)]


def _check(post, hot, logits):
    C = logits.shape[1]
    assert post.dtype == torch.float32 and hot.dtype == torch.int64 and post.shape == hot.shape == logits.shape
    post, hot = post.cpu(), hot.cpu()
    err = (post.double() - torch.softmax(logits, dim=1)).abs().max().item()
    row_sum = (post.double().sum(dim=1) - 1).abs().max().item()
    print(f"R={logits.shape[0]} C={C}: max abs err {err:.3e} (bound {4 * _f32_dev():.3e}), max |row sum - 1| {row_sum:.3e}")
    assert err <= 4 * _f32_dev()
    assert row_sum <= 1e-6
    assert torch.equal(hot, F.one_hot(logits.argmax(dim=1), C))


@pytest.mark.parametrize("R,C", list(itertools.product((1, 33, 401), (2, 42, 65, 251))))
def test_posteriors_and_one_hot_match_torch_float64(R, C):
    x, W, b, logits = _case(R, C)
    assert U.close_rows(logits) == 0                      # one-hot compares exactly on every row
    xd, Wd, bd = x.cuda(), W.cuda(), b.cuda()
    post, hot = ops.posterior(xd, Wd, bd), ops.posterior(xd, Wd, bd, one_hot=True)
    _check(post, hot, logits)
    assert torch.equal(ops.posterior(xd, Wd, bd), post) and torch.equal(ops.posterior(xd, Wd, bd, one_hot=True), hot)   # same bits
    ops.check_device_errors()


@pytest.mark.parametrize("C", [384, 385, 449])
def test_more_classes_than_stay_in_lds(C):
    """Up to 384 classes a tile's logits all stay in LDS; beyond, the posteriors take a second walk over the classes."""
    x, W, b, logits = _case(35, C)
    assert U.close_rows(logits) == 0
    xd, Wd, bd = x.cuda(), W.cuda(), b.cuda()
    _check(ops.posterior(xd, Wd, bd), ops.posterior(xd, Wd, bd, one_hot=True), logits)
    ops.check_device_errors()


def test_the_last_frame_is_read_through_its_row_stride():
    Bq, S, C = 33, 7, 42
    x, W, b, _ = _case(Bq * S, C)
    c = x.view(Bq, S, H).cuda()
    last = c[:, -1, :]
    assert last.stride(0) == S * H and not last.is_contiguous()
    logits = F.linear(x.view(Bq, S, H)[:, -1, :].double(), W.double(), b.double())
    assert U.close_rows(logits) == 0
    post, hot = ops.posterior(last, W.cuda(), b.cuda()), ops.posterior(last, W.cuda(), b.cuda(), one_hot=True)
    _check(post, hot, logits)
    assert torch.equal(post, ops.posterior(last.contiguous(), W.cuda(), b.cuda()))
    ops.check_device_errors()


def test_rows_off_the_16_byte_grid_take_the_scalar_loads():
    R, C = 33, 65
    x, W, b, logits = _case(R, C)
    buf = torch.empty(R * H + 1, device="cuda")
    view = buf[1:].view(R, H)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    assert torch.equal(ops.posterior(view, W.cuda(), b.cuda()), ops.posterior(x.cuda(), W.cuda(), b.cuda()))
    ops.check_device_errors()


def test_a_workgroup_walks_several_tiles():
    """More 32-row tiles than the 512 workgroups of a one-step call: the bits of two calls that stay under the cap."""
    R, C, cut = 512 * 32 + 33, 5, 512 * 32
    x, W, b, _ = _case(R, C)
    xd, Wd, bd = x.cuda(), W.cuda(), b.cuda()
    for one_hot in (False, True):
        out = ops.posterior(xd, Wd, bd, one_hot=one_hot)
        parts = torch.cat([ops.posterior(xd[:cut], Wd, bd, one_hot=one_hot), ops.posterior(xd[cut:], Wd, bd, one_hot=one_hot)])
        assert torch.equal(out, parts)
    assert bool((out.sum(dim=1) == 1).all())
    ops.check_device_errors()


def test_other_inputs_are_refused():
    W, b = torch.zeros(42, H, device="cuda"), torch.zeros(42, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.posterior(torch.zeros(4, H), W, b)
    with pytest.raises(TypeError):
        ops.posterior(torch.zeros(4, H, device="cuda", dtype=torch.float64), W, b)
    with pytest.raises(NotImplementedError):
        ops.posterior(torch.zeros(4, 128, device="cuda"), W[:, :128], b)
    with pytest.raises(ValueError):
        ops.posterior(torch.zeros(4, H, device="cuda"), W[:1], b[:1])                 # one class
    with pytest.raises(ValueError):
        ops.posterior(torch.zeros(4, H, device="cuda"), W, b[:41])
