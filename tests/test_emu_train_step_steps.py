"""cpc_train_step runs the recurrence only over the time steps the loss reads (csrc/train_step.hip), on the host emulator.

The criterion reads c[:, :W], W = S - K.  The step's BACKWARD recurrence therefore runs W steps in every phase mask (dc[:, W:] is
the zero tail the step writes itself), and with phase bit 32 -- "the caller reads neither hN nor c beyond step W - 1" -- the
FORWARD recurrence does too.  B = 16, S = 16, K = 12 (W = 4: three quarters of the steps go), N = 16, workspace NaN-filled:
    * phases 3 against the stage-wise path, whose backward is the untrimmed cpc_gru_backward_streams: out, z, c, hN and every
      gradient torch.equal -- the backward trim changes no value;
    * phases 3 | 32 against phases 3: out, z, c[:, :W] and every gradient torch.equal, c[:, W:] == 0, hN still the NaN it held;
    * phases 3 | 32 with h0, and phases 2 | 32, are argument errors."""
import ctypes

import torch

from emu_util import P, emu
from test_emu_train_step import ENC, GRU, _composite, _setup, _stagewise

B, L, K, N = 16, 2560, 12, 16
ERR_ARG = 2
_cache = {}


def _runs():
    """The three steps, computed once and left unchanged."""
    if not _cache:
        lib = emu()
        sizes = (ctypes.c_long * 8)()
        assert lib.cpc_train_step_layout(B, L, K, N, sizes) == 0 and sizes[3] == 16
        p, wave, S, bidx, sidx, plist = _setup(B, L, K, N)
        assert S == 16
        _cache["setup"] = (wave, bidx, sidx, plist)
        _cache["stagewise"] = _stagewise(lib, wave, bidx, sidx, None, plist, B, L, K, N)
        _cache["full"] = _composite(lib, wave, bidx, sidx, None, 1.0, plist, B, L, K, N, phases=(3,))
        _cache["trimmed"] = _composite(lib, wave, bidx, sidx, None, 1.0, plist, B, L, K, N, phases=(3 | 32,))
        assert lib.cpc_device_error_flags(1) == 0
    return _cache


def test_backward_over_the_window_steps_matches_the_stagewise_step_emulated():
    r = _runs()
    out, hN, grads, z, c = r["full"]
    out2, hN2, grads2, z2, c2 = r["stagewise"]
    assert torch.isfinite(out).all() and torch.isfinite(c).all() and torch.isfinite(hN).all()
    assert torch.equal(out, out2) and torch.equal(hN, hN2) and torch.equal(z, z2) and torch.equal(c, c2)
    for n, a, b in zip(ENC + GRU + ["wall"], grads, grads2):
        assert torch.isfinite(a).all(), n
        assert torch.equal(a, b), n


def test_forward_over_the_window_steps_changes_only_what_nobody_reads_emulated():
    r = _runs()
    W = 16 - K
    out, hN, grads, z, c = r["full"]
    out2, hN2, grads2, z2, c2 = r["trimmed"]
    assert torch.equal(out, out2) and torch.equal(z, z2)
    assert torch.equal(c[:, :W], c2[:, :W])
    assert (c2[:, W:] == 0).all()
    assert torch.isnan(hN2).all()                         # not written: the NaN it was filled with
    for n, a, b in zip(ENC + GRU + ["wall"], grads, grads2):
        assert torch.isfinite(b).all(), n
        assert torch.equal(a, b), n


def test_the_forward_bit_needs_phase_one_and_no_carried_state_emulated():
    lib = emu()
    wave, bidx, sidx, plist = _runs()["setup"]
    sizes = (ctypes.c_long * 8)()
    assert lib.cpc_train_step_layout(B, L, K, N, sizes) == 0
    ws = torch.full((sizes[0],), float("nan"))
    grads = [torch.zeros_like(t) for t in plist]
    parr = (ctypes.c_void_p * 29)(*[P(t) for t in plist])
    garr = (ctypes.c_void_p * 29)(*[P(t) for t in grads])
    out, hN, ones, h0 = torch.zeros(2, K), torch.zeros(2, B, 256), torch.ones(K), torch.zeros(2, B, 256)

    def call(h, phases):
        return lib.cpc_train_step(P(wave), P(bidx), P(sidx), P(h), 1.0, parr, garr, P(ones), P(ws), out[0].data_ptr(),
                                  out[1].data_ptr(), P(hN), B, L, K, N, phases, None, None, None, None)
    assert call(h0, 3 | 32) == ERR_ARG
    assert call(None, 2 | 32) == ERR_ARG
    assert call(None, 64 | 3) == ERR_ARG
    assert torch.isnan(ws).all()                          # refused before any launch
