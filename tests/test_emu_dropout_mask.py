"""The transformer layer's dropout masks on the host SIMT emulator against the independent Philox reference (tests/philox_util.py):
what cpc_dropout_keep_mask reports, bit for bit, and the wrap-around of a group's seed + g.  (The masks the kernels APPLY are
pinned in tests/test_emu_transformer.py::test_transformer_layer_training_dropout_emulated, whose oracle runs on the reference's
masks.)"""
import pytest
import torch

import philox_util as PU
from dropout_util import MASK64, assert_layer_matches, group_call, layer_call, library_masks, oracle_with_reference_masks
from emu_util import emu
from oracle import transformer_oracle as T

SEEDS = [0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1]
PS = [0.0, 0.1, 0.2, 0.3, 0.5]


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_reported_mask_equals_the_reference_emulated(seed):
    lib = emu()
    for BH, S in [(8, 1), (8, 37), (16, 33), (8, 128)]:
        bits = PU.attn_bits(BH, S, seed)
        for p in PS:
            got, _ = library_masks(lib, BH, S, 0, p, seed)
            assert torch.equal(got, PU.attn_keep_ref(BH, S, p, seed, bits)), ("site 0", BH, S, p)
    for rows in [1, 3, 37, 128]:
        bits = PU.ffn_bits(rows, seed)
        for p in PS:
            _, got = library_masks(lib, 0, 1, rows, p, seed)
            assert torch.equal(got, PU.ffn_keep_ref(rows, p, seed, bits)), ("site 1", rows, p)


def test_group_seed_wraps_around_emulated():
    """Layer g of a group call draws with (seed + g) mod 2^64: with seed = 2^64 - 2 the three layers use 2^64 - 2, 2^64 - 1 and 0.
    Each layer's output and gradients equal the single-layer call with that seed, and the masks of those seeds are the reference's."""
    lib = emu()
    B, S, G, p = 1, 37, 3, 0.1
    seed = 2 ** 64 - 2
    prms = [T.make_layer_params(seed=60 + q, size_seq=S, abspos=False) for q in range(G)]
    g = torch.Generator().manual_seed(91)
    x = torch.randn(B, S, 256, generator=g)
    dy = torch.randn(B * S, G * 256, generator=g)
    out, dx, sgrads = group_call(lib, prms, x, dy, p, seed)
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    for q in range(G):
        sq = (seed + q) & MASK64
        assert sq == [2 ** 64 - 2, 2 ** 64 - 1, 0][q]
        attn, ffn = library_masks(lib, B * 8, S, B * S, p, sq)
        assert torch.equal(attn, PU.attn_keep_ref(B * 8, S, p, sq)), q
        assert torch.equal(ffn, PU.ffn_keep_ref(B * S, p, sq)), q
        dyq = dy[:, q * 256:(q + 1) * 256].contiguous()
        o1, d1, g1 = layer_call(lib, prms[q], x, dyq, p, sq)
        assert torch.equal(out[:, q * 256:(q + 1) * 256], o1.view(B * S, 256)), q
        for k, t in g1.items():
            assert torch.equal(sgrads[k][q], t), (q, k)
        # ... and directly: the group's layer against the oracle under the reference's masks of the wrapped seed
        ref = oracle_with_reference_masks(prms[q], x, dyq, p, sq)
        assert_layer_matches((out[:, q * 256:(q + 1) * 256].reshape(B, S, 256), d1, {k: v[q] for k, v in sgrads.items()}), ref, 1e-5,
                             f"group layer {q}")
    # the three layers drew three different masks (same parameters would still differ): no seed was used twice
    m = [PU.ffn_keep_ref(B * S, p, (seed + q) & MASK64) for q in range(G)]
    assert not torch.equal(m[0], m[1]) and not torch.equal(m[1], m[2]) and not torch.equal(m[0], m[2])
