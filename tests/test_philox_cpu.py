"""The independent dropout-mask reference (tests/philox_util.py) against published vectors, and the properties a dropout mask
must have, asserted on that reference: tests/test_emu_dropout_mask.py and tests/test_gpu_dropout_mask.py then require the library
to equal it bit for bit, which transfers every property here to the kernels.  CPU only, no emulator, no library."""
import math

import numpy as np
import pytest

import philox_util as PU


def test_reference_reproduces_the_published_known_answer_vectors():
    for counter, key, expect in PU.KNOWN_ANSWERS:
        got = tuple(int(w) for w in PU.philox4x32(counter, key))
        assert got == expect, (counter, key, [hex(w) for w in got])
    # vectorised: the three at once through one key each, and a scalar counter broadcast against an array
    blocks = np.array([0, 1, 2], dtype=np.uint64)
    many = PU.draw(5, 1, blocks)
    for n, b in enumerate(blocks):
        assert [int(w) for w in many[:, n]] == [int(w) for w in PU.philox4x32((int(b), 0, 1, 0), (5, 0))]


def _assert_injective(block, word, field):
    key = block.astype(np.uint64) * np.uint64(8) + word.astype(np.uint64) * np.uint64(2) + field.astype(np.uint64)
    assert word.min() >= 0 and word.max() <= 3 and field.min() >= 0 and field.max() <= 1
    assert np.unique(key).size == key.size


@pytest.mark.parametrize("BH,S", [(8, 1), (8, 37), (16, 128)])
def test_attention_element_map_is_injective(BH, S):
    block, word, field = PU.attn_element_map(BH, S)
    assert block.shape == (BH, S, S) and not field.any()
    _assert_injective(block, word, field)


@pytest.mark.parametrize("rows", [1, 37, 512])
def test_hidden_layer_element_map_is_injective(rows):
    block, word, field = PU.ffn_element_map(rows)
    assert block.shape == (rows, 2048)
    _assert_injective(block, word, field)
    # eight elements per block: the map wastes no draw but in the ragged last row block
    assert int(block.max()) + 1 == ((rows + 3) // 4) * 1024


def test_upper_counter_word_is_out_of_reach():
    """The blocks of the largest shapes the suite runs stay far below 2^32, so counter word 1 (block >> 32) is zero in every
    test here and in the emulator and GPU files: NOT covered.  It is not reachable at any shape the layer accepts either -- site 0
    needs B * 8 * 32 * 128 >= 2^32 (B >= 131072 at S = 128: 64 TiB of saved probabilities), site 1 needs 2^24 rows (a saved hidden
    layer of 128 GiB and its gradient of another 128 GiB: more than an MI355X's 288 GB holds)."""
    assert int(PU.attn_element_map(24, 128)[0].max()) == 24 * 32 * 128 - 1 < 1 << 32
    assert int(PU.ffn_element_map(384)[0].max()) == 96 * 1024 - 1 < 1 << 32
    # the reference itself does place block >> 32 in counter word 1
    hi = PU.draw(3, 1, np.array([(7 << 32) | 9], dtype=np.uint64))[:, 0]
    assert [int(w) for w in hi] == [int(w) for w in PU.philox4x32((9, 7, 1, 0), (3, 0))]


@pytest.mark.parametrize("p", [0.1, 0.2, 0.3, 0.5])
def test_exact_keep_probability_is_within_a_16_bit_step_of_nominal(p):
    for site in (0, 1):
        q = PU.keep_probability(site, p)
        assert abs(q - (1.0 - p)) <= 2.0 ** -16, (site, q)
    assert PU.threshold32(0.0) == 0 and PU.threshold16(0.0) == 0       # p = 0 keeps everything
    assert PU.keep_probability(1, 0.1) == 1.0 - 6553 / 65536.0


# ------------------------------------------------------------------ statistics of the reference's masks
# Fixed seed and shapes: deterministic.  Every bound is five standard deviations of the binomial the ideal generator would
# give, 5 sqrt(a (1 - a) / n) with a the exact probability of the event -- derived, not tuned.  Both masks have 2^20 elements.
SEED, P_DROP = 7, 0.1
ROWS, BH, S = 512, 64, 128
Q0, Q1 = PU.keep_probability(0, P_DROP), PU.keep_probability(1, P_DROP)


@pytest.fixture(scope="module")
def masks():
    m = {"attn": PU.attn_keep_bool(BH, S, P_DROP, SEED), "ffn": PU.ffn_keep_bool(ROWS, P_DROP, SEED),
         "attn+1": PU.attn_keep_bool(BH, S, P_DROP, SEED + 1), "ffn+1": PU.ffn_keep_bool(ROWS, P_DROP, SEED + 1)}
    for v in m.values():
        v.setflags(write=False)
    return m


def _check_rate(hits, a, what):
    n = hits.size
    rate, bound = float(hits.mean()), 5.0 * math.sqrt(a * (1.0 - a) / n)
    print(f"{what}: rate {rate:.6f} expected {a:.6f} |dev| {abs(rate - a):.2e} bound {bound:.2e} (n = {n})")
    assert abs(rate - a) < bound, (what, rate, a, bound)


def _agree(q, r):
    return q * r + (1.0 - q) * (1.0 - r)


def test_overall_keep_rate(masks):
    assert masks["attn"].size == masks["ffn"].size == 1 << 20
    _check_rate(masks["attn"], Q0, "site 0")
    _check_rate(masks["ffn"], Q1, "site 1")


def test_keep_rate_per_output_word(masks):
    for w in range(4):
        _check_rate(masks["attn"][:, w::4, :], Q0, f"site 0 word {w}")      # rows i with i & 3 == w
        _check_rate(masks["ffn"][w::4, :], Q1, f"site 1 word {w}")


def test_keep_rate_per_16_bit_field(masks):
    col = np.arange(2048)
    for f in (0, 1):
        _check_rate(masks["ffn"][:, ((col >> 5) & 1) == f], Q1, f"site 1 field {f}")
        for w in range(4):
            _check_rate(masks["ffn"][w::4][:, ((col >> 5) & 1) == f], Q1, f"site 1 word {w} field {f}")


def test_masks_of_consecutive_seeds_are_independent(masks):
    _check_rate(masks["attn"] == masks["attn+1"], _agree(Q0, Q0), "site 0, seed vs seed + 1")
    _check_rate(masks["ffn"] == masks["ffn+1"], _agree(Q1, Q1), "site 1, seed vs seed + 1")
    # ... and a group's layer g + 1 does not reuse layer g's site-0 draws for its site 1 (seed + 1 is a different KEY)
    _check_rate(masks["attn+1"].ravel() == masks["ffn"].ravel(), _agree(Q0, Q1), "site 0 of seed + 1 vs site 1 of seed")


def test_masks_of_the_two_sites_are_independent(masks):
    _check_rate(masks["attn"].ravel() == masks["ffn"].ravel(), _agree(Q0, Q1), "site 0 vs site 1, element by element")
    # block by block: the same (seed, block, word) under the two site words -- identical if the site word were ignored
    blocks = np.arange(1 << 18, dtype=np.uint64)
    th = np.uint64(PU.threshold32(P_DROP))
    _check_rate((PU.draw(SEED, 0, blocks) >= th) == (PU.draw(SEED, 1, blocks) >= th), _agree(Q0, Q0), "site 0 vs site 1, word by word")


def test_block_mates_are_independent(masks):
    """Elements that share a Philox block (its four words; at site 1 also the two halves of a word) agree no more often than
    independent draws.  Each pairing takes every block at most once per pair, so the pairs are independent."""
    for a, b in [(0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2)]:
        _check_rate(masks["attn"][:, a::4, :] == masks["attn"][:, b::4, :], _agree(Q0, Q0), f"site 0 words {a},{b}")
        _check_rate(masks["ffn"][a::4, :] == masks["ffn"][b::4, :], _agree(Q1, Q1), f"site 1 words {a},{b}")
    col = np.arange(2048)
    lo, hi = masks["ffn"][:, ((col >> 5) & 1) == 0], masks["ffn"][:, ((col >> 5) & 1) == 1]       # col and col + 32, in order
    _check_rate(lo == hi, _agree(Q1, Q1), "site 1 low vs high field of a word")
    for a, b in [(0, 1), (2, 3), (0, 3), (1, 2)]:
        _check_rate(lo[a::4] == hi[b::4], _agree(Q1, Q1), f"site 1 low field of word {a} vs high field of word {b}")
    # neighbouring blocks (consecutive counters): column j vs j + 1 of the same rows
    _check_rate(masks["attn"][:, :, 0:-1:2] == masks["attn"][:, :, 1::2], _agree(Q0, Q0), "site 0 consecutive blocks")
    _check_rate(lo[:, 0::2] == lo[:, 1::2], _agree(Q1, Q1), "site 1 consecutive blocks")     # (column k of `lo` <-> block offset k)
