"""An independent restatement of the transformer layer's dropout masks ("dropout"): Philox4x32-10 written from the
published algorithm (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the layer's numbering of its two
dropout sites.  Plain numpy; imports neither the library nor anything of oracle/ -- the tests compare the library against it.

Generator: counter (block & 0xFFFFFFFF, block >> 32, site, 0), key (seed & 0xFFFFFFFF, seed >> 32), ten rounds
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   key += (W0, W1) after each round.
Site 0, attention probability (bh, i, j) of (B*8, S, S): block (bh ceil(S/4) + (i >> 2)) S + j, word i & 3, kept iff
    word >= floor(double(float32(p)) 2^32).
Site 1, hidden activation (row, col) of (B*S, 2048): block (row >> 2) 1024 + (((col >> 6) << 5) | (col & 31)), word row & 3,
    field = the word's high 16 bits if col & 32 else its low 16 bits, kept iff field >= floor(double(float32(p)) 65536).
A kept element carries float32(1) / (float32(1) - float32(p)), a dropped one 0; layer g of a group call uses (seed + g) mod 2^64.
"""
import numpy as np

M0 = 0xD2511F53
M1 = 0xCD9E8D57
W0 = 0x9E3779B9
W1 = 0xBB67AE85
FFN_WIDTH = 2048
MASK32 = np.uint64(0xFFFFFFFF)

# published known-answer vectors of Philox4x32-10 (Random123's kat_vectors): (counter c0..c3, key k0 k1, output)
KNOWN_ANSWERS = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit words, key: two -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(w, dtype=np.uint64) & MASK32 for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.uint64(int(w) & 0xFFFFFFFF) for w in key)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]                     # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return c


def draw(seed, site, block):
    """The four words of block `block` (uint64 array) of dropout site `site` under the 64-bit `seed`: (4,) + block.shape."""
    seed = int(seed) % (1 << 64)
    block = np.asarray(block, dtype=np.uint64)
    return np.stack(philox4x32((block & MASK32, block >> np.uint64(32), site, 0), (seed & 0xFFFFFFFF, seed >> 32)))


def attn_element_map(BH, S):
    """Site 0: (block, word, field) of every element (bh, i, j) of a (BH, S, S) tensor; field is 0 (a whole word per element)."""
    bh, i, j = np.meshgrid(np.arange(BH, dtype=np.uint64), np.arange(S, dtype=np.uint64), np.arange(S, dtype=np.uint64),
                           indexing="ij")
    block = (bh * np.uint64((S + 3) // 4) + (i >> np.uint64(2))) * np.uint64(S) + j
    return block, (i & np.uint64(3)).astype(np.int64), np.zeros(block.shape, dtype=np.int64)


def ffn_element_map(rows):
    """Site 1: (block, word, field) of every element (row, col) of a (rows, 2048) tensor; field 1 = the high 16 bits."""
    row, col = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(FFN_WIDTH, dtype=np.uint64), indexing="ij")
    block = (row >> np.uint64(2)) * np.uint64(FFN_WIDTH // 2) + (((col >> np.uint64(6)) << np.uint64(5)) | (col & np.uint64(31)))
    return block, (row & np.uint64(3)).astype(np.int64), ((col >> np.uint64(5)) & np.uint64(1)).astype(np.int64)


def threshold32(p):
    return int(float(np.float32(p)) * 4294967296.0)


def threshold16(p):
    return int(float(np.float32(p)) * 65536.0)


def keep_probability(site, p):
    """The exact probability that the specification keeps an element (uniform words)."""
    return 1.0 - threshold32(p) / 4294967296.0 if site == 0 else 1.0 - threshold16(p) / 65536.0


def keep_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _select(words, word):
    return np.take_along_axis(words, word[None], axis=0)[0]


def attn_bits(BH, S, seed):
    """The 32 random bits of every element of site 0 (independent of p): uint64 (BH, S, S)."""
    block, word, _ = attn_element_map(BH, S)
    return _select(draw(seed, 0, block), word)


def ffn_bits(rows, seed):
    """The 16 random bits of every element of site 1 (independent of p): uint64 (rows, 2048)."""
    block, word, field = ffn_element_map(rows)
    w = _select(draw(seed, 1, block), word)
    return np.where(field == 1, w >> np.uint64(16), w & np.uint64(0xFFFF))


def attn_keep_bool(BH, S, p, seed, bits=None):
    return (attn_bits(BH, S, seed) if bits is None else bits) >= np.uint64(threshold32(p))


def ffn_keep_bool(rows, p, seed, bits=None):
    return (ffn_bits(rows, seed) if bits is None else bits) >= np.uint64(threshold16(p))


def _as_mask(keep, p):
    import torch
    return torch.from_numpy(np.where(keep, keep_scale(p), np.float32(0)).astype(np.float32))


def attn_keep_ref(BH, S, p, seed, bits=None):
    """What cpc_dropout_keep_mask(site 0) must return: float32 (BH, S, S), 0 or 1 / (1 - p).  (bits: attn_bits(BH, S, seed), to
    threshold one draw at several p.)"""
    return _as_mask(attn_keep_bool(BH, S, p, seed, bits), p)


def ffn_keep_ref(rows, p, seed, bits=None):
    """What cpc_dropout_keep_mask(site 1) must return: float32 (rows, 2048), 0 or 1 / (1 - p)."""
    return _as_mask(ffn_keep_bool(rows, p, seed, bits), p)
