"""Reference and named cases of the mask-map tests (tests/test_mask_cases_cpu.py, tests/test_gpu_mask_iou_abi.py): pure NumPy, no
import of the library under test and none of the oracle - tests/test_mask_cases_cpu.py holds this file to oracle/mask_iou.py.

  pack_words      masks -> [words, N] uint64, the layout include/cim_hip.h states for cim_mask_pack: bit b of word w of mask n is
                  pixel 64 w + b != 0, tail bits zero
  maps_from_words [words, N] uint64 -> (iou f16, asy f16, area int64) by integer popcounts and the reference's rounding chain
                  int64 -> float64 divide -> float32 -> float16

Every builder is deterministic (its own RandomState)."""
import numpy as np

BYTES = (0, 1, 2, 0x80, 0xFF)            # what a uint8 mask may hold: "non-zero = inside"
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
WITNESS = (683, 8195)                    # inter, union (and inter, area): f64 -> f16 differs from f64 -> f32 -> f16
WITNESS_WORDS = 129                      # 8195 set pixels need 129 words


def n_words(hw):
    return (hw + 63) // 64


def pack_words(masks_u8):
    """masks [N, HW] or [N, H, W], any dtype (non-zero = inside) -> [words, N] uint64, word-major, tail bits zero"""
    m = np.asarray(masks_u8)
    n = m.shape[0]
    bits = m.reshape(n, -1) != 0
    hw = bits.shape[1]
    words = n_words(hw)
    padded = np.zeros((n, words * 64), dtype=bool)
    padded[:, :hw] = bits
    packed = np.packbits(padded, axis=1, bitorder="little")              # [N, 8 words] bytes, pixel 8 q + b = bit b of byte q
    return np.ascontiguousarray(np.ascontiguousarray(packed).view("<u8").T).astype(np.uint64)


def unpack_words(words_u64, hw=None):
    """[words, N] uint64 -> bool [N, 64 words] (or [N, hw])"""
    w = np.ascontiguousarray(np.asarray(words_u64, dtype="<u8").T)
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)
    return bits if hw is None else bits[:, :hw]


def popcount(a):
    """Set bits of every uint64 of `a` -> int64 (the SWAR sum; no float on the way)"""
    x = np.asarray(a, dtype=np.uint64).copy()
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    x = x + (x >> np.uint64(8))
    x = x + (x >> np.uint64(16))
    x = x + (x >> np.uint64(32))
    return (x & np.uint64(0x7F)).astype(np.int64)


def ratio_f16(num_i64, den_i64):
    """int64 / int64 -> float64 -> float32 -> float16 (0 / 0 = NaN, as the reference's true_divide gives it)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (num_i64.astype(np.float64) / den_i64.astype(np.float64)).astype(np.float32).astype(np.float16)


def maps_from_words(words_u64):
    """[words, N] uint64 -> (iou f16 [N, N], asy f16 [N, N], area int64 [N]):
    iou[i, j] = |m_i & m_j| / |m_i | m_j|, asy[i, j] = |m_i & m_j| / |m_j|"""
    w = np.asarray(words_u64, dtype=np.uint64)
    n = w.shape[1]
    area = popcount(w).sum(axis=0)
    inter = np.zeros((n, n), dtype=np.int64)
    for row in w:                                                        # one word of every mask at a time: [N, N] ands
        inter += popcount(row[:, None] & row[None, :])
    union = area[:, None] + area[None, :] - inter
    return ratio_f16(inter, union), ratio_f16(inter, np.broadcast_to(area[None, :], (n, n))), area


# ---- named cases ---------------------------------------------------------------------------------------------------------------

def byte_masks(n, hw, seed=0):
    """[n, hw] uint8 drawn from BYTES (half of the pixels 0): what cim_mask_pack reads"""
    rng = np.random.RandomState(1000 * n + hw + seed)
    return np.array(BYTES, np.uint8)[rng.choice(len(BYTES), size=(n, hw), p=[0.5, 0.125, 0.125, 0.125, 0.125])]


def _random_bits(rng, n, nbits):
    """bool [n, nbits], the masks' densities cycling through 5 %, 50 % and 95 %"""
    dens = np.array([0.05, 0.5, 0.95])[np.arange(n) % 3]
    return rng.random_sample((n, nbits)) < dens[:, None]


# where pair_bits places its named masks (N >= 63; "OUTER" only where N >= 65: the second tile)
EMPTY_A, FULL, EMPTY_B, SAME_A, SAME_B, BIT63, BIT64, LAST, DISJ_A, DISJ_B, INNER, OUTER = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 64


def pair_bits(n, words):
    """bool [n, 64 words]: the operand of one cim_mask_iou_pair case.  n = 1: one random mask; n = 2: an empty and a full mask;
    n >= 63: random masks of three densities with the named masks at the indices above (BIT64 is bit 0 where words = 1)."""
    nbits = 64 * words
    rng = np.random.RandomState(7919 * n + words)
    b = _random_bits(rng, n, nbits)
    b[:, 0] = True                                                       # a random mask is never empty
    if n == 2:
        b[0], b[1] = False, True
    if n >= 63:
        b[EMPTY_A] = b[EMPTY_B] = False
        b[FULL] = True
        b[SAME_B] = b[SAME_A]
        for at, bit in ((BIT63, 63), (BIT64, 64 % nbits), (LAST, nbits - 1)):
            b[at] = False
            b[at, bit] = True
        half = rng.random_sample(nbits) < 0.5
        half[:2] = (True, False)
        b[DISJ_A] &= half
        b[DISJ_B] &= ~half
        b[DISJ_A, 0] = b[DISJ_B, 1] = True
    if n > OUTER:
        b[OUTER] = rng.random_sample(nbits) < 0.7
        b[OUTER, :2] = True
        b[INNER] = b[OUTER] & (rng.random_sample(nbits) < 0.5)
        b[INNER, :2] = (True, False)                                     # non-empty and strictly inside
    return b


def pair_words(n, words):
    """pair_bits packed: [words, n] uint64"""
    return pack_words(pair_bits(n, words))


WITNESS_N, WIT_IN, WIT_OUT_SAME, WIT_OUT_NEXT = 65, 3, 5, 64


def witness_words():
    """[129, 65] uint64: pair_bits(65, 129) with the double-rounding witness in it: mask WIT_IN = the first 683 pixels, masks
    WIT_OUT_SAME (same tile) and WIT_OUT_NEXT (the mirrored tile of one row) = the first 8195 pixels, so that
    inter = 683, union = 8195 = the outer mask's area: iou[in, out] = iou[out, in] = asy[in, out] = 683 / 8195."""
    b = pair_bits(WITNESS_N, WITNESS_WORDS)
    for at, count in ((WIT_IN, WITNESS[0]), (WIT_OUT_SAME, WITNESS[1]), (WIT_OUT_NEXT, WITNESS[1])):
        b[at] = False
        b[at, :count] = True
    return pack_words(b)


def small_masks():
    """-> (uint8 [14, 130], names): every named case at a size the oracle's double loop takes (3 words, a 2-pixel tail word)"""
    hw = 130
    rng = np.random.RandomState(5)
    m = byte_masks(14, hw, seed=1)
    names = {"empty_a": 0, "empty_b": 1, "full": 2, "same_a": 3, "same_b": 4, "disj_a": 5, "disj_b": 6, "inner": 7, "outer": 8,
             "last": 9, "bit63": 10, "bit64": 11, "bytes_a": 12, "bytes_b": 13}
    m[0] = m[1] = 0
    m[2] = 0xFF
    m[4] = m[3]
    half = rng.random_sample(hw) < 0.5
    m[5] = np.where(half, np.maximum(m[5], 1), 0)
    m[6] = np.where(half, 0, np.maximum(m[6], 2))
    m[8] = np.where(rng.random_sample(hw) < 0.7, 0x80, 0)
    m[8, :2] = 1
    m[7] = np.where(rng.random_sample(hw) < 0.5, m[8], 0)
    m[7, :2] = (2, 0)
    for at, px in ((9, hw - 1), (10, 63), (11, 64)):
        m[at] = 0
        m[at, px] = 0xFF
    return m, names
