"""The NumPy reference and the named cases of the mask-map tests (tests/golden/mask_cases.py), proved without a GPU: the packing
against its definition bit by bit, the maps against oracle.mask_iou.mask_iou_maps_loops, and every builder against the list of
contents tests/test_gpu_mask_iou_abi.py relies on (a case that lost its empty mask would leave that test blind, not failing)."""
import numpy as np
import pytest

import mask_cases as mc
from oracle import mask_iou as oracle


def _same_f16(a, b):
    """Equal NaN positions, equal bits elsewhere"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb])


@pytest.mark.parametrize("hw", [1, 63, 64, 65, 130, 1028])
def test_pack_words_is_the_definition(hw):
    m = mc.byte_masks(5, hw)
    got = mc.pack_words(m)
    assert got.shape == (mc.n_words(hw), 5) and got.dtype == np.uint64 and got.flags["C_CONTIGUOUS"]
    want = np.zeros(got.shape, dtype=object)                  # Python integers: no packing routine in the reference of the packing
    for n in range(5):
        for px in range(hw):
            if m[n, px] != 0:
                want[px // 64, n] |= 1 << (px % 64)
    assert [[int(v) for v in row] for row in got] == [[int(v) for v in row] for row in want]
    assert np.array_equal(mc.unpack_words(got, hw), m != 0)
    assert not mc.unpack_words(got)[:, hw:].any()             # tail bits
    assert np.array_equal(mc.pack_words(m.reshape(5, 1, hw)), got) and np.array_equal(mc.pack_words(m != 0), got)


def test_popcount():
    rng = np.random.RandomState(0)
    a = rng.randint(0, 1 << 32, size=200).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, size=200).astype(np.uint64)
    a[:3] = (0, mc.ONES, 1 << 63)
    assert mc.popcount(a).tolist() == [bin(int(v)).count("1") for v in a]


def test_maps_equal_the_oracle_loops_on_every_small_case():
    m, _ = mc.small_masks()
    iou, asy, area = mc.maps_from_words(mc.pack_words(m))
    riou, rasy = oracle.mask_iou_maps_loops(m.reshape(len(m), 10, 13) != 0)
    assert _same_f16(iou, riou) and _same_f16(asy, rasy)
    assert np.array_equal(area, (m != 0).sum(axis=1))
    for n, words in ((1, 1), (2, 1), (2, 33), (63, 1), (65, 2)):
        bits = mc.pair_bits(n, words)
        iou, asy, area = mc.maps_from_words(mc.pack_words(bits))
        riou, rasy = oracle.mask_iou_maps_loops(bits)
        assert _same_f16(iou, riou) and _same_f16(asy, rasy), (n, words)
        assert np.array_equal(area, bits.sum(axis=1))


def test_maps_equal_the_oracle_matmul_at_the_largest_case():
    bits = mc.pair_bits(193, 65)
    iou, asy, _ = mc.maps_from_words(mc.pack_words(bits))
    riou, rasy = oracle.mask_iou_maps(bits)
    assert _same_f16(iou, riou) and _same_f16(asy, rasy)


def _one(x):
    return x.view(np.uint16) == 0x3C00


def test_small_masks_hold_every_named_case():
    m, at = mc.small_masks()
    b = m != 0
    assert set(np.unique(m)) == set(mc.BYTES)
    assert set(np.unique(m[at["bytes_a"]])) == set(mc.BYTES)
    assert not b[at["empty_a"]].any() and not b[at["empty_b"]].any() and b[at["full"]].all()
    assert np.array_equal(b[at["same_a"]], b[at["same_b"]]) and b[at["same_a"]].any() and not b[at["same_a"]].all()
    assert not np.array_equal(m[at["disj_a"]], m[at["disj_b"]])
    assert not (b[at["disj_a"]] & b[at["disj_b"]]).any() and b[at["disj_a"]].any() and b[at["disj_b"]].any()
    assert (b[at["inner"]] <= b[at["outer"]]).all() and 0 < b[at["inner"]].sum() < b[at["outer"]].sum()
    for name, px in (("last", 129), ("bit63", 63), ("bit64", 64)):
        assert np.flatnonzero(b[at[name]]).tolist() == [px]
    iou, asy, area = mc.maps_from_words(mc.pack_words(m))
    e = [at["empty_a"], at["empty_b"]]
    assert np.isnan(iou[np.ix_(e, e)]).all() and np.isnan(asy[:, e]).all()            # 0 / 0: the diagonal, the pair, a column
    assert not np.isnan(asy[:, 2:]).any() and (asy[e, 2:] == 0).all()
    assert np.isnan(iou).sum() == 4
    assert _one(iou[at["same_a"], at["same_b"]]) and iou[at["disj_a"], at["disj_b"]] == 0
    assert _one(asy[at["outer"], at["inner"]]) and 0 < asy[at["inner"], at["outer"]] < 1


@pytest.mark.parametrize("n,words", [(63, 1), (64, 31), (65, 32), (128, 33), (129, 65), (193, 65), (193, 1)])
def test_pair_cases_hold_every_named_case(n, words):
    b = mc.pair_bits(n, words)
    w = mc.pack_words(b)
    nbits = 64 * words
    assert w.shape == (words, n) and np.array_equal(mc.unpack_words(w), b)
    assert not b[mc.EMPTY_A].any() and not b[mc.EMPTY_B].any() and b[mc.FULL].all()
    assert (w[:, mc.FULL] == mc.ONES).all()                                        # a word with all 64 bits set
    assert np.array_equal(b[mc.SAME_A], b[mc.SAME_B]) and 0 < b[mc.SAME_A].sum() < nbits
    assert not (b[mc.DISJ_A] & b[mc.DISJ_B]).any() and b[mc.DISJ_A].any() and b[mc.DISJ_B].any()
    assert np.flatnonzero(b[mc.BIT63]).tolist() == [63] and np.flatnonzero(b[mc.LAST]).tolist() == [nbits - 1]
    assert np.flatnonzero(b[mc.BIT64]).tolist() == [64 if words > 1 else 0]
    empty = np.flatnonzero(~b.any(axis=1)).tolist()
    assert empty == [mc.EMPTY_A, mc.EMPTY_B]                                       # no other mask is empty
    iou, asy, area = mc.maps_from_words(w)
    assert np.isnan(iou).sum() == 4 and np.isnan(asy).sum() == 2 * n
    assert _one(iou[mc.SAME_A, mc.SAME_B]) and iou[mc.DISJ_A, mc.DISJ_B] == 0 and area[mc.FULL] == nbits
    if n > mc.OUTER:
        assert mc.INNER < 64 <= mc.OUTER                                           # i in tile 0, j in tile 1
        assert (b[mc.INNER] <= b[mc.OUTER]).all() and 0 < b[mc.INNER].sum() < b[mc.OUTER].sum()
        assert _one(asy[mc.OUTER, mc.INNER]) and 0 < asy[mc.INNER, mc.OUTER] < 1


def test_the_two_small_pair_cases():
    assert mc.pair_bits(1, 33).shape == (1, 33 * 64) and mc.pair_bits(1, 33).any()
    b = mc.pair_bits(2, 31)
    assert not b[0].any() and b[1].all()
    iou, asy, _ = mc.maps_from_words(mc.pack_words(b))
    assert np.isnan(iou[0, 0]) and iou[0, 1] == 0 and _one(iou[1, 1]) and np.isnan(asy[:, 0]).all() and asy[0, 1] == 0


def test_the_witness_is_a_witness():
    """683 / 8195 rounds to different halves directly and through float32; the case holds it as iou both ways and as asy"""
    inter, union = mc.WITNESS
    q = np.float64(inter) / np.float64(union)
    direct, chain = q.astype(np.float16), q.astype(np.float32).astype(np.float16)
    assert direct.view(np.uint16) != chain.view(np.uint16)
    assert abs(int(direct.view(np.uint16)) - int(chain.view(np.uint16))) == 1
    assert union > 64 * (mc.WITNESS_WORDS - 1)                                     # it needs the 129th word
    w = mc.witness_words()
    assert w.shape == (mc.WITNESS_WORDS, mc.WITNESS_N)
    b = mc.unpack_words(w)
    assert b[mc.WIT_IN].sum() == inter and b[mc.WIT_OUT_SAME].sum() == union and b[mc.WIT_OUT_NEXT].sum() == union
    assert (b[mc.WIT_IN] <= b[mc.WIT_OUT_NEXT]).all() and mc.WIT_IN < 64 <= mc.WIT_OUT_NEXT and mc.WIT_OUT_SAME < 64
    iou, asy, area = mc.maps_from_words(w)
    for out in (mc.WIT_OUT_SAME, mc.WIT_OUT_NEXT):
        for got in (iou[mc.WIT_IN, out], iou[out, mc.WIT_IN], asy[mc.WIT_IN, out]):
            assert got.view(np.uint16) == chain.view(np.uint16) != direct.view(np.uint16)
    assert np.isnan(iou).sum() == 4                                                # the empty masks of pair_bits are still there


def test_no_smaller_union_has_a_witness():
    """Every inter <= union < 8195: the two chains agree (so the witness cannot be had in fewer than 129 words)"""
    for union in range(1, mc.WITNESS[1]):
        q = np.arange(0, union + 1, dtype=np.float64) / np.float64(union)
        assert np.array_equal(q.astype(np.float16).view(np.uint16), q.astype(np.float32).astype(np.float16).view(np.uint16)), union
    q = np.arange(0, mc.WITNESS[0], dtype=np.float64) / np.float64(mc.WITNESS[1])
    assert np.array_equal(q.astype(np.float16).view(np.uint16), q.astype(np.float32).astype(np.float16).view(np.uint16))
