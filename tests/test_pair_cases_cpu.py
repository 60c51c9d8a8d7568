"""The cases of tests/golden/pair_cases.py are sound and not vacuous - shown on the CPU, from the host model alone:

  * every recipe is EXACT: the split loses nothing (h + l == x s), the side meant to carry l does (in at least half of its elements)
    and the other side does not, and sum (|h| + |l|)_A (|h| + |l|)_B plus the bias stays below 2^24 granules - so fp32 accumulation
    gives the float64 value in any order, at any split count, through any reduce order.  If a recipe stops being exact (a changed
    range, a longer K), it fails HERE with the bound that broke, not as a mystery element on the GPU;
  * the table reaches every slab-loop instantiation of cim_amd/csrc/gemm_pair.hip: (wm, MIV) for wm in {0, 1}, MIV in {1, 2, 3, 4} and
    the idle / working boundary for each of form 0's four layouts, MIV in {1, 2, 3, 4 full, 4 ragged} for form 1, for products 3 and 1;
    a case deleted from the table fails the assertion that names what it reached;
  * scale_of's special values."""
import numpy as np
import pytest

import pair_cases as pc
from pair_cases import F32, F64

LIMIT = 2.0 ** 24


def _entries(c):
    return range(c.batch)


@pytest.mark.parametrize("recipe", pc.RECIPES)
def test_every_case_is_exact(recipe):
    worst = 0.0
    for c in pc.CASES:
        assert c.K % 32 == 0 and c.K <= pc.K_MAX and c.N % 4 == 0, c
        for z in _entries(c):
            A, B = pc.operands(c, recipe, z)
            assert A.dtype == F32 and B.dtype == F32 and A.shape == (c.M, c.K) and B.shape == (c.K, c.N)
            sa, sb = pc.entry_scales(c, recipe, z, A, B)
            parts = []
            for x, s, carries in ((A, sa, recipe == "a_l"), (B, sb, recipe == "b_l")):
                h, l = pc.split(x, s)
                xs = x.astype(F64) * F64(s)
                assert np.array_equal((x * F32(s)).astype(F64), xs), (c, "x s is not exact in float32")
                assert np.array_equal(h.astype(F64) + l.astype(F64), xs), (c, recipe, "the split loses bits")
                assert np.all(np.isfinite(h.astype(F64)))
                if carries:
                    assert np.count_nonzero(l) * 2 >= l.size, (c, recipe, np.count_nonzero(l) / l.size)
                else:
                    assert not l.any(), (c, recipe, "the other side carries l")
                parts.append((h, l, pc.granule(h, l)))
            (ha, la, ga), (hb, lb, gb) = parts
            g = ga * gb                                     # divides every product of an element of {hA, lA} with one of {hB, lB}
            assert g > 0
            mag = (np.abs(ha.astype(F64)) + np.abs(la.astype(F64))) @ (np.abs(hb.astype(F64)) + np.abs(lb.astype(F64)))
            unit = F64(sa) * F64(sb) / g                    # 1.0 in granules: the bias (integers) must be whole granules too
            assert unit >= 1 and unit == np.floor(unit), (c, recipe, unit)
            total = mag.max() / g + pc.BIAS_MAX * unit
            assert total < LIMIT, (c, recipe, np.log2(total))
            # the issue's form of the same bound, on the operands themselves
            assert (np.abs(A).astype(F64) @ np.abs(B).astype(F64)).max() * unit < LIMIT
            worst = max(worst, total)
            # the references: float64 of the documented arithmetic is a float32 value; with one side free of l the three products
            # are the plain product, and with both sides free of l so is the single one
            exact = A.astype(F64) @ B.astype(F64)
            p3, p1 = pc.product(A, sa, B, sb, 3), pc.product(A, sa, B, sb, 1)
            assert np.array_equal(p3, exact), (c, recipe)
            assert np.array_equal(p3.astype(F32).astype(F64), p3) and np.array_equal(p1.astype(F32).astype(F64), p1)
            if recipe == "ints":
                assert np.array_equal(p1, exact)
            elif z == 0:
                assert np.count_nonzero(p1 != p3) * 4 >= p3.size, (c, recipe, "dropping the l cluster would go unnoticed")
    assert worst < LIMIT


def test_scales_are_powers_of_two_and_differ_per_batch_entry():
    for c in pc.BATCH_CASES:
        seen = set()
        for z in _entries(c):
            A, B = pc.operands(c, "ints", z)
            sa, sb = pc.entry_scales(c, "ints", z, A, B)
            for s in (sa, sb):
                assert np.frexp(F64(s))[0] == 0.5
            seen.add((float(sa), float(sb)))
        assert len(seen) >= min(c.batch, 12), c
    a0, _ = pc.operands(pc.BATCH_CASES[0], "ints", 0)
    a1, _ = pc.operands(pc.BATCH_CASES[0], "ints", 1)
    assert not np.array_equal(a0, a1)


WORKING = {(wm, miv) for wm in (0, 1) for miv in (1, 2, 3, 4)}


@pytest.mark.parametrize("am,bk", pc.LAYOUTS)
def test_table_reaches_every_form0_instantiation(am, bk):
    cases = [c for c in pc.ROW_CASES if c.form == 0 and (c.a_mcontig, c.b_kcontig) == (am, bk)]
    ragged = set()                      # what the LAST tile selects: a full tile in front reaches (., 4) only
    for c in cases:
        r = pc.last_rows(c)
        ragged.add((0, min(4, -(-r // 32))))
        ragged.add((1, 0) if r <= 128 else (1, -(-(r - 128) // 32)))
        assert ragged <= set().union(*(pc.instantiations(k) for k in cases))
    assert ragged >= WORKING | {(1, 0)}, sorted(WORKING - ragged)
    rs = {pc.last_rows(c) for c in cases}
    assert 128 in rs and (136 if am else 129) in rs, sorted(rs)               # the idle / working boundary of the wm = 1 waves
    assert 256 in rs
    for miv in (1, 2, 3, 4):            # each count also with a RAGGED last sub-tile (r % 32 != 0), on either row of waves
        assert any(r % 32 and r <= 128 and -(-r // 32) == miv for r in rs), (miv, sorted(rs))
        assert any(r % 32 and r > 128 and -(-(r - 128) // 32) == miv for r in rs), (miv, sorted(rs))
    assert {c.M > 256 for c in cases} == {True, False}                        # alone and behind a full tile
    assert any(c.pad_a and c.pad_b and c.pad_c for c in cases) and any(not c.pad_a for c in cases)


def test_table_reaches_every_form1_instantiation():
    cases = [c for c in pc.ROW_CASES if c.form == 1]
    assert all((c.a_mcontig, c.b_kcontig) == (1, 0) for c in cases)
    kinds = set()
    for c in cases:
        r = pc.last_rows(c)
        miv = -(-r // 32)
        assert (0, miv) in pc.instantiations(c) and all(wm == 0 for wm, _ in pc.instantiations(c))
        kinds.add((miv, "full" if r == 128 else "ragged") if miv == 4 else (miv, "any"))
    assert kinds == {(1, "any"), (2, "any"), (3, "any"), (4, "full"), (4, "ragged")}, kinds
    assert {c.M > 128 for c in cases} == {True, False}
    assert {c.K // 16 > 5 for c in cases} == {True, False}                    # the ring of five slabs wraps, and does not


def test_every_case_runs_both_product_counts_and_every_recipe():
    assert set(pc.PRODUCTS) == {3, 1} and set(pc.RECIPES) == {"ints", "a_l", "b_l"}


def test_column_cases():
    ns = {c.N for c in pc.COLUMN_CASES}
    assert ns == {4, 12, 36, 100, 252, 260}
    for c in pc.COLUMN_CASES:
        assert c.b_kcontig or c.N % 8 == 0
        assert c.pad_c > 0
    assert {(c.a_mcontig, c.N) for c in pc.COLUMN_CASES if c.b_kcontig} == {(a, n) for a in (0, 1) for n in ns}


def test_split_cases_force_every_reduce_shape():
    shapes = {}
    for c in pc.SPLIT_CASES:
        eff, per = pc.effective_splits(c)
        slabs = c.K // 32
        shapes.setdefault((c.form, c.a_mcontig, c.b_kcontig), set()).update(
            {("short last split", slabs % per != 0), ("splits > slabs", c.splits > slabs), ("odd count", eff % 2 == 1),
             ("second round of the four-at-a-time walk", eff > 5), ("ragged round of the walk", (eff - 1) % 4 != 0),
             ("one slab per split", per == 1)})
        assert eff > 1 and c.pad_c > 0 and c.K in (160, 512)
    assert set(shapes) == {(0,) + l for l in pc.LAYOUTS} | {(1, 1, 0)}
    for key, got in shapes.items():
        for what in ("short last split", "splits > slabs", "odd count", "second round of the four-at-a-time walk",
                     "ragged round of the walk", "one slab per split"):
            assert (what, True) in got, (key, what)
    assert {c.splits for c in pc.SPLIT_CASES if c.K == 160} == {2, 3, 4, 5, 8, 16}
    assert {c.splits for c in pc.SPLIT_CASES if c.K == 512} == {2, 3, 4, 5, 16, 19}
    assert pc.effective_splits(pc.Case(0, 0, 0, 8, 8, 160, 0, 0, 0, 4, 1, 0)) == (3, 2)          # 2 + 2 + 1 slabs


def test_batch_cases_take_both_branches_of_the_tile_map():
    assert {c.batch for c in pc.BATCH_CASES} == {7, 8, 9, 17} and {c.limit for c in pc.BATCH_CASES} == {0, 1, 3}
    assert {c.form for c in pc.BATCH_CASES} == {0, 1}
    assert {c.N > c.M for c in pc.BATCH_CASES} == {True, False}               # tile_m fastest / tile_n fastest
    for c in pc.BATCH_CASES:
        assert c.splits == 1 and c.pad_a and c.pad_b and c.pad_c


def _bits(x):
    return int(pc.bits(x))


def test_scale_of_special_values():
    assert pc.scale_of(0) == 1.0
    assert pc.scale_of(1) == 1.0 and pc.scale_of(0x007FFFFF) == 1.0           # subnormals
    assert pc.scale_of(_bits(1.0)) == 2.0 ** 14
    assert pc.scale_of(_bits(1.999)) == 2.0 ** 14 and pc.scale_of(_bits(2.0)) == 2.0 ** 13
    assert pc.scale_of(0x7F7FFFFF) == 2.0 ** (14 - 127)                        # the largest finite value
    assert pc.scale_of(0x7F800000) == 1.0                                      # inf
    assert pc.scale_of(0x7FC00000) == 1.0 and pc.scale_of(0x7F800001) == 1.0   # NaN
    assert pc.scale_of(0x00800000) == 2.0 ** 126                               # 2^-126: 268 - 1 clamped to 253
    assert pc.scale_of(15 << 23) == 2.0 ** 126 and pc.scale_of(16 << 23) == 2.0 ** 125       # the clamp's edge
    assert pc.scale_of(_bits(-3.0)) == pc.scale_of(_bits(3.0))                 # (the sign bit is not part of the exponent)
    for v in (1e-30, 0.37, 5.0, 1234.5, 3e30):                                 # |x| s < 2^15, and >= 2^14 where the clamp is idle
        s = float(pc.scale_of(_bits(v)))
        assert 2.0 ** 14 <= v * s < 2.0 ** 15


def test_encode_decode_round_trip_and_layout():
    rng = np.random.RandomState(0)
    x = (rng.randn(5, 24) * np.exp2(8 * (rng.rand(5, 24) - 0.5))).astype(F32)
    s = pc.natural_scale(x)
    h, l = pc.split(x, s)
    img = pc.encode(h, l)
    assert img.dtype == np.int32 and img.shape == (5, 24)
    h2, l2 = pc.decode(img)
    assert np.array_equal(h2.view(np.uint16), h.view(np.uint16)) and np.array_equal(l2.view(np.uint16), l.view(np.uint16))
    raw = img.view(np.float16).reshape(5, 48)
    assert np.array_equal(raw[:, 0:8], h[:, 0:8]) and np.array_equal(raw[:, 8:16], l[:, 0:8]) and np.array_equal(raw[:, 16:24], h[:, 8:16])
    # 22 significant bits: |x s - (h + l)| <= 2^-22 |x s| down to fp16's subnormal range
    err = np.abs(x.astype(F64) * F64(s) - (h.astype(F64) + l.astype(F64)))
    assert np.all(err <= np.maximum(np.abs(x.astype(F64) * F64(s)) * 2.0 ** -22, 2.0 ** -25))
