"""Host model of the pair engine (cim_amd/csrc/gemm_pair.hip, csrc/common.h) and the case table of tests/test_gpu_gemm_pair_abi.py.
NumPy only; tests/test_pair_cases_cpu.py proves on the CPU that every case is exact and that the table reaches every instantiation.

The model: scale_of = cim::pair_scale_of, split = cim::pair_split2 on x * s, encode / decode = the image layout
[row][col / 8][h: 8 x f16 | l: 8 x f16], product = the documented arithmetic (hA.hB + hA.lB + lA.hB) / (sA sB) in float64.

Three operand recipes (all float32) make that arithmetic EXACT in fp32, in any summation order:
  "ints"  small integers on both sides: l == 0 everywhere, the h.h cluster alone carries the result;
  "a_l"   A = a0 + a1 / 4096 (integers a0 in [-2, 2], a1 in [-2, 2] without 0), B in {-1, 0, 1}: lB == 0 and A's split is exact, so
          (hA + lA).hB is the float64 product A @ B - and a missing or misread l.h cluster (lA) is a wrong result;
  "b_l"   the mirror image: pins the h.l cluster (lB).
Why a1 / 4096: at the scale 2^13 (max |A| in [2, 4)) x s = 8192 a0 + 2 a1; fp16 holds multiples of 8 there, so h = 8192 a0 (or its
neighbour at a tie) and l = the remainder, non-zero whenever a0 and a1 are.  (a1 / 1024 gives x s = 8192 a0 + 8 a1: h absorbs it.)
Every element product is then a multiple of one power of two (the granule) and sum |a||b| stays below 2^24 granules at K <= 512."""
import collections

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
RECIPES = ("ints", "a_l", "b_l")
PRODUCTS = (3, 1)                  # every case runs the three-product and the ONEP instantiation
BIAS_MAX = 8                       # |bias| of every exact test: small integers
K_MAX = 512


# ---- the engine's arithmetic ---------------------------------------------------------------------------------------------------

def bits(x):
    """float32 value(s) -> IEEE bit pattern(s)"""
    return np.asarray(x, F32).view(np.uint32)


def scale_of(amax_bits):
    """cim::pair_scale_of: the bit pattern of max |x| -> the power-of-two scale 2^(14 - e); 1 for zero / subnormal / inf / NaN,
    biased exponent of the scale clamped at 253."""
    e = (int(amax_bits) >> 23) & 0xFF
    b = min(268 - e, 253)
    if e == 0 or e == 255:
        b = 127
    return np.array([b << 23], np.uint32).view(F32)[0]


def split(x, s):
    """cim::pair_split2 on x * s (float32 multiply): h = f16_rne(x s), l = f16_rne(x s - h). -> (h, l) float16"""
    xs = np.asarray(x, F32) * F32(s)
    h = xs.astype(F16)
    l = (xs - h.astype(F32)).astype(F16)
    return h, l


def encode(h, l):
    """(h, l) float16 [rows][cols], cols % 8 == 0 -> the image as int32 [rows][cols]: per 8 columns 8 x h then 8 x l"""
    rows, cols = h.shape
    assert cols % 8 == 0
    img = np.stack([h.reshape(rows, cols // 8, 8), l.reshape(rows, cols // 8, 8)], axis=2)
    return np.ascontiguousarray(img).view(np.int32).reshape(rows, cols)


def decode(img):
    """int32 [rows][cols] -> (h, l) float16 [rows][cols]"""
    rows, cols = img.shape
    raw = np.ascontiguousarray(img).view(F16).reshape(rows, cols // 8, 2, 8)
    return raw[:, :, 0, :].reshape(rows, cols).copy(), raw[:, :, 1, :].reshape(rows, cols).copy()


def product(A, sa, B, sb, products=3):
    """The kernel's documented result in float64: A [M][K], B [K][N] float32, scales sa, sb."""
    (ha, la), (hb, lb) = split(A, sa), split(B, sb)
    ha, la, hb, lb = (t.astype(F64) for t in (ha, la, hb, lb))
    acc = ha @ hb
    if products == 3:
        acc = acc + ha @ lb + la @ hb
    else:
        assert products == 1
    return acc / (F64(sa) * F64(sb))


# ---- the case table ------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "form a_mcontig b_kcontig M N K pad_a pad_b pad_c splits batch limit")
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (a_mcontig, b_kcontig) of form 0; form 1 is (1, 0) only


def case_id(c):
    return "f%d-a%db%d-%dx%dx%d-s%d-b%d-l%d" % (c.form, c.a_mcontig, c.b_kcontig, c.M, c.N, c.K, c.splits, c.batch, c.limit)


def _rows_cases():
    """Section 2: for every layout the rows r of the last M-tile that select each slab-loop instantiation (issue: for_valid_subtiles),
    alone (M = r) or behind a full tile (M = tile + r).  An M-contiguous A needs M % 8 == 0."""
    out = []
    shapes = ((8, 32), (72, 64), (264, 96), (36, 160), (520, 32))            # (N, K) walked along the rows
    for am, bk in LAYOUTS:
        rs = (8, 40, 72, 104, 128, 136, 168, 200, 232, 256) if am else (5, 33, 72, 100, 128, 129, 161, 199, 250, 256)
        for i, r in enumerate(rs):
            N, K = shapes[i % len(shapes)]
            if not bk and N % 8:
                N += 4
            pad = 8 * (i % 2)                                                # every other case: leading dimensions beyond the extent
            out.append(Case(0, am, bk, r + 256 * (i % 2), N, K, pad, pad, 4 * (i % 3), 1, 1, 0))
    for i, r in enumerate((8, 40, 72, 104, 120, 128)):                       # form 1: 128-row tiles, MIV = ceil(r / 32)
        N, K = shapes[i % len(shapes)]
        if N % 8:
            N += 4
        out.append(Case(1, 1, 0, r + 128 * (i % 3), N, K, 8 * (i % 2), 8 * (i % 2), 4 * (i % 3), 1, 1, 0))
    return out


def _column_cases():
    """Section 3: N % 8 == 4, which the ABI admits for a K-contiguous B only, below and just above one 256-column tile.  (None of the
    six values is a multiple of 8: an N-contiguous B gets its ragged columns from ROW_CASES - N = 8, 40, 72, 264, 520.)"""
    out = []
    for N in (4, 12, 36, 100, 252, 260):
        for am, bk in LAYOUTS:
            if bk or N % 8 == 0:
                out.append(Case(0, am, bk, 40, N, 64, 0, 8, 4, 1, 1, 0))
    return out


def _split_cases():
    """Section 5: forced split counts.  K = 160 is 5 slabs (4 -> 2 + 2 + 1: a short last split; 8 and 16 > slabs: clamped), K = 512 is
    16 (3 -> 6 + 6 + 4, 5 -> 4 + 4 + 4 + 4 after the clamp, 19 > slabs); odd counts walk the reduce's four-at-a-time loop raggedly."""
    out = []
    for K in (160, 512):
        slabs = K // 32
        for s in sorted({2, 3, 4, 5, slabs, slabs + 3, 16}):
            for form, (am, bk) in [(0, l) for l in LAYOUTS] + [(1, (1, 0))]:
                out.append(Case(form, am, bk, 296, 264, K, 8, 8, 4, s, 1, 0))
    return out


def _batch_cases():
    """Section 7: both branches of pair_tile_map (whole slices per XCD from 8 entries on, the rest remapped inside its slice), N > M
    (tile_m fastest) and M > N, chunked launches."""
    out = []
    for batch in (7, 8, 9, 17):
        for limit in (0, 1, 3):
            out.append(Case(0, 0, 0, 264, 8, 64, 8, 8, 4, 1, batch, limit))
            out.append(Case(0, 1, 1, 40, 520, 32, 8, 8, 4, 1, batch, limit))
            out.append(Case(1, 1, 0, 136, 264, 64, 8, 8, 4, 1, batch, limit))
    return out


ROW_CASES = _rows_cases()
COLUMN_CASES = _column_cases()
SPLIT_CASES = _split_cases()
BATCH_CASES = _batch_cases()
CASES = ROW_CASES + COLUMN_CASES + SPLIT_CASES + BATCH_CASES


def tile_rows(c):
    return 128 if c.form == 1 else 256


def last_rows(c):
    """r: the rows of the case's last M-tile, 1 .. 256 (form 0) or 1 .. 128 (form 1)"""
    t = tile_rows(c)
    return (c.M - 1) % t + 1


def instantiations(c):
    """The (wm, MIV) slab loops the case runs, by the kernel's formulas: form 0 - wm = 0: min(4, ceil(r / 32)); wm = 1: idle (MIV 0)
    for r <= 128, else ceil((r - 128) / 32); form 1 - one row of waves, ceil(r / 32).  A full tile in front adds MIV = 4."""
    t, r = tile_rows(c), last_rows(c)
    got = set()
    if c.M > t:
        got |= {(0, 4)} | ({(1, 4)} if c.form == 0 else set())
    got.add((0, min(4, -(-r // 32))))
    if c.form == 0:
        got.add((1, 0) if r <= 128 else (1, -(-(r - 128) // 32)))
    return got


def effective_splits(c):
    """launch_pair: the count clamped to the slabs, whole slabs per split, then the splits that hold work."""
    slabs = c.K // 32
    s = max(1, min(c.splits, slabs))
    per = -(-slabs // s)
    return -(-slabs // per), per


# ---- operands ------------------------------------------------------------------------------------------------------------------

def _ints(rng, shape, lo, hi):
    return rng.randint(lo, hi + 1, size=shape).astype(F32)


def _fine(rng, shape):
    """a0 + a1 / 4096 with a0 in [-2, 2], a1 in {-2, -1, 1, 2} (l != 0 wherever a0 != 0: four elements in five), max |.| forced
    into [2, 4) so that the scale is 2^13"""
    a1 = _ints(rng, shape, 1, 2) * (1 - 2 * _ints(rng, shape, 0, 1))
    x = _ints(rng, shape, -2, 2) + a1 / F32(4096)
    x.flat[0] = F32(2) + F32(1) / F32(4096)
    return x.astype(F32)


def operands(c, recipe, z=0):
    """A [M][K], B [K][N] float32 of batch entry z.  Deterministic in (case, recipe, z)."""
    seed = (c.form * 7 + c.a_mcontig * 3 + c.b_kcontig) * 1000003 + c.M * 8191 + c.N * 131 + c.K + 17 * c.splits + RECIPES.index(recipe) * 977 + z * 101
    rng = np.random.RandomState(seed % (2 ** 31))
    if recipe == "ints":
        return _ints(rng, (c.M, c.K), -4, 4), _ints(rng, (c.K, c.N), -4, 4)
    if recipe == "a_l":
        return _fine(rng, (c.M, c.K)), _ints(rng, (c.K, c.N), -1, 1)
    assert recipe == "b_l"
    return _ints(rng, (c.M, c.K), -1, 1), _fine(rng, (c.K, c.N))


def natural_scale(x):
    """The scale cim_pair_amax + cim_pair_scales derive from the data"""
    return scale_of(bits(np.abs(x).max()))


def entry_scales(c, recipe, z, A, B):
    """One scale per batch entry: the natural one, and for the integer recipe of a batched case a different power of two per entry
    (|x| <= 4: x s stays an fp16 integer up to 2^12)."""
    if c.batch > 1 and recipe == "ints":
        return F32(2.0 ** (z % 12)), F32(2.0 ** ((5 * z + 3) % 12))
    return natural_scale(A), natural_scale(B)


def granule(h, l):
    """The largest power of two that divides every element of h and l (float64; 0 when all are zero)"""
    v = np.concatenate([np.abs(h.astype(F64)).ravel(), np.abs(l.astype(F64)).ravel()])
    v = v[v != 0]
    if v.size == 0:
        return 0.0
    ints = (v * 2.0 ** 40).astype(np.int64)           # scaled to integers (|v| <= 2^15, granules >= 2^-24 here: exact); lowest set bit
    assert np.all(ints.astype(F64) == v * 2.0 ** 40)
    low = np.bitwise_and(ints, -ints).min()
    return float(low) / 2.0 ** 40
