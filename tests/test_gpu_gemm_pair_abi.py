"""-m gpu: the pair engine (cim_amd/csrc/gemm_pair.hip: gemm_pair_kernel, gemm_pair_ring_kernel, pair_splitk_reduce_kernel and the
producers cim_pair_split / cim_pair_scales / cim_pair_amax) straight at the C ABI, on data whose result is EXACT, at every slab-loop
instantiation, with every buffer guarded.  tests/test_gpu_gemm_pair.py holds the same kernels to an error bound on random data; here
every assertion on a value is torch.equal or an integer comparison - this file contains no tolerance - and a failure names the first
wrong (m, n): a wrong sub-tile shows as a band of rows, a wrong plane or swizzle as a pattern in k.

Data (tests/golden/pair_cases.py; tests/test_pair_cases_cpu.py proves it sound without a GPU): "ints" - small integers, l == 0, the
h.h cluster alone; "a_l" / "b_l" - one side a0 + a1 / 4096 whose split is exact and whose l is non-zero in four elements of five, the
other side in {-1, 0, 1}: the three products are then the plain float64 product A @ B, and the l.h resp. h.l cluster is pinned on its
own.  Every partial sum is a whole number of granules below 2^24: fp32 accumulation is exact in any order, at any split count.
The references are pair_cases.product (the documented arithmetic in float64: products = 1 has a reference of its own, not "form 0 ==
form 1") and, where it must agree, A @ B in float64.

Guards, on every call of this file: operand images are built on the host (pair_cases.encode; section 1 shows cim_pair_split writes the
same bytes) inside buffers filled with fp16 NaN - the pad rows up to pad32(rows) zero as the contract says, NaN in the gaps lda / ldb >
extent, between batch entries and on both sides; C inside sentinel memory (abi_guards._Out, base only 4-byte aligned while no reduce
runs: the epilogue's stores are scalar), a batched C with c_bs > M ldc; the split-K workspace NaN until written.
What the poison can and cannot show: NaN in the M / N gaps does NOT reveal an over-read there - the stagers clamp rows and chunks to
the matrix, and a clamped read feeds accumulators that the epilogue discards.  What it catches is a read past the K extent (a split's
range, the ring kernel's re-read slabs past the last one, a K-contiguous row read beyond K into the gap) and ANY store outside the
result."""
import numpy as np
import pytest
import torch

import pair_cases as pc
from abi_guards import GUARD, NAN, SENT, _Out, _Ws, _same          # tests/golden/abi_guards.py
from pair_cases import F32, F64, Case

pytestmark = pytest.mark.gpu

F16_NAN2 = 0x7E007E00        # two fp16 quiet NaNs: what every int32 of an image buffer holds outside the image


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- helpers ---------------------------------------------------------------------------------------------------------------------

def _pad32(n):
    return (n + 31) & ~31


def _bits(x):
    return int(pc.bits(x))


class _Image:
    """The pair images of the stored matrices `mats` ([batch] x float32 [rows][cols], cols % 8 == 0) written with `scales`:
    [batch][pad32(rows)][cols + pad] int32 with `gap` more between entries, pad rows zero, fp16 NaN everywhere else."""

    def __init__(self, mats, scales, pad, gap, dev):
        rows, cols = mats[0].shape
        assert cols % 8 == 0 and pad % 8 == 0 and gap % 8 == 0
        rp = _pad32(rows)
        self.ld, self.bs = cols + pad, rp * (cols + pad) + gap
        buf = np.full(GUARD + len(mats) * self.bs + GUARD, F16_NAN2, np.int32)
        for z, (x, s) in enumerate(zip(mats, scales)):
            v = buf[GUARD + z * self.bs:GUARD + z * self.bs + rp * self.ld].reshape(rp, self.ld)
            v[:rows, :cols] = pc.encode(*pc.split(x, s))
            v[rows:, :cols] = 0
        self.buf = torch.from_numpy(buf).to(dev)
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.ptr % 32 == 0


class _OutBatch:
    """[batch][M][N] with leading dimension N + pad and batch stride M ld + gap, every float preset to SENT.  Base 16-byte aligned + 4 shift."""

    def __init__(self, batch, M, N, pad, gap, dev, shift=1):
        self.batch, self.M, self.N, self.ld, self.bs = batch, M, N, N + pad, M * (N + pad) + gap
        assert self.bs % 4 == 0
        self.front = (2 * self.ld + GUARD + 3) // 4 * 4 + shift
        self.raw = torch.full((self.front + batch * self.bs + GUARD,), SENT, dtype=torch.int32, device=dev)
        self.view = self.raw.view(torch.float32).as_strided((batch, M, N), (self.bs, self.ld, 1), self.front)
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == 4 * shift

    def check(self):
        got = self.view.clone()
        assert bool(torch.isfinite(got).all()), "an element of the result was not written (or is not finite)"
        rest = self.raw.clone()
        rest.as_strided((self.batch, self.M, self.N), (self.bs, self.ld, 1), self.front).fill_(SENT)
        assert bool((rest == SENT).all()), "a store outside [batch][M][N]: %d floats changed" % int((rest != SENT).sum())
        return got


def _stored(c, A, B):
    """The logical A [M][K], B [K][N] as the matrices the images hold: a_mcontig: [K][M], else [M][K]; b_kcontig: [N][K], else [K][N]"""
    return (np.ascontiguousarray(A.T) if c.a_mcontig else A), (np.ascontiguousarray(B.T) if c.b_kcontig else B)


def _dev64(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F64)).to(dev)


def _case_data(c, recipe):
    """-> per batch entry (A, B, sa, sb)"""
    out = []
    for z in range(c.batch):
        A, B = pc.operands(c, recipe, z)
        out.append((A, B) + tuple(pc.entry_scales(c, recipe, z, A, B)))
    return out


def _gemm(dev, c, data, products, bias=None, relu=False, amax_word=None, splits=None):
    """One product of the case `c` on `data` (_case_data) through cim_gemm_pair / cim_gemm_pair_batched with every guard of the module
    docstring.  -> (C [M][N] or [batch][M][N] on the device, the c_amax word afterwards or None)"""
    from cim_amd import _lib
    splits = c.splits if splits is None else splits
    sa = torch.tensor([float(d[2]) for d in data], dtype=torch.float32, device=dev)
    sb = torch.tensor([float(d[3]) for d in data], dtype=torch.float32, device=dev)
    st = [_stored(c, d[0], d[1]) for d in data]
    gap = 8 * (c.batch > 1)
    ia = _Image([s[0] for s in st], [d[2] for d in data], c.pad_a, gap, dev)
    ib = _Image([s[1] for s in st], [d[3] for d in data], c.pad_b, 3 * gap, dev)
    if c.batch > 1:
        assert bias is None and not relu and amax_word is None and splits == 1
        out = _OutBatch(c.batch, c.M, c.N, c.pad_c, 12, dev)
        _lib.call("cim_gemm_pair_batched", ia.ptr, ib.ptr, out.ptr, c.M, c.N, c.K, ia.ld, ib.ld, out.ld, c.a_mcontig, c.b_kcontig,
                  c.batch, ia.bs, ib.bs, out.bs, sa.data_ptr(), sb.data_ptr(), c.limit, products, c.form, _lib.stream_ptr())
        torch.cuda.synchronize()
        return out.check(), None
    reduce_runs = min(splits, c.K // 32) > 1
    out = _Out(c.M, c.N, c.pad_c, dev, shift=0 if reduce_runs else 1)
    ws = _Ws(splits * c.M * c.N, dev, shift=0) if splits > 1 else None
    b = None
    if bias is not None:                                   # between NaN floats, 16-byte aligned (the reduce reads it as float4)
        b = torch.full((GUARD + c.N + GUARD,), NAN, dtype=torch.float32, device=dev)
        b[GUARD:GUARD + c.N] = torch.from_numpy(bias).to(dev)
    word = None if amax_word is None else torch.tensor([amax_word], dtype=torch.int32, device=dev)
    _lib.call("cim_gemm_pair", ia.ptr, ib.ptr, out.ptr, None if b is None else b.data_ptr() + 4 * GUARD, c.M, c.N, c.K, ia.ld, ib.ld,
              out.ld, c.a_mcontig, c.b_kcontig, int(relu), splits, None if ws is None else ws.ptr, sa.data_ptr(), sb.data_ptr(),
              _lib.ptr(word), c.limit, products, c.form, _lib.stream_ptr())
    torch.cuda.synchronize()
    if ws is not None:
        ws.check()
    return out.check(), (None if word is None else int(word.item()))


def _want(data, products, bias=None, relu=False):
    """float64 [M][N] or [batch][M][N]: pair_cases.product (+ bias)(ReLU)"""
    res = []
    for A, B, sa, sb in data:
        w = pc.product(A, sa, B, sb, products)
        if bias is not None:
            w = w + bias.astype(F64)
        res.append(np.maximum(w, 0.0) if relu else w)
    return res[0] if len(res) == 1 else np.stack(res)


def _check_case(dev, c, recipes=pc.RECIPES, **kw):
    """Every recipe x product count of one case against both references."""
    for recipe in recipes:
        data = _case_data(c, recipe)
        for products in pc.PRODUCTS:
            got, _ = _gemm(dev, c, data, products, **kw)
            what = "%s, recipe %s, products %d" % (pc.case_id(c), recipe, products)
            _same(got, _dev64(_want(data, products), dev), what)
            if products == 3 or recipe == "ints":          # no l on one side: the documented arithmetic IS the plain product
                plain = [d[0].astype(F64) @ d[1].astype(F64) for d in data]
                _same(got, _dev64(plain[0] if len(plain) == 1 else np.stack(plain), dev), what + " against A @ B")


# ---- 1. the split producer, bit for bit ----------------------------------------------------------------------------------------------

def _split_call(dev, X, rows_pad, cols, pad_x, pad_p, gap_x, gap_p, scales, Y=None):
    """cim_pair_split of X [batch][rows][cols] (host float32) with ld = cols + pad_x inside NaN, into sentinel memory with
    ldp = cols + pad_p; relu_y = Y laid out as X.  -> (raw int32 buffer afterwards, the buffer expected from the host model)"""
    from cim_amd import _lib
    batch, rows, _ = X.shape
    ld, ldp = cols + pad_x, cols + pad_p
    x_bs, p_bs = rows * ld + gap_x, rows_pad * ldp + gap_p

    def laid_out(T):
        buf = np.full(GUARD + batch * x_bs + GUARD, np.nan, F32)
        for z in range(batch):
            buf[GUARD + z * x_bs:GUARD + z * x_bs + rows * ld].reshape(rows, ld)[:, :cols] = T[z]
        return torch.from_numpy(buf).to(dev)

    xb = laid_out(X)
    yb = laid_out(Y) if Y is not None else None
    P = torch.full((GUARD + batch * p_bs + GUARD,), SENT, dtype=torch.int32, device=dev)
    sc = torch.tensor([float(s) for s in scales], dtype=torch.float32, device=dev)
    _lib.call("cim_pair_split", xb.data_ptr() + 4 * GUARD, P.data_ptr() + 4 * GUARD, rows, rows_pad, cols, ld, ldp, batch, x_bs, p_bs,
              sc.data_ptr(), None if yb is None else yb.data_ptr() + 4 * GUARD, _lib.stream_ptr())
    torch.cuda.synchronize()
    want = np.full(GUARD + batch * p_bs + GUARD, SENT, np.int32)
    Xm = X if Y is None else np.where(Y > 0, X, F32(0))
    for z in range(batch):
        v = want[GUARD + z * p_bs:GUARD + z * p_bs + rows_pad * ldp].reshape(rows_pad, ldp)
        v[:rows, :cols] = pc.encode(*pc.split(Xm[z], scales[z]))
        v[rows:, :cols] = 0
    return P.cpu().numpy(), want


def _same_image(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d int32 of the image buffer differ, first at %d (GUARD = %d in front): got %#x, want %#x"
                             % (what, bad.size, bad[0], GUARD, int(got[bad[0]]) & 0xFFFFFFFF, int(want[bad[0]]) & 0xFFFFFFFF))


def _float_data(rng, shape):
    """Exponents spread over 2^+-8 (h and l of every size down to fp16 subnormals), exact zeros and -0.0 among them"""
    x = (rng.randn(*shape) * np.exp2(16 * (rng.rand(*shape) - 0.5))).astype(F32)
    x[rng.rand(*shape) < 0.05] = 0.0
    x[rng.rand(*shape) < 0.02] = -0.0
    return x


@pytest.mark.parametrize("batch,rows,rows_pad,cols,pad_x,pad_p,gap_x,gap_p",
                         [(1, 1, 32, 8, 0, 0, 0, 0),                  # one chunk of data, 31 zero rows
                          (1, 32, 32, 264, 0, 0, 0, 0),               # no pad rows, dense both ways
                          (1, 70, 96, 64, 4, 8, 0, 0),                # ld > cols with NaN in the gaps, ldp > cols with sentinel
                          (3, 33, 64, 72, 12, 16, 20, 40),            # batched with gaps in x_bs / p_bs, one scale per entry
                          (2, 5, 5, 8, 0, 0, 0, 0)])                  # rows_pad == rows (the caller pads nothing)
def test_split_image_equals_the_host_model(dev, batch, rows, rows_pad, cols, pad_x, pad_p, gap_x, gap_p):
    """The image is encode(host split) as int32; rows rows .. rows_pad are zero; the gaps of P, the floats between entries and
    everything behind rows_pad keep the sentinel (ONE comparison of the whole buffer says all of it); the NaN around X is not read."""
    rng = np.random.RandomState(rows * 100 + cols + batch)
    X = _float_data(rng, (batch, rows, cols))
    for z in range(batch):          # max |X[z]| in [8^z, 2 * 8^z): another scale in every entry
        X[z] *= np.exp2(3.0 * z - np.floor(np.log2(np.abs(X[z]).max()))).astype(F32)
    scales = [pc.natural_scale(X[z]) for z in range(batch)]
    assert len(set(float(s) for s in scales)) == batch
    got, want = _split_call(dev, X, rows_pad, cols, pad_x, pad_p, gap_x, gap_p, scales)
    _same_image(got, want, "split")
    # relu_y: x where y > 0, +0.0 elsewhere - y = 0.0, -0.0 and negative all mask
    Y = rng.choice(np.array([1.5, 0.0, -0.0, -2.0], F32), size=X.shape)
    got, want = _split_call(dev, X, rows_pad, cols, pad_x, pad_p, gap_x, gap_p, scales, Y)
    _same_image(got, want, "split with relu_y")
    for z in range(batch):          # (the masked image differs from the plain one: the mask was applied)
        assert not np.array_equal(pc.encode(*pc.split(X[z], scales[z])), pc.encode(*pc.split(np.where(Y[z] > 0, X[z], F32(0)), scales[z])))


# ---- 2. exact products at every instantiation --------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", pc.ROW_CASES, ids=pc.case_id)
def test_exact_products_every_instantiation(dev, c):
    """Every (wm, MIV) slab loop of form 0's four layouts and every MIV of form 1 (pair_cases.instantiations; the table's coverage is
    asserted in tests/test_pair_cases_cpu.py) x three recipes x products 3 and 1."""
    _check_case(dev, c)


# ---- 3. ragged columns -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", pc.COLUMN_CASES, ids=pc.case_id)
def test_ragged_columns_exact(dev, c):
    """N % 8 == 4 with a K-contiguous B (the last chunk of a row of C is half a chunk of B's rows), below and above one column tile;
    ldc = N + 4 inside sentinel memory."""
    assert c.pad_c > 0
    _check_case(dev, c)


# ---- 4. guards ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,am,bk", [(0,) + l for l in pc.LAYOUTS] + [(1, 1, 0)])
def test_reads_stay_inside_k_and_stores_inside_the_result(dev, form, am, bk):
    """The K extent at its tightest: K = 32 is ONE slab of the 256 x 256 kernel (nothing to prefetch) and two of the ring's (its
    prologue and every step re-read the last one); K = 96 in two splits is 2 + 1 slabs.  Operands with lda / ldb > extent: behind K
    lies NaN (a K-contiguous row's gap; the row after the last k of the other layout is the buffer's NaN tail)."""
    for K, splits in ((32, 1), (64, 2), (96, 2), (160, 1)):
        _check_case(dev, Case(form, am, bk, 136, 264, K, 8, 8, 4, splits, 1, 0), recipes=("ints", "a_l"))


# ---- 5. forced split counts -----------------------------------------------------------------------------------------------------------

SPLIT_GROUPS = sorted({(c.K, c.form, c.a_mcontig, c.b_kcontig) for c in pc.SPLIT_CASES})


@pytest.mark.parametrize("key", SPLIT_GROUPS, ids=lambda k: "K%d-f%d-a%db%d" % k)
def test_forced_split_counts_exact(dev, key):
    """Split counts the policy never picks (a short last split, more splits than slabs, odd counts through the reduce's four-at-a-time
    walk) with bias + ReLU + c_amax in pair_splitk_reduce_kernel and ldc > N: equal to the one-launch result and to the reference,
    bit for bit; the workspace holds exactly splits * M * N floats and is NaN until written."""
    cases = [c for c in pc.SPLIT_CASES if (c.K, c.form, c.a_mcontig, c.b_kcontig) == key]
    rng = np.random.RandomState(key[0] + key[1])
    for recipe in ("ints", "b_l"):
        data = _case_data(cases[0], recipe)                 # one set of operands for every split count of the group
        bias = rng.randint(-pc.BIAS_MAX, pc.BIAS_MAX + 1, size=cases[0].N).astype(F32)
        want = _dev64(_want(data, 3, bias, True), dev)
        assert bool((want > 0).any()) and bool((want == 0).any())
        one, word1 = _gemm(dev, cases[0], data, 3, bias=bias, relu=True, amax_word=0, splits=1)
        _same(one, want, "splits 1, " + recipe)
        assert word1 == _bits(float(want.max()))
        for c in cases:
            got, word = _gemm(dev, c, data, 3, bias=bias, relu=True, amax_word=0)
            what = "%s, recipe %s" % (pc.case_id(c), recipe)
            _same(got, want, what)
            assert torch.equal(got, one), what
            assert word == _bits(float(want.max())), (what, hex(word))
        got, _ = _gemm(dev, cases[-1], data, 1)             # the ONEP kernel through the reduce, bare
        _same(got, _dev64(_want(data, 1), dev), "products 1, " + pc.case_id(cases[-1]))


# ---- 6. c_amax and degenerate scales -----------------------------------------------------------------------------------------------------

def _ints_data(rng, M, N, K):
    A, B = rng.randint(-3, 4, size=(M, K)).astype(F32), rng.randint(-3, 4, size=(K, N)).astype(F32)
    A[0, 0] = B[0, 0] = 3                                   # (both maxima are 3 whatever rows are overwritten below: scale 2^13)
    return A, B


@pytest.mark.parametrize("form,am,bk", [(0, 0, 1), (0, 1, 0), (1, 1, 0)])
def test_c_amax_word(dev, form, am, bk):
    M, N, K = 296, 264, 64
    c = Case(form, am, bk, M, N, K, 0, 0, 4, 1, 1, 0)
    rng = np.random.RandomState(form * 4 + am * 2 + bk)
    # (m, n) of the planted extreme: inside the first (full) tile, and in the ragged corner tile of both forms
    for m, n in ((7, 9), (M - 1, N - 1)):
        A, B = _ints_data(rng, M, N, K)
        A[m, :], B[:, n] = 3, -3                            # C[m][n] = -9 K: the largest magnitude, negative
        data = [(A, B, pc.natural_scale(A), pc.natural_scale(B))]
        want = _want(data, 3)
        assert want[m, n] == -9 * K and np.abs(want).max() == 9 * K and want.max() < 9 * K
        for splits in (1, 2):
            got, word = _gemm(dev, c, data, 3, amax_word=0, splits=splits)
            _same(got, _dev64(want, dev), "max at (%d, %d), splits %d" % (m, n, splits))
            assert word == _bits(9.0 * K), (m, n, splits, hex(word))
            # a word preset above the result keeps the preset; one preset below is raised
            _, word = _gemm(dev, c, data, 3, amax_word=_bits(1e9), splits=splits)
            assert word == _bits(1e9)
            _, word = _gemm(dev, c, data, 3, amax_word=_bits(0.5), splits=splits)
            assert word == _bits(9.0 * K)
    # a ReLU that zeroes everything: the word keeps the caller's value
    A, B = -np.abs(_ints_data(rng, M, N, K)[0]), np.abs(_ints_data(rng, M, N, K)[1])
    bias = -rng.randint(0, pc.BIAS_MAX + 1, size=N).astype(F32)
    data = [(A, B, pc.natural_scale(A), pc.natural_scale(B))]
    assert _want(data, 3, bias).max() <= 0 and _want(data, 3, bias).min() < 0
    for splits in (1, 2):
        for preset in (0, _bits(0.5)):
            got, word = _gemm(dev, c, data, 3, bias=bias, relu=True, amax_word=preset, splits=splits)
            assert torch.equal(got, torch.zeros_like(got)), splits
            assert word == preset, (splits, hex(word))


@pytest.mark.parametrize("form,am,bk", [(0, 0, 0), (0, 1, 1), (1, 1, 0)])
def test_all_zero_operand_through_the_device_scale_chain(dev, form, am, bk):
    """A ReLU mask that kills a whole gradient: max |A| = 0 -> cim_pair_amax leaves the word 0 -> cim_pair_scales gives 1 (not inf)
    -> cim_pair_split writes zeros -> C is the bias exactly, every element finite, at one split and through the reduce."""
    from cim_amd import _lib
    M, N, K = 136, 40, 64
    st = _lib.stream_ptr()
    rng = np.random.RandomState(3)
    rows, cols = (K, M) if am else (M, K)
    x = torch.zeros(rows, cols, device=dev)
    x[1, 3] = -0.0
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("cim_pair_amax", x.data_ptr(), x.numel(), word.data_ptr(), st)
    sa = torch.full((1,), NAN, device=dev)
    _lib.call("cim_pair_scales", word.data_ptr(), 1, None, sa.data_ptr(), 1, 0, st)
    img = torch.full((_pad32(rows), cols), F16_NAN2, dtype=torch.int32, device=dev)
    _lib.call("cim_pair_split", x.data_ptr(), img.data_ptr(), rows, _pad32(rows), cols, cols, cols, 1, 0, 0, sa.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and float(sa.item()) == 1.0
    assert bool(((img & 0x7FFF7FFF) == 0).all())                                      # +-0 in either half
    B = rng.randint(-4, 5, size=(K, N)).astype(F32)
    sb = pc.natural_scale(B)
    ib = _Image([np.ascontiguousarray(B.T) if bk else B], [sb], 8, 0, dev)
    sbt = torch.tensor([float(sb)], device=dev)
    bias = torch.from_numpy(rng.randint(-pc.BIAS_MAX, pc.BIAS_MAX + 1, size=N).astype(F32)).to(dev)
    for splits in (1, 2):
        out = _Out(M, N, 4, dev, shift=0 if splits > 1 else 1)
        ws = _Ws(splits * M * N, dev, shift=0)
        _lib.call("cim_gemm_pair", img.data_ptr(), ib.ptr, out.ptr, bias.data_ptr(), M, N, K, cols, ib.ld, out.ld, am, bk, 0, splits,
                  ws.ptr, sa.data_ptr(), sbt.data_ptr(), None, 0, 3, form, st)
        torch.cuda.synchronize()
        ws.check()
        _same(out.check(), bias.double().expand(M, N), "splits %d" % splits)


def test_pair_scales_against_scale_of(dev):
    """cim_pair_scales at the special words (0, a subnormal, the smallest normal, inf, NaN, the largest finite value), with `factor`,
    with n > n_amax (the last word serves the rest) and with reduce_all, against pair_cases.scale_of.  Integer comparison."""
    from cim_amd import _lib
    st = _lib.stream_ptr()
    words = [0, 1, 0x007FFFFF, 0x00800000, 15 << 23, 16 << 23, _bits(1e-30), _bits(0.75), _bits(1.0), _bits(3.0), _bits(65504.0),
             0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7F800001]

    def run(ws, n, factor=None, reduce_all=0):
        w = torch.tensor(np.array(ws, np.uint32).view(np.int32), dtype=torch.int32, device=dev)
        f = None if factor is None else torch.tensor(factor, dtype=torch.float32, device=dev)
        out = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device=dev)
        _lib.call("cim_pair_scales", w.data_ptr(), len(ws), _lib.ptr(f), out.data_ptr() + 4 * GUARD, n, reduce_all, st)
        torch.cuda.synchronize()
        assert bool((out[:GUARD] == SENT).all()) and bool((out[GUARD + n:] == SENT).all())
        return out[GUARD:GUARD + n].cpu().numpy()

    def model(ws, n, factor=None, reduce_all=0):
        res = []
        for i in range(n):
            wbits = max(w & 0x7FFFFFFF for w in ws) if reduce_all else ws[min(i, len(ws) - 1)]
            a = np.array([wbits], np.uint32).view(F32)[0]
            if factor is not None:
                with np.errstate(all="ignore"):
                    a = F32(a * F32(factor[i]))
            res.append(_bits(pc.scale_of(_bits(a))))
        return np.array(res, np.int32)

    n = len(words)
    assert np.array_equal(run(words, n), model(words, n))
    assert np.array_equal(run(words[:10], 300), model(words[:10], 300))                        # n > n_amax, more than one block
    # factors: powers of two and not; 2^-126 * 0.5 is subnormal (or flushed: exponent field 0 either way), largest finite * 2 is inf
    factor = [1.0, 2.0, 0.5, 0.5, 3.0, 0.25, 1e10, 49.0, 1.5, 1e-3, 16.0, 2.0, 1.0, 1.0, 2.0]
    assert np.array_equal(run(words, n, factor), model(words, n, factor))
    for ws in ([_bits(0.25), _bits(5.0), _bits(1.0)], [0, 0], [_bits(2.0)] * 122 + [_bits(7.0)] + [_bits(2.0)] * 177,
               [_bits(3.0), 0x7F800000], [0x7FC00000, _bits(3.0)]):
        for m in (1, 5):
            assert np.array_equal(run(ws, m, None, 1), model(ws, m, None, 1)), (len(ws), m)
    f5 = [1.0, 2.0, 0.5, 4.0, 8.0]
    assert np.array_equal(run([_bits(0.25), _bits(5.0)], 5, f5, 1), model([_bits(0.25), _bits(5.0)], 5, f5, 1))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_pair_amax_small_and_ragged_counts(dev, n):
    """n < 4 (no whole float4), n % 4 != 0 (a tail), the maximum in the LAST element and negative, -0.0 present; NaN lies behind the n
    floats: an element read past n would be the maximum."""
    from cim_amd import _lib
    rng = np.random.RandomState(n)
    x = rng.randn(n).astype(F32)
    x[0] = -0.0
    x[n - 1] = -37.5
    buf = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + n] = torch.from_numpy(x).to(dev)
    for preset, want in ((0, _bits(37.5)), (_bits(100.0), _bits(100.0))):
        word = torch.tensor([preset], dtype=torch.int32, device=dev)
        _lib.call("cim_pair_amax", buf.data_ptr() + 4 * GUARD, n, word.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert int(word.item()) == want, (n, hex(int(word.item())))
    buf[GUARD:GUARD + n] = -0.0                              # nothing but -0.0: the word stays zero (a bit pattern of |x|, not of x)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("cim_pair_amax", buf.data_ptr() + 4 * GUARD, n, word.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(word.item()) == 0


# ---- 7. batched order ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", pc.BATCH_CASES, ids=pc.case_id)
def test_batched_order_exact(dev, c):
    """Both branches of pair_tile_map - whole slices per XCD (the first 8 floor(batch / 8) entries) and the remap inside a slice (the
    rest, and everything below 8 entries) - with different data AND a different pair of power-of-two scales in every entry (a tile
    that takes another entry's operands, scale or place in C is wrong), chunked launches, a_bs / b_bs / c_bs with gaps."""
    _check_case(dev, c, recipes=("ints", "a_l") if c.limit == 0 else ("ints",))


# ---- 8. rejections: the argument checks, nothing is launched ------------------------------------------------------------------------------

def test_rejections(dev):
    from cim_amd import _lib
    st = _lib.stream_ptr()
    img = torch.zeros(64 * 64, dtype=torch.int32, device=dev)                  # (zero images: large enough for every shape below)
    one = torch.ones(2, device=dev)
    out = _Out(40, 16, 0, dev, shift=0)
    ws = _Ws(2 * 40 * 16, dev, shift=0)
    bias = torch.zeros(16 + 4, device=dev)
    assert bias.data_ptr() % 16 == 0

    def single(M=40, N=16, K=64, lda=64, ldb=64, ldc=16, am=0, bk=1, splits=1, wsp=None, products=3, form=0, C=out.ptr, b=None):
        _lib.call("cim_gemm_pair", img.data_ptr(), img.data_ptr(), C, b, M, N, K, lda, ldb, ldc, am, bk, 0, splits, wsp, one.data_ptr(),
                  one.data_ptr(), None, 0, products, form, st)

    def batched(a_bs=64 * 64 // 2, c_bs=8 * 16):
        _lib.call("cim_gemm_pair_batched", img.data_ptr(), img.data_ptr(), out.ptr, 8, 16, 64, 64, 64, 16, 0, 1, 2, a_bs, 0, c_bs,
                  one.data_ptr(), one.data_ptr(), 0, 3, 0, st)

    bad = [dict(K=48, lda=48, ldb=48),                       # K % 32 != 0
           dict(N=14),                                       # N % 4 != 0
           dict(lda=68),                                     # lda % 8 != 0
           dict(ldb=68),
           dict(am=1, M=12, lda=16),                         # an M-contiguous A with M % 8 != 0
           dict(bk=0, N=12, ldb=16, ldc=12),                 # an N-contiguous B with N % 8 != 0 (N % 4 == 0)
           dict(ldc=12),                                     # ldc < N
           dict(splits=2, wsp=None),                         # splits > 1 without a workspace
           dict(products=2),
           dict(form=1),                                     # the co-resident form with a forward layout
           dict(form=2, am=1, bk=0, lda=40, ldb=16),
           # the split-K reduce moves float4s: C, the workspace and the bias must be 16-byte aligned when it runs
           dict(splits=2, wsp=ws.ptr, C=out.ptr + 4),
           dict(splits=2, wsp=ws.ptr + 4),
           dict(splits=2, wsp=ws.ptr, b=bias.data_ptr() + 4)]
    for kw in bad:
        with pytest.raises(_lib.CimHipError):
            single(**kw)
    with pytest.raises(_lib.CimHipError):
        batched(a_bs=64 * 64 // 2 + 4)                       # a_bs % 8 != 0
    with pytest.raises(_lib.CimHipError):
        batched(c_bs=8 * 16 + 2)                             # c_bs % 4 != 0
    torch.cuda.synchronize()
    assert bool((out.raw == SENT).all()) and bool(torch.isnan(ws.raw[ws.front:ws.front + ws.n].view(torch.float32)).all())
    ws.check()
    # each refusal above is due to the ONE argument it changes: the unchanged call, and the aligned split call, are accepted
    single()
    single(splits=2, wsp=ws.ptr, b=bias.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.check(), torch.zeros(40, 16, device=dev))
