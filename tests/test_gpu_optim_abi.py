"""cim_sgd_multi and cim_adam_multi at the C ABI: the chunk walk they share (csrc/optim_stream.h) on tails, unaligned pointers,
ragged tiles and the elements next to a tensor.

The construction is test_gpu_grad_clip.Case's: one device image per array (p, g, every state array) with 64 poison elements
on either side of every tensor, every array of a tensor at the same element offset of its image; the |max| words of the
matrix-mode tensors live in an image of zeros (an atomicMax of anything next to an array raises a zero; it would leave the
poison pattern, which is larger than every finite |x|, as it is).  Records are built from _lib.STRUCTS.

What is compared is bits.  SGD's values come from a host model: the rule is three fp32 FMAs per element, and `fma32` below is
a correctly rounded fp32 fma (the fp64 product of two fp32 values is exact; TwoSum gives the error of the fp64 sum; the sum
is moved to the neighbour with an odd last bit when it is inexact - round to odd - after which the one rounding to fp32
cannot go wrong: 53 >= 2 * 24 + 2).  Adam's values stay with test_gpu_optim_adam.py.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

POISON = 0x7FA5A5A5          # a NaN bit pattern: a guard element that is read makes NaNs, one that is written changes its bits
GUARD = 64                   # guard elements on either side of every tensor
SIZES = [1, 3, 4, 5, 16383, 16384, 16385]
ODD = 6                      # the 16385 (two chunks) starts at element offset 1 of a 16-byte boundary: the scalar path
MATRICES = [(67, 1028), (2, 8)]     # a full tile + a 3-row tile, a second column tile with only lane 0 inside; remainder loop only
PAIRS = ((0.05, 1e-4), (0.1, 0.0))  # (lr, wd): tensor i takes PAIRS[(i + step) % 2]
MOMENTUM = 0.9
BETAS_EPS = (0.9, 0.999, 1e-8)
RULES = {"sgd": ("cim_sgd_multi", "cim_sgd_tensor", ("buf",)),
         "adam": ("cim_adam_multi", "cim_adam_tensor", ("exp_avg", "exp_avg_sq"))}
FLAT = [(n, 0, 0) for n in SIZES]
MATRIX = [(r * c, r, c) for r, c in MATRICES]


def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise on fp32 arrays (finite, no overflow)."""
    a, b, c = (np.atleast_1d(np.asarray(v, dtype=np.float32)).astype(np.float64) for v in (a, b, c))
    p = a * b                                            # exact: 48 significant bits
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                        # TwoSum: s + err = p + c exactly
    bits = s.view(np.int64)
    away = np.where((err > 0) == (s > 0), 1, -1)         # the other neighbour of the exact sum, in steps of the bit pattern
    bits = np.where((err != 0) & ((bits & 1) == 0), bits + away, bits)
    return bits.view(np.float64).astype(np.float32)


def _round_fraction_to_fp32(x):
    """Round-to-nearest-even of a rational to fp32 (normal range), in integers."""
    if x == 0:
        return np.float32(0.0)
    sign, x, e = (-1 if x < 0 else 1), abs(x), 0
    while x >= 1 << 24:
        x, e = x / 2, e + 1
    while x < 1 << 23:
        x, e = x * 2, e - 1
    n, rem = divmod(x.numerator, x.denominator)
    if 2 * rem > x.denominator or (2 * rem == x.denominator and n & 1):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** e)


def test_fma_model_against_rational_arithmetic():
    rng = np.random.RandomState(5)
    a = (rng.randn(3000) * 10.0 ** rng.randint(-3, 4, 3000)).astype(np.float32)
    b = (rng.randn(3000) * 10.0 ** rng.randint(-3, 4, 3000)).astype(np.float32)
    c = (rng.randn(3000) * 10.0 ** rng.randint(-3, 4, 3000)).astype(np.float32)
    c[:500] = -(a[:500] * b[:500])                       # cancellation: the result is the product's own rounding error
    # sums next to an fp32 half-way point: c + h (1 - i^2 2^-46) with h = half an ulp of c, on either side of the tie and on it.
    # The fp64 sum of these rounds ONTO the tie: a model that rounds twice gets them wrong.
    cc = np.abs(rng.randn(600)).astype(np.float32) + np.float32(1.0)
    h = (np.nextafter(cc, np.float32(np.inf)) - cc).astype(np.float32) * np.float32(0.5)
    i = rng.randint(0, 4, 600).astype(np.float32)
    ta, tb = np.float32(1.0) + i * np.float32(2.0 ** -23), (np.float32(1.0) - i * np.float32(2.0 ** -23)) * h
    below = rng.rand(600) < 0.5                          # c + h - tiny   |   (c + ulp) - h + tiny
    tc = np.where(below, cc, np.nextafter(cc, np.float32(np.inf))).astype(np.float32)
    tb = np.where(below, tb, -tb).astype(np.float32)
    flip = np.where(rng.rand(600) < 0.5, np.float32(-1.0), np.float32(1.0))
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb * flip]), np.concatenate([c, tc * flip])
    got = fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    want = np.array([_round_fraction_to_fp32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert int((naive.view(np.uint32) != want.view(np.uint32)).sum()) > 100      # (the cases do tell the two models apart)


class Case:
    """Tensors `layout` = (numel, rows, cols) each (rows = cols = 0: flat) in one host image per array; `spans` = (first element,
    elements) per tensor, the same in every image.  The values only depend on the seed and the sizes, not on the placement."""

    def __init__(self, layout, rule, odd=(), seed=0):
        rng = np.random.RandomState(seed)
        self.layout, self.rule, self.spans, off = list(layout), rule, [], 0
        for i, (n, _, _) in enumerate(self.layout):
            off = (off + GUARD + 3) & ~3
            if i in odd:
                off += 1
            self.spans.append((off, n))
            off += n
        self.names = ("p", "g") + RULES[rule][2]
        self.images = {k: np.full(off + GUARD, POISON, dtype=np.uint32) for k in self.names}
        self.inside = np.zeros(off + GUARD, dtype=bool)
        for a, n in self.spans:
            self.inside[a:a + n] = True
            for k in self.names:
                v = rng.randn(n) * (0.1 if k == "g" else 1.0)
                self.images[k][a:a + n] = (0.01 * v * v if k == "exp_avg_sq" else v).astype(np.float32).view(np.uint32)
        self.amax_spans, off = [], 0                     # (first word of row_amax, rows, cols); col_amax follows row_amax
        for _, rows, cols in self.layout:
            off += GUARD
            self.amax_spans.append((off, rows, cols))
            off += rows + cols
        self.amax_words = off + GUARD

    def values(self, image):
        return [image[a:a + n] for a, n in self.spans]

    def hyper(self, i, step):
        return PAIRS[(i + step) % 2]

    def run(self, dev, wgs=0, steps=2, call=None):
        """-> {array name: image after `steps` calls, "amax": the |max| words of the LAST step} through the C entry point."""
        from cim_amd import _lib
        from cim_amd.optim import fused
        call = call or _lib.call
        entry, struct, _ = RULES[self.rule]
        bufs = {k: torch.from_numpy(v.view(np.int32).copy()).to(dev) for k, v in self.images.items()}
        amax = torch.zeros(self.amax_words, dtype=torch.int32, device=dev)
        assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
        tab = np.zeros(len(self.layout), dtype=np.dtype(_lib.STRUCTS[struct]))
        for k in self.names:
            tab[k] = [bufs[k].data_ptr() + 4 * a for a, _ in self.spans]
        tab["n"], tab["rows"], tab["cols"] = (list(v) for v in zip(*self.layout))
        tab["row_amax"] = [amax.data_ptr() + 4 * a for a, _, _ in self.amax_spans]
        tab["col_amax"] = [amax.data_ptr() + 4 * (a + rows) for a, rows, _ in self.amax_spans]
        chunks = fused.chunk_table(self.layout)
        dchunks = torch.from_numpy(chunks.view(np.uint8).reshape(-1).copy()).to(dev)
        keep = []
        for step in range(steps):
            lr, wd = (np.array(v) for v in zip(*(self.hyper(i, step) for i in range(len(self.layout)))))
            tab["wd"] = wd
            if self.rule == "sgd":
                tab["lr"], consts = lr, (MOMENTUM,)
            else:
                tab["step_size"], tab["bc2_sqrt"] = lr / (1.0 - BETAS_EPS[0] ** (step + 1)), np.sqrt(1.0 - BETAS_EPS[1] ** (step + 1))
                consts = BETAS_EPS
            keep.append(torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).to(dev))
            amax.zero_()
            call(entry, keep[-1].data_ptr(), dchunks.data_ptr(), len(chunks), *consts, wgs, _lib.stream_ptr())
        torch.cuda.synchronize()
        out = {k: b.cpu().numpy().view(np.uint32) for k, b in bufs.items()}
        out["amax"] = amax.cpu().numpy().view(np.uint32)
        return out

    def check_surroundings(self, out):
        for k in self.names:
            assert np.all(out[k][~self.inside] == POISON), k                     # the guards of every image
        assert np.array_equal(out["g"], self.images["g"])                        # the gradients, bit for bit
        for (a, n), p in zip(self.spans, self.values(out["p"])):
            assert not np.array_equal(p, self.images["p"][a:a + n]), n           # (and every tensor was updated)


CASES = {"flat": lambda rule: Case(FLAT, rule, odd=(ODD,)),
         "flat_moved": lambda rule: Case(FLAT, rule, odd=set(range(len(FLAT))) - {ODD}),      # every tensor 4 bytes from where "flat" has it
         "matrix": lambda rule: Case(MATRIX, rule, seed=1),
         "matrix_as_flat": lambda rule: Case([(n, 0, 0) for n, _, _ in MATRIX], rule, seed=1),
         "mixed": lambda rule: Case(FLAT + MATRIX, rule, odd=(ODD,), seed=2)}
GRIDS = {"mixed": (0, 1, 3)}                             # every other case runs with one workgroup per chunk


@pytest.fixture(scope="module")
def runs():
    """run(kind, rule, wgs=0) -> (case, images after two steps); every combination runs once per module."""
    assert torch.cuda.is_available()
    dev, done = torch.device("cuda:0"), {}

    def run(kind, rule, wgs=0):
        if (kind, rule, wgs) not in done:
            case = CASES[kind](rule)
            done[kind, rule, wgs] = (case, case.run(dev, wgs=wgs))
        return done[kind, rule, wgs]
    return run


@gpu
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_flat_chunks_tails_and_unaligned_tensors(runs, rule):
    case, out = runs("flat", rule)
    assert [a % 4 for a, _ in case.spans] == [0, 0, 0, 0, 0, 0, 1]
    case.check_surroundings(out)
    moved, out_moved = runs("flat_moved", rule)
    assert [a % 4 for a, _ in moved.spans] == [1, 1, 1, 1, 1, 1, 0]
    moved.check_surroundings(out_moved)
    for k in case.names:                                 # 16-byte path and scalar path: the same bits
        for i, (x, y) in enumerate(zip(case.values(out[k]), moved.values(out_moved[k]))):
            assert np.array_equal(x, y), (k, SIZES[i])


@gpu
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_matrix_mode_is_the_flat_update_plus_the_maxima(runs, rule):
    case, out = runs("matrix", rule)
    flat, out_flat = runs("matrix_as_flat", rule)
    case.check_surroundings(out)
    for k in case.names:
        assert np.array_equal(out[k], out_flat[k]), k
    assert not out_flat["amax"].any()                    # flat chunks leave the |max| words alone
    inside = np.zeros(case.amax_words, dtype=bool)
    for (a, rows, cols), p in zip(case.amax_spans, case.values(out["p"])):
        mag = (p & 0x7FFFFFFF).reshape(rows, cols)
        assert np.array_equal(out["amax"][a:a + rows], mag.max(axis=1)), (rows, cols)
        assert np.array_equal(out["amax"][a + rows:a + rows + cols], mag.max(axis=0)), (rows, cols)
        inside[a:a + rows + cols] = True
    assert not out["amax"][~inside].any()                # the words around both arrays


@gpu
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_result_does_not_depend_on_the_grid(runs, rule):
    case, out = runs("mixed", rule, 0)
    case.check_surroundings(out)
    for wgs in GRIDS["mixed"][1:]:
        other = runs("mixed", rule, wgs)[1]
        for k in out:
            assert np.array_equal(out[k], other[k]), (k, wgs)


@gpu
def test_sgd_values_are_the_three_fmas_exactly(runs):
    case, out = runs("mixed", "sgd", 0)
    mom = np.float32(MOMENTUM)
    for i, (a, n) in enumerate(case.spans):
        p, g, buf = (case.images[k][a:a + n].view(np.float32) for k in ("p", "g", "buf"))
        for step in range(2):
            lr, wd = (np.float32(v) for v in case.hyper(i, step))
            buf = fma32(mom, buf, fma32(wd, p, g))
            p = fma32(-lr, buf, p)
        assert np.array_equal(out["buf"][a:a + n], buf.view(np.uint32)), case.layout[i]
        assert np.array_equal(out["p"][a:a + n], p.view(np.uint32)), case.layout[i]
