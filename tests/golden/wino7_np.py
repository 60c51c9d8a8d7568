"""Table-free reference of the Winograd stage kernels (cim_amd/csrc/winograd.hip) for tests/test_gpu_wino7_abi.py.  NumPy only;
tests/test_wino7_np_cpu.py proves it sound without a GPU.  Nothing here knows the transform matrices or the tile geometry: a stage
is described by its MEASURED impulse responses, and the definition of a 3 x 3 convolution with padding 1 on a 7 x 7 map decides
whether they are right.

Responses (q: one of the 121 positions; pixels p = y * 7 + x, taps t = a * 3 + b):
  Tin  [121][49]  input transform        position <- input pixel         Tfil [121][9]   filter transform   position <- tap
  Tout [49][121]  output transform       output pixel <- position        Tgd  [121][49]  dy transform of the weight gradient
  Tadj [121][49]  dy transform of the adjoint data gradient              Tdx  [49][121]  adjoint output     input pixel <- position
  Taw  [9][121]   weight-gradient output tap <- position
Identities (delta[o][i][t] = 1 where input pixel i = output pixel o + tap t - (1, 1) lies inside the map):
  forward          sum_q Tout[o,q] Tin[q,i] Tfil[q,t] = delta        weight gradient  sum_q Taw[t,q] Tin[q,i] Tgd[q,o] = delta
  data gradient    Tadj == Tout^T and Tdx == Tin^T, bit for bit (all four are dyadic)
Bound of the two sums: 2^-21 K element by element, K the same sum over absolute values (exactly 0 where K == 0): the fp32 rounding
of the tables' thirds and fifteenths is at most 0.625 2^-24 K, a measured Tfil / Tgd entry adds one product rounding (2^-24) and
the 22 significant bits of its pair image (2^-22): under 6 2^-24 K in all."""
import numpy as np

import pair_cases as pc

F32, F64 = np.float32, np.float64
NQ, P, PIX, TAPS = 121, 7, 49, 9
IDENTITY_RATIO = 8.0          # 2^-21 in units of 2^-24 K
STAGE_RATIO = 32.0            # 2^-19 in units of 2^-24 sum |T| |x|: 8 (two fp32 stages of <= four terms) + 4 (pair image) + 5 (T itself) < 32
MASK_VALUES = (0.0, 0.5, 1.0, 2.0, -1.0)
INT_MAX = 3                   # integer data: -3 .. 3


def pad32(n):
    return (n + 31) & ~31


# ---- the definition -------------------------------------------------------------------------------------------------------------

def conv_delta():
    """[49 o][49 i][9 t] float64: 1 where i = o + t - (1, 1) inside the 7 x 7 map.  Both identities share it: y[o] = sum x[i] w[t]
    and dW[t] = sum x[i] dy[o] run over the same triples."""
    d = np.zeros((P, P, P, P, 3, 3), F64)
    for oy in range(P):
        for ox in range(P):
            for a in range(3):
                for b in range(3):
                    iy, ix = oy + a - 1, ox + b - 1
                    if 0 <= iy < P and 0 <= ix < P:
                        d[oy, ox, iy, ix, a, b] = 1.0
    return d.reshape(PIX, PIX, TAPS)


def forward_sums(Tout, Tin, Tfil):
    """-> (sum, K) [49 o][49 i][9 t] of the forward identity"""
    Tout, Tin, Tfil = (np.asarray(t, F64) for t in (Tout, Tin, Tfil))
    assert Tout.shape == (PIX, NQ) and Tin.shape == (NQ, PIX) and Tfil.shape == (NQ, TAPS)
    return (np.einsum("oq,qi,qt->oit", Tout, Tin, Tfil), np.einsum("oq,qi,qt->oit", np.abs(Tout), np.abs(Tin), np.abs(Tfil)))


def wgrad_sums(Taw, Tin, Tgd):
    """-> (sum, K) [49 o][49 i][9 t] of the weight-gradient identity"""
    Taw, Tin, Tgd = (np.asarray(t, F64) for t in (Taw, Tin, Tgd))
    assert Taw.shape == (TAPS, NQ) and Tin.shape == (NQ, PIX) and Tgd.shape == (NQ, PIX)
    return (np.einsum("tq,qi,qo->oit", Taw, Tin, Tgd), np.einsum("tq,qi,qo->oit", np.abs(Taw), np.abs(Tin), np.abs(Tgd)))


def check_identity(sums, what):
    """|sum - delta| <= 2^-21 K element by element, sum == 0 exactly where K == 0.  -> the worst |sum - delta| / (2^-24 K)"""
    total, K = sums
    delta = conv_delta()
    dead = K == 0
    assert np.all(total[dead] == 0), "%s: a sum is not 0 where no position connects the triple" % what
    assert np.all(delta[dead] == 0), "%s: no position connects a triple of the convolution: (o, i, t) = %s" % (
        what, np.argwhere(dead & (delta != 0))[0].tolist())
    ratio = np.zeros_like(K)
    ratio[~dead] = np.abs(total - delta)[~dead] / (2.0 ** -24 * K[~dead])
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[worst] <= IDENTITY_RATIO, "%s: |sum - delta| = %.3e at (o, i, t) = %s is %.1f x 2^-24 K (K = %.3f), bound %.0f" % (
        what, abs(total[worst] - delta[worst]), [int(v) for v in worst], ratio[worst], K[worst], IDENTITY_RATIO)
    return float(ratio[worst])


def check_adjoint(Tadj, Tout, Tdx, Tin):
    """The data gradient is the adjoint of the forward, bit for bit"""
    bad = np.argwhere(np.asarray(Tadj) != np.asarray(Tout).T)
    assert bad.size == 0, "Tadj[q][o] != Tout[o][q] at (q, o) = %s" % bad[0].tolist()
    bad = np.argwhere(np.asarray(Tdx) != np.asarray(Tin).T)
    assert bad.size == 0, "Tdx[i][q] != Tin[q][i] at (i, q) = %s" % bad[0].tolist()


def check_dyadic(T, what):
    """The precondition of every exact comparison: entries are whole multiples of 1 / 64 and 3 * (largest absolute row sum) * 64 <
    2^22, so that on integers -3 .. 3 every partial sum (two-stage or not, masked by {0, 0.5, 1, 2, -1} or not) is a whole number
    of one granule below 2^24: fp32 is exact in any order, and so is the 22-bit pair image."""
    T = np.asarray(T, F64)
    assert np.all(T * 64 == np.round(T * 64)), "%s: an entry is not a multiple of 1 / 64: %r" % (what, float(T[(T * 64 != np.round(T * 64))][0]))
    rows = np.abs(T).sum(axis=1).max()
    assert INT_MAX * rows * 64 < 2.0 ** 22, "%s: absolute row sum %g" % (what, rows)


# ---- the float64 linear model ---------------------------------------------------------------------------------------------------

def to_positions(T, x):
    """T [121][n], x [R][n][C] -> [121][R][C] float64   (input / dy transforms: n = 49 pixels)"""
    return np.einsum("qi,ric->qrc", np.asarray(T, F64), np.asarray(x, F64))


def from_positions(T, M):
    """T [n][121], M [121][R][C] -> [R][n][C] float64   (output / adjoint output transforms)"""
    return np.einsum("oq,qrc->roc", np.asarray(T, F64), np.asarray(M, F64))


def filter_positions(T, W):
    """Tfil [121][9], W [Cout][Cin][9] -> U' [121][Cout][Cin]"""
    return np.einsum("qt,oit->qoi", np.asarray(T, F64), np.asarray(W, F64))


def wgrad_from_positions(T, dU):
    """Taw [9][121], dU [121][Cin][Cout] -> dW [Cout][Cin][9]"""
    return np.einsum("tq,qio->oit", np.asarray(T, F64), np.asarray(dU, F64))


def flatten_chw(src):
    """src [R][PP][C] -> [R][C * PP] in (c, p) order: `.view(N, -1)` of the NCHW tensor"""
    R, PP, C = src.shape
    return np.ascontiguousarray(np.transpose(src, (0, 2, 1))).reshape(R, C * PP)


def flatten_chw_bwd(src, y, PP, C):
    """src [R][C * PP], y [R][PP][C] or None -> (dst [R][PP][C] = src[r, c PP + p] where y > 0 else +0.0, bias_partial [R][C] float64)"""
    dst = np.transpose(src.reshape(src.shape[0], C, PP), (0, 2, 1))
    if y is not None:
        assert y.shape == dst.shape
        dst = np.where(y > 0, dst, np.zeros_like(dst))
    dst = np.ascontiguousarray(dst)
    return dst, dst.astype(F64).sum(axis=1)


def mask_fold(dcat, mask):
    """dcat [R][49][2 Cb] float64, mask [R][49] -> dbox [R][49][Cb] = dcat[..., :Cb] + mask * dcat[..., Cb:]"""
    Cb = dcat.shape[2] // 2
    return dcat[..., :Cb] + np.asarray(mask, F64)[..., None] * dcat[..., Cb:]


# ---- pair images ------------------------------------------------------------------------------------------------------------------

def decode_image(words, npos, rows, cols, scale):
    """int32 [npos * rows * cols] -> float64 [npos][rows][cols] = (h + l) / scale[position]; every half must be finite"""
    h, l = pc.decode(np.asarray(words, np.int32).reshape(npos * rows, cols))
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(l)), "a half of the image is infinite or NaN"
    v = (h.astype(F64) + l.astype(F64)).reshape(npos, rows, cols)
    return v / np.asarray(scale, F64).reshape(npos, 1, 1)


def image_floor(scale):
    """The absolute term of a pair image's error at each position: 2^-38 of the position's bound 2^15 / scale.  [121][1][1]"""
    return (2.0 ** -38 * 2.0 ** 15 / np.asarray(scale, F64)).reshape(-1, 1, 1)


def check_stage(got, T_apply, T, x, scale, what):
    """An inexact stage (thirds in its table): |got - sum T x| <= 2^-19 sum |T| |x| + floor element by element.
    T_apply: to_positions or filter_positions.  -> the worst (|error| - floor) / (2^-24 sum |T| |x|)"""
    want, mag = T_apply(T, x), T_apply(np.abs(T), np.abs(x))
    err = np.abs(got - want)
    floor = image_floor(scale)
    over = np.maximum(err - floor, 0.0)
    bad = over > STAGE_RATIO * 2.0 ** -24 * mag
    ratio = np.zeros_like(err)
    live = mag > 0
    ratio[live] = over[live] / (2.0 ** -24 * mag[live])
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert not bad.any(), "%s: %d elements beyond the bound, worst %.1f x 2^-24 sum |T||x| at (q, row, col) = %s: got %r, want %r" % (
        what, int(bad.sum()), ratio[worst], [int(v) for v in worst], float(got[worst]), float(want[worst]))
    return float(ratio[worst])


# ---- impulse layouts ----------------------------------------------------------------------------------------------------------------

ACT_R, ACT_RS, ACT_C = 49, 64, 8          # input and dy stages: ROI r carries pixel r in channel r % C
FIL_COUT, FIL_CIN = 18, 8                 # filter: element (co, ci) carries tap (co + 2 ci) % 9
POS_R, POS_C = 31, 4                      # output and dx: impulse n (position n) in (row, channel) = (n / 4, n % 4); 124 >= 121


def act_impulses():
    """x [49][49][8]"""
    x = np.zeros((ACT_R, PIX, ACT_C), F32)
    for r in range(ACT_R):
        x[r, r, r % ACT_C] = 1.0
    return x


def act_response(d):
    """decoded image [121][64][8] -> T [121][49]; every other element must be exactly 0"""
    assert d.shape == (NQ, ACT_RS, ACT_C)
    r = np.arange(ACT_R)
    T = d[:, r, r % ACT_C].copy()
    rest = d.copy()
    rest[:, r, r % ACT_C] = 0.0
    bad = np.argwhere(rest != 0)
    assert bad.size == 0, "a response outside the impulse's row and channel: (q, row, channel) = %s" % bad[0].tolist()
    return T


def filter_taps():
    """[18][8]: the tap of element (co, ci)"""
    co, ci = np.meshgrid(np.arange(FIL_COUT), np.arange(FIL_CIN), indexing="ij")
    return (co + 2 * ci) % TAPS


def filter_impulses():
    """W [18][8][9]"""
    W = np.zeros((FIL_COUT, FIL_CIN, TAPS), F32)
    taps = filter_taps()
    for co in range(FIL_COUT):
        for ci in range(FIL_CIN):
            W[co, ci, taps[co, ci]] = 1.0
    return W


def filter_response(d):
    """decoded image [121][18][8] -> T [121][9]; elements that share a tap must agree bit for bit"""
    assert d.shape == (NQ, FIL_COUT, FIL_CIN)
    taps = filter_taps()
    T = np.zeros((NQ, TAPS), F64)
    for t in range(TAPS):
        sel = d[:, taps == t]                 # [121][elements of tap t]
        assert sel.shape[1] >= 2
        bad = np.argwhere(sel != sel[:, :1])
        assert bad.size == 0, "two filter elements with tap %d differ at position %d" % (t, bad[0][0] if bad.size else -1)
        T[:, t] = sel[:, 0]
    return T


def pos_impulses(rows, cols):
    """M [121][rows][cols] with M[n].flat[n] = 1 (rows * cols >= 121)"""
    assert rows * cols >= NQ
    M = np.zeros((NQ, rows * cols), F32)
    M[np.arange(NQ), np.arange(NQ)] = 1.0
    return M.reshape(NQ, rows, cols)


def pos_response(y):
    """y [rows][n][cols] (the response of row, col = divmod(q, cols) to position q) -> T [n][121]; slots past 121 exactly 0"""
    rows, n, cols = y.shape
    flat = np.transpose(y, (1, 0, 2)).reshape(n, rows * cols)
    bad = np.argwhere(flat[:, NQ:] != 0)
    assert bad.size == 0, "a response where no impulse was: (pixel, slot) = %s" % (bad[0] + [0, NQ]).tolist()
    return flat[:, :NQ].astype(F64)


# ---- data recipes -----------------------------------------------------------------------------------------------------------------------

def ints(rng, shape):
    """integers -3 .. 3 as float32, the extremes present"""
    x = rng.randint(-INT_MAX, INT_MAX + 1, size=shape).astype(F32)
    x.flat[0], x.flat[-1] = INT_MAX, -INT_MAX
    return x


def randoms(rng, shape):
    """fp32 data of the inexact stages: normal, exponents spread over 2^+-4, a few exact zeros"""
    x = (rng.randn(*shape) * np.exp2(8 * (rng.rand(*shape) - 0.5))).astype(F32)
    x[rng.rand(*shape) < 0.05] = 0.0
    return x


def worst_case(T, amax=float(INT_MAX)):
    """[121][n]: row q is the input that maximises |transformed value| at position q under max |x| = amax: amax * sign(T[q])
    (amax itself where the response is 0: the maximum is attained whatever the rest holds)"""
    s = np.sign(np.asarray(T, F64))
    s[s == 0] = 1.0
    return (amax * s).astype(F32)


def is_power_of_two(s):
    m, _ = np.frexp(np.asarray(s, F64))
    return np.all(m == 0.5)
