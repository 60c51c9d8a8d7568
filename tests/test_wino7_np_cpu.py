"""No GPU: tests/golden/wino7_np.py - the table-free reference of tests/test_gpu_wino7_abi.py - is sound.  A stand-in for the
kernels' responses is derived HERE, in exact fractions, by Toom-Cook from the points {0, 1, -1, 2, -1/2, inf} (4-wide tile) and
{0, 1, -1, 2, inf} (3-wide tile); it shares no table with cim_amd/csrc.  Shown: the identities hold for the stand-in under the
stated bound, the delta tensor is what torch.nn.functional.conv2d computes on impulses, and each of four defects - an entry off by
2^-12, a shifted tile origin, two swapped positions, (h, w, c) instead of (c, h, w) - fails the check that is there to catch it."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wino7_np as wn
from wino7_np import F32, F64

INF = None
POINTS = ((Fraction(0), Fraction(1), Fraction(-1), Fraction(2), Fraction(-1, 2), INF), (Fraction(0), Fraction(1), Fraction(-1), Fraction(2), INF))
OUTS = (4, 3)               # outputs per axis of the two tile kinds
OUT0 = (0, 4)               # first output row / column; the patch starts one before it (padding 1)


# ---- Toom-Cook in fractions ---------------------------------------------------------------------------------------------------

def _vander(points, k):
    """[n][k]: row of a finite point p is (1, p, .., p^(k-1)); of infinity (0, .., 0, 1): the leading coefficient"""
    return [[(Fraction(int(j == k - 1)) if p is INF else p ** j) for j in range(k)] for p in points]


def _inverse(A):
    n = len(A)
    M = [list(row) + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def _f(rows):
    """fractions -> the float32 value of each entry (what a table holds), as float64"""
    return np.array([[float(v) for v in r] for r in rows], F64).astype(F32).astype(F64)


def _axis(kind):
    """The 1-D correlation F(m, 3) with n = m + 2 points is the transpose of the polynomial product s = V^-1 [(V_3 g) . (V_m d)]:
    y = V_m^T [(V_3 g) . (V^-T x)].  -> A^T [m][n], G [n][3], B^T [n][n], and of the weight gradient dw = V_3^T [(V_m dy) . (V^-T x)]
    GD [n][m], AW [3][n]."""
    pts, m = POINTS[kind], OUTS[kind]
    n = len(pts)
    assert n == m + 2
    Vinv = _inverse(_vander(pts, n))
    # the free diagonal between the two factors of a position: the Lagrange denominator of each finite point goes to the g / dy
    # side, so that B^T (and with it every response but Tfil and Tgd) is dyadic
    den = [Fraction(1)] * n
    for r, p in enumerate(pts):
        for o in pts:
            if p is not INF and o is not INF and o != p:
                den[r] *= p - o
    BT = [[Vinv[c][r] * den[r] for c in range(n)] for r in range(n)]
    Vm, V3 = ([[v / den[r] for v in row] for r, row in enumerate(_vander(pts, k))] for k in (m, 3))
    # (A^T and AW below are the unscaled Vandermonde columns)
    AT, AW = _vander(pts, m), _vander(pts, 3)
    return dict(AT=_f([[AT[p][a] for p in range(n)] for a in range(m)]), G=_f(V3), BT=_f(BT), GD=_f(Vm),
                AW=_f([[AW[p][a] for p in range(n)] for a in range(3)]), n=n, m=m)


def _stand_in(in0=(OUT0[0] - 1, OUT0[1] - 1), tweak=None):
    """The seven responses of wino7_np's docstring for the mixed tiling, positions in the order (4, 4), (4, 3), (3, 4), (3, 3) of the
    tile kinds per axis, row-major inside a tile.  in0: first patch row / column per kind; tweak(axes): edit the 1-D matrices."""
    axes = [_axis(0), _axis(1)]
    if tweak is not None:
        tweak(axes)
    one = []
    for k, ax in enumerate(axes):
        n, m = ax["n"], ax["m"]
        tin, tgd, tout = np.zeros((n, 7)), np.zeros((n, 7)), np.zeros((7, n))
        for pix in range(7):
            if 0 <= pix - in0[k] < n:
                tin[:, pix] = ax["BT"][:, pix - in0[k]]
        tgd[:, OUT0[k]:OUT0[k] + m] = ax["GD"]
        tout[OUT0[k]:OUT0[k] + m, :] = ax["AT"]
        one.append(dict(tin=tin, tgd=tgd, tout=tout, tfil=ax["G"], taw=ax["AW"]))
    kinds = [(0, 0), (0, 1), (1, 0), (1, 1)]
    cat = lambda name, axis: np.concatenate([np.kron(one[a][name], one[b][name]) for a, b in kinds], axis=axis)
    T = dict(Tin=cat("tin", 0), Tfil=cat("tfil", 0), Tgd=cat("tgd", 0), Tout=cat("tout", 1), Taw=cat("taw", 1))
    T["Tadj"], T["Tdx"] = T["Tout"].T.copy(), T["Tin"].T.copy()
    assert T["Tin"].shape == (121, 49) and T["Tout"].shape == (49, 121) and T["Tfil"].shape == (121, 9) and T["Taw"].shape == (9, 121)
    return T


@pytest.fixture(scope="module")
def T():
    return _stand_in()


# ---- the reference is sound -------------------------------------------------------------------------------------------------------

def test_delta_is_conv2d_on_impulses():
    x = torch.eye(49, dtype=torch.float64).reshape(49, 1, 7, 7)
    w = torch.eye(9, dtype=torch.float64).reshape(9, 1, 3, 3)
    y = F.conv2d(x, w, padding=1).reshape(49, 9, 49).permute(2, 0, 1)          # [o][i][t]
    assert np.array_equal(y.numpy(), wn.conv_delta())
    assert wn.conv_delta().sum() == 9 * 49 - 2 * 3 * 7 * 2 + 4                 # 3 x 3 windows clipped by the map's border


def test_identities_hold_for_the_stand_in(T):
    fwd = wn.check_identity(wn.forward_sums(T["Tout"], T["Tin"], T["Tfil"]), "forward")
    wg = wn.check_identity(wn.wgrad_sums(T["Taw"], T["Tin"], T["Tgd"]), "weight gradient")
    assert fwd < 1.0 and wg < 1.0               # float32 entries, float64 sums: table rounding alone is below one 2^-24 K
    wn.check_adjoint(T["Tadj"], T["Tout"], T["Tdx"], T["Tin"])


def test_the_linear_model_is_the_convolution_and_its_gradients(T):
    """The composite of the stand-in's stages through wino7_np's apply functions against conv2d and autograd in float64"""
    rng = np.random.RandomState(0)
    R, C, Co = 3, 4, 5
    x = torch.tensor(rng.randn(R, C, 7, 7), requires_grad=True)
    w = torch.tensor(rng.randn(Co, C, 3, 3), requires_grad=True)
    y = F.conv2d(x, w, padding=1)
    dy = torch.tensor(rng.randn(*y.shape))
    y.backward(dy)
    cl = lambda t: t.detach().permute(0, 2, 3, 1).reshape(R, 49, -1).numpy()   # channels-last [R][49][C]
    V = wn.to_positions(T["Tin"], cl(x))                                       # [121][R][C]
    U = wn.filter_positions(T["Tfil"], w.detach().reshape(Co, C, 9).numpy())   # [121][Co][C]
    got = wn.from_positions(T["Tout"], np.einsum("qrc,qoc->qro", V, U))
    assert np.abs(got - cl(y)).max() < 1e-5
    E = wn.to_positions(T["Tadj"], cl(dy))                                     # [121][R][Co]
    dx = wn.from_positions(T["Tdx"], np.einsum("qro,qoc->qrc", E, U))
    assert np.abs(dx - cl(x.grad)).max() < 1e-5
    D = wn.to_positions(T["Tgd"], cl(dy))
    dW = wn.wgrad_from_positions(T["Taw"], np.einsum("qrc,qro->qco", V, D))     # dU [121][Cin][Cout]
    assert np.abs(dW - w.grad.reshape(Co, C, 9).numpy()).max() < 1e-5


def test_stand_in_meets_the_exact_data_precondition(T):
    for name in ("Tin", "Tout", "Tadj", "Tdx", "Taw"):
        wn.check_dyadic(T[name], name)
    with pytest.raises(AssertionError):
        wn.check_dyadic(T["Tfil"], "Tfil")          # thirds: the filter stage is held to a bound instead


def test_flatten_definitions_are_the_nchw_view():
    rng = np.random.RandomState(1)
    R, PP, C = 2, 49, 3
    src = rng.randn(R, PP, C).astype(F32)                                   # channels-last [R][7][7][C]
    nchw = torch.from_numpy(src).reshape(R, 7, 7, C).permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(wn.flatten_chw(src), nchw.view(R, -1).numpy())
    y = rng.randn(R, PP, C).astype(F32)
    y[0, 0, 0], y[0, 1, 0] = 0.0, -0.0
    flat = torch.from_numpy(wn.flatten_chw(src)).requires_grad_()
    g = rng.randn(R, C * PP).astype(F32)
    dst, bsum = wn.flatten_chw_bwd(g, y, PP, C)
    yt = torch.from_numpy(y)
    want = torch.from_numpy(g).view(R, C, PP).permute(0, 2, 1) * (yt > 0)
    assert np.array_equal(dst, want.numpy()) and dst[0, 0, 0] == 0 and dst[0, 1, 0] == 0
    assert np.array_equal(bsum, dst.astype(F64).sum(axis=1))
    plain, _ = wn.flatten_chw_bwd(g, None, PP, C)
    assert np.array_equal(wn.flatten_chw(plain), g)                          # without a mask: the inverse permutation


def test_layouts_hold_every_impulse():
    x = wn.act_impulses()
    assert x.sum() == 49 and all(x[r, r, r % 8] == 1 for r in range(49))
    W = wn.filter_impulses()
    assert np.all(W.sum(axis=2) == 1) and set(wn.filter_taps().ravel()) == set(range(9))
    assert np.all(np.bincount(wn.filter_taps().ravel()) >= 2)
    M = wn.pos_impulses(31, 4)
    assert M.sum() == 121 and M[7, 1, 3] == 1 and M[120, 30, 0] == 1
    # a response laid out as the kernels do reads back as the matrix
    Tt = np.arange(49 * 121, dtype=F64).reshape(49, 121)
    assert np.array_equal(wn.pos_response(wn.from_positions(Tt, M)), Tt)
    Tq = np.arange(121 * 49, dtype=F64).reshape(121, 49) + 1
    d = np.zeros((121, 64, 8))
    d[:, :49, :] = wn.to_positions(Tq, x)
    assert np.array_equal(wn.act_response(d), Tq)
    d[5, 50, 0] = 1.0                                                         # a word in a pad row
    with pytest.raises(AssertionError):
        wn.act_response(d)
    Tf = np.arange(121 * 9, dtype=F64).reshape(121, 9)
    assert np.array_equal(wn.filter_response(wn.filter_positions(Tf, W)), Tf)


def test_worst_case_attains_the_row_sum(T):
    for name in ("Tin", "Tgd", "Tadj", "Tfil"):
        x = wn.worst_case(T[name])
        assert np.abs(x).max() == 3 and np.allclose((T[name] * x).sum(axis=1), 3 * np.abs(T[name]).sum(axis=1))
    assert wn.is_power_of_two([0.25, 1.0, 2.0 ** 13]) and not wn.is_power_of_two([3.0])


# ---- negative controls: each defect fails its check --------------------------------------------------------------------------------

def test_an_entry_off_by_2_to_minus_12_fails(T):
    def tweak(axes):
        axes[1]["AT"][2][4] += 2.0 ** -12
    bad = _stand_in(tweak=tweak)
    with pytest.raises(AssertionError, match="forward"):
        wn.check_identity(wn.forward_sums(bad["Tout"], bad["Tin"], bad["Tfil"]), "forward")

    def tweak_gd(axes):
        axes[0]["GD"][3][1] += 2.0 ** -12
    bad = _stand_in(tweak=tweak_gd)
    with pytest.raises(AssertionError, match="weight gradient"):
        wn.check_identity(wn.wgrad_sums(bad["Taw"], bad["Tin"], bad["Tgd"]), "weight gradient")
    wn.check_identity(wn.forward_sums(bad["Tout"], bad["Tin"], bad["Tfil"]), "forward")      # (the forward does not use GD)


def test_a_shifted_tile_origin_fails(T):
    bad = _stand_in(in0=(-1, 4))
    with pytest.raises(AssertionError, match="forward"):
        wn.check_identity(wn.forward_sums(bad["Tout"], bad["Tin"], bad["Tfil"]), "forward")
    with pytest.raises(AssertionError, match="weight gradient"):
        wn.check_identity(wn.wgrad_sums(bad["Taw"], bad["Tin"], bad["Tgd"]), "weight gradient")
    with pytest.raises(AssertionError):
        wn.check_adjoint(T["Tadj"], T["Tout"], bad["Tdx"], T["Tin"])


def test_two_swapped_positions_fail(T):
    Tin = T["Tin"].copy()
    Tin[[36, 66]] = Tin[[66, 36]]                   # the first positions of the (4, 3) and the (3, 4) tile
    with pytest.raises(AssertionError, match="forward"):
        wn.check_identity(wn.forward_sums(T["Tout"], Tin, T["Tfil"]), "forward")
    with pytest.raises(AssertionError, match="weight gradient"):
        wn.check_identity(wn.wgrad_sums(T["Taw"], Tin, T["Tgd"]), "weight gradient")
    with pytest.raises(AssertionError):
        wn.check_adjoint(T["Tadj"], T["Tout"], T["Tdx"], Tin)


def test_hwc_order_instead_of_chw_fails():
    rng = np.random.RandomState(2)
    R, PP, C = 2, 49, 64
    src = wn.ints(rng, (R, PP, C))
    hwc = src.reshape(R, PP * C)                     # what a flatten that keeps (h, w, c) order writes
    assert not np.array_equal(hwc, wn.flatten_chw(src))
    g = wn.ints(rng, (R, C * PP))
    dst, _ = wn.flatten_chw_bwd(g, None, PP, C)
    assert not np.array_equal(g.reshape(R, PP, C), dst)
