"""-m gpu: the backbone GEMM kernels of cim_amd/csrc/conv1x1.hip and the multi-chunk forms of cim_amd/csrc/bn_act.hip where
tests/test_gpu_gemm.py is blind: straight at the C ABI, with every operand inside NaN-poisoned memory (NaN in front, behind and in
the gap between the extent and the leading dimension, base address only 4-byte aligned), every output inside sentinel-guarded
memory, the split-K workspace pre-filled with NaN, at forced split counts (empty splits included), at the geometry limits of the
3 x 3 kernel and at maps of one or two pixels.

Operands are small INTEGERS stored as float32: every product and every partial sum stays far below 2^24 (the largest, section 1:
K = 2047 products of magnitude <= 16), so the fp32 result equals the float64 result bit for bit in ANY summation order, at any
split count and through atomicAdd.  Every assertion on such data is torch.equal; no tolerance can hide a wrong element.  The
"exact" BatchNorm (eps = 0, var = 1, gamma a power of two, beta / mean small integers) keeps the epilogue exact as well.
Tolerances appear only on float (randn) data, and they are the bounds tests/test_gpu_gemm.py already holds the same kernels to."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

from abi_guards import SENT, _Out, _Ws, _poisoned, _same      # tests/golden/abi_guards.py (shared with test_gpu_gemm_pair_abi.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- shared helpers -------------------------------------------------------------------------------------------------------------

def _ints(shape, lo, hi, dev):
    return torch.randint(lo, hi + 1, shape, device=dev).float()


def _pvec(t):
    """A dense tensor of any shape between NaN floats (per-channel vectors, NCHW images, weights)."""
    return _poisoned(t.reshape(1, -1))[0]


def _rel_fro(a, ref):
    return float((a.double() - ref).norm() / (ref.norm() + 1e-30))


def _exact_bn(C, dev):
    """(gamma, beta, mean, var, eps) whose epilogue a = gamma rsqrt(var + eps), y = x a + (beta - mean a) is exact on integers,
    different from row to row."""
    gamma = torch.tensor([0.5, 1.0, 2.0, 4.0], device=dev)[torch.randint(0, 4, (C,), device=dev)]
    gamma = gamma * (1 - 2 * torch.randint(0, 2, (C,), device=dev)).float()
    return gamma, _ints((C,), -3, 3, dev), _ints((C,), -3, 3, dev), torch.ones(C, device=dev), 0.0


def _epilogue64(P, bn, res, relu):
    """float64: relu?(BatchNorm(P) + res) with per-row statistics, P [M][N]."""
    y = P.double()
    if bn is not None:
        gamma, beta, mean, var, eps = bn
        y = (y - mean.double()[:, None]) / torch.sqrt(var.double() + eps)[:, None] * gamma.double()[:, None] + beta.double()[:, None]
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def _bn_ptrs(bn):
    if bn is None:
        return [None, None, None, None, 0.0], []
    keep = [_pvec(v) for v in bn[:4]]
    return [k.data_ptr() for k in keep] + [float(bn[4])], keep


def _gemm(A, B, am, bk, splits, in_pad=0, out_pad=0, bn=None, res=None, relu=False, xraw=False, shift=1, ws_shift=1):
    """cim_gemm_small_f32 of the logical A [M][K], B [K][N] in the layout (a_mcontig, b_kcontig), poisoned operands, guarded
    outputs and workspace.  -> (C, x_raw or None), both checked for stray stores."""
    from cim_amd import _lib
    dev = A.device
    (M, K), N = A.shape, B.shape[1]
    a, lda = _poisoned(A.t() if am else A, in_pad)            # a_mcontig: element (m, k) at A[k * lda + m]
    b, ldb = _poisoned(B.t() if bk else B, in_pad)            # b_kcontig: element (k, n) at B[n * ldb + k]
    C = _Out(M, N, out_pad, dev, shift)
    X = _Out(M, N, out_pad, dev, shift) if xraw else None
    ws = _Ws(splits * M * N, dev, ws_shift)
    bn_args, keep = _bn_ptrs(bn)
    r = _poisoned(res, out_pad)[0] if res is not None else None          # (the residual shares C's leading dimension)
    _lib.call("cim_gemm_small_f32", a.data_ptr(), b.data_ptr(), C.ptr, M, N, K, lda, ldb, C.ld, int(am), int(bk),
              X.ptr if xraw else None, *bn_args, _lib.ptr(r), int(relu), splits, ws.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    ws.check()
    return C.check(), (X.check() if xraw else None)


# ---- 1. cim_gemm_small_f32: layouts x tile width x splits ----------------------------------------------------------------------

GEMM_SHAPES = [(1, 1, 1), (5, 3, 2), (33, 31, 35), (64, 64, 32), (65, 129, 33), (70, 100, 324), (128, 96, 1000), (257, 40, 2047)]
LAYOUTS = list(itertools.product((0, 1), (0, 1)))


def _policy(M, N, K):
    from cim_amd import _lib
    return _lib.call("cim_gemm_small_splits", M, N, K)


def _split_counts(M, N, K):
    return sorted({1, 2, 3, 7, 64, _policy(M, N, K)})


def test_gemm_table_reaches_both_tile_widths(dev):
    """The launcher takes the 64 x 32 tile (128 threads) when tiles * splits < 128 and the 64 x 64 tile otherwise (tiles counted
    in 64 x 64 units, conv1x1.hip gemm_small_impl): the table of section 1 must reach both, and both with splits that do work."""
    forms = {}
    for M, N, K in GEMM_SHAPES:
        tiles = -(-M // 64) * -(-N // 64)
        for s in _split_counts(M, N, K):
            kper = -(-(-(-K // s)) // 32) * 32                                      # ceil(K / s), rounded up to whole slabs
            forms.setdefault(tiles * s < 128, set()).add((s - 1) * kper < K)       # (False: the last split is empty)
    assert forms[True] == {True, False} and forms[False] == {True, False}, forms


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_small_layouts_and_splits_exact(dev, M, N, K):
    """Bare product, four layouts x {ld == extent, ld > extent} x forced split counts (most of them EMPTY splits for these K):
    with ld == extent the floats behind a K tail are the next row's data, with ld > extent they are NaN; ldc in {N, N + 3}."""
    torch.manual_seed(M * 1000 + N + K)
    A, B = _ints((M, K), -4, 4, dev), _ints((K, N), -4, 4, dev)
    want = A.double() @ B.double()
    for (am, bk), padded, s in itertools.product(LAYOUTS, (False, True), _split_counts(M, N, K)):
        in_pad = (1 if am == bk else 3) if padded else 0
        C, _ = _gemm(A, B, am, bk, s, in_pad=in_pad, out_pad=3 if padded else 0)
        _same(C, want, "a_mcontig %d b_kcontig %d ld +%d splits %d" % (am, bk, in_pad, s))


EPILOGUES = [dict(bn=True, xraw=True), dict(res=True), dict(relu=True), dict(bn=True, res=True), dict(bn=True, res=True, relu=True, xraw=True)]


@pytest.mark.parametrize("M,N,K", [(65, 129, 33), (70, 100, 324)])
@pytest.mark.parametrize("form", EPILOGUES, ids=lambda f: "+".join(sorted(f)))
def test_gemm_small_epilogue_forms_exact(dev, M, N, K, form):
    """x_raw (the bare product, while C holds the epilogue), the exact BatchNorm, an integer residual and ReLU, in the product's
    own epilogue (splits 1) and in the reduce kernel's (splits 3)."""
    torch.manual_seed(M + N + K + len(form))
    A, B = _ints((M, K), -4, 4, dev), _ints((K, N), -4, 4, dev)
    bn = _exact_bn(M, dev) if form.get("bn") else None
    res = _ints((M, N), -50, 50, dev) if form.get("res") else None
    P = A.double() @ B.double()
    want = _epilogue64(P, bn, res, form.get("relu", False))
    assert bool((want != P).any())
    for (am, bk), padded, s in itertools.product(LAYOUTS, (False, True), (1, 3)):
        C, X = _gemm(A, B, am, bk, s, in_pad=3 if padded else 0, out_pad=3 if padded else 0, bn=bn, res=res,
                     relu=form.get("relu", False), xraw=form.get("xraw", False))
        what = "a_mcontig %d b_kcontig %d padded %d splits %d" % (am, bk, padded, s)
        _same(C, want, "C, " + what)
        if X is not None:
            _same(X, P, "x_raw, " + what)


def test_gemm_small_general_batchnorm(dev):
    """Random statistics and float operands (still poisoned / guarded) against float64, to the bound test_conv1x1_bn_act_vs_aten
    holds this epilogue to: relative Frobenius error below 2e-6."""
    torch.manual_seed(11)
    M, N, K = 70, 100, 324
    A, B = torch.randn(M, K, device=dev), torch.randn(K, N, device=dev)
    bn = (torch.empty(M, device=dev).uniform_(0.5, 1.5), torch.empty(M, device=dev).uniform_(-0.5, 0.5),
          torch.empty(M, device=dev).uniform_(-0.3, 0.3), torch.empty(M, device=dev).uniform_(0.5, 2.0), 1e-5)
    res = torch.randn(M, N, device=dev)
    P = A.double() @ B.double()
    want = _epilogue64(P, bn, res, True)
    for (am, bk), s in itertools.product(LAYOUTS, (1, _policy(M, N, K))):
        C, X = _gemm(A, B, am, bk, s, in_pad=1, out_pad=3, bn=bn, res=res, relu=True, xraw=True)
        for name, got, ref in (("y", C, want), ("x_raw", X, P)):
            err = _rel_fro(got, ref)
            assert err < 2e-6, (name, am, bk, s, err)


# ---- 2. the reduce kernels -----------------------------------------------------------------------------------------------------

def _takes_reduce4(M, N, out, xraw, ws):
    """launch_splitk_reduce's dispatch, restated: four elements per thread from 2^19 elements, dense rows, 16-byte alignment."""
    return M * N >= (1 << 19) and out.ld == N and (M * N) % 4 == 0 and (out.ptr | xraw.ptr | ws.ptr) % 16 == 0


@pytest.mark.parametrize("M,N,K", [(512, 1024, 256), (1024, 514, 256)])
def test_reduce4_and_scalar_reduce_exact_and_equal(dev, M, N, K):
    """small_splitk_reduce4_kernel (M N >= 2^19, ldc == N, aligned C / x_raw / workspace) against the scalar reduce that the SAME
    inputs take with C shifted by one float or with ldc = N + 3.  N = 514: N % 4 == 2, the four elements of a thread straddle two
    rows; the per-row BatchNorm makes a wrong row attribution a wrong value."""
    from cim_amd import _lib
    torch.manual_seed(N)
    A, B = _ints((M, K), -4, 4, dev), _ints((K, N), -4, 4, dev)
    bn, res = _exact_bn(M, dev), _ints((M, N), -50, 50, dev)
    P = A.double() @ B.double()
    want = _epilogue64(P, bn, res, False)
    a, lda = _poisoned(A, 1)
    b, ldb = _poisoned(B, 1)
    bn_args, keep = _bn_ptrs(bn)
    for s in (2, 6):
        results = []
        for out_pad, shift, vector in ((0, 0, True), (0, 1, False), (3, 0, False)):
            C, X, ws = _Out(M, N, out_pad, dev, shift), _Out(M, N, out_pad, dev, shift), _Ws(s * M * N, dev, 0)
            assert _takes_reduce4(M, N, C, X, ws) == vector
            r = _poisoned(res, out_pad)[0]
            _lib.call("cim_gemm_small_f32", a.data_ptr(), b.data_ptr(), C.ptr, M, N, K, lda, ldb, C.ld, 0, 0, X.ptr, *bn_args,
                      r.data_ptr(), 0, s, ws.ptr, _lib.stream_ptr())
            torch.cuda.synchronize()
            ws.check()
            c, x = C.check(), X.check()
            what = "splits %d ldc N + %d shift %d" % (s, out_pad, shift)
            _same(c, want, "C, " + what)
            _same(x, P, "x_raw, " + what)
            results.append(c)
        assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])


@pytest.mark.parametrize("M,N,K", [(128, 96, 1000), (512, 1024, 256)])
def test_split_k_is_deterministic(dev, M, N, K):
    """Float operands: two runs of the same call are bit-identical at every split count (fixed summation order, no atomics), and
    the results at different split counts agree with each other - and with float64 - within the suite's 2e-6 Frobenius bound."""
    torch.manual_seed(K)
    A, B = torch.randn(M, K, device=dev), torch.randn(K, N, device=dev)
    ref = A.double() @ B.double()
    runs = {}
    for s in sorted({1, _policy(M, N, K), 64}):
        first, _ = _gemm(A, B, 0, 0, s, shift=0, ws_shift=0)
        again, _ = _gemm(A, B, 0, 0, s, shift=0, ws_shift=0)
        assert torch.equal(first, again), s
        runs[s] = first
        err = _rel_fro(first, ref)
        assert err < 2e-6, (s, err)
    assert len(runs) == 3
    for s, t in itertools.combinations(runs, 2):
        err = _rel_fro(runs[s], runs[t].double())
        assert err < 2e-6, (s, t, err)


# ---- 3. cim_linear_bias_f32 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(37, 168, 4096), (1, 648, 100)])
def test_linear_bias_exact(dev, M, N, K):
    """Y = X . W^T + bias (both operands K-contiguous with ld == K: behind every K tail lies the next row), column bias in the
    product's epilogue and in the reduce's."""
    from cim_amd import _lib
    torch.manual_seed(N)
    X, W, bias = _ints((M, K), -2, 2, dev), _ints((N, K), -2, 2, dev), _ints((N,), -9, 9, dev)
    want = X.double() @ W.double().t() + bias.double()
    x, w, b = _poisoned(X)[0], _poisoned(W)[0], _pvec(bias)
    for s in sorted({1, 4, _policy(M, N, K)}):
        Y, ws = _Out(M, N, 0, dev), _Ws(s * M * N, dev)
        _lib.call("cim_linear_bias_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), Y.ptr, M, N, K, s, ws.ptr, _lib.stream_ptr())
        torch.cuda.synchronize()
        ws.check()
        _same(Y.check(), want, "splits %d" % s)


# ---- 4. cim_conv3x3_nchw_f32 / cim_conv7x7_nchw_f32 ----------------------------------------------------------------------------

def _conv3(x, w, stride, dil, splits, bn=None, res=None, relu=False):
    """One image x [cin][H][W], w [cout][cin][3][3] -> (y, x_raw) as [cout][Ho Wo]"""
    from cim_amd import _lib
    dev = x.device
    cin, H, W = x.shape
    cout = w.shape[0]
    n = ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    px, pw = _pvec(x), _pvec(w)
    Y, X, ws = _Out(cout, n, 0, dev), _Out(cout, n, 0, dev), _Ws(splits * cout * n, dev)
    bn_args, keep = _bn_ptrs(bn)
    r = _pvec(res) if res is not None else None
    _lib.call("cim_conv3x3_nchw_f32", px.data_ptr(), pw.data_ptr(), Y.ptr, cin, cout, H, W, stride, dil, X.ptr, *bn_args,
              _lib.ptr(r), int(relu), splits, ws.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    ws.check()
    return Y.check(), X.check()


def _conv64(x, w, stride, dil, k=3):
    y = F.conv2d(x.double()[None], w.double(), padding=dil * (k // 2), dilation=dil, stride=stride)[0]
    return y.reshape(y.shape[0], -1)


@pytest.mark.parametrize("cin,cout,H,W,stride,dil", [(3, 5, 1, 1, 1, 1), (4, 33, 1, 7, 2, 1), (5, 64, 2, 2, 2, 1), (8, 65, 3, 3, 1, 2),
                                                     (7, 16, 5, 9, 1, 8), (36, 70, 9, 13, 1, 1)])
def test_conv3x3_forward_tiny_maps_exact(dev, cin, cout, H, W, stride, dil):
    """Maps of one to a few pixels (nearly every tap is padding), stride 2 on 1 x 7 and 2 x 2, a dilation larger than the map,
    9 cin < 32, forced split counts (K = 27 ... 72: the later splits are empty; K = 324: the fifth of 5): NaN lies in front of and
    behind x and w, so a padding tap that is let in, or a K tail that is not zeroed, cannot pass."""
    from cim_amd import _lib
    torch.manual_seed(cin * cout + H)
    x, w = _ints((cin, H, W), -4, 4, dev), _ints((cout, cin, 3, 3), -4, 4, dev)
    P = _conv64(x, w, stride, dil)
    bn, res = _exact_bn(cout, dev), _ints(tuple(P.shape), -50, 50, dev)
    want = _epilogue64(P, bn, res, True)
    for s in sorted({1, 2, 5, _lib.call("cim_conv3x3_nchw_splits", cin, cout, H, W, stride)}):
        y, xr = _conv3(x, w, stride, dil, s)
        _same(y, P, "bare y, splits %d" % s)
        _same(xr, P, "bare x_raw, splits %d" % s)
        y, xr = _conv3(x, w, stride, dil, s, bn=bn, res=res, relu=True)
        _same(y, want, "y, splits %d" % s)
        _same(xr, P, "x_raw, splits %d" % s)


@pytest.mark.parametrize("cin,cout,H,W,stride", [(1, 1, 255, 4096, 1), (1, 2, 256, 4093, 2)])
def test_conv3x3_forward_at_the_geometry_limit(dev, cin, cout, H, W, stride):
    """The widest row and (nearly) the most pixels the launcher admits (W <= 4096, H W < 2^20): the kernel's pixel -> (row, column)
    decode (int)((n + 0.5f) * (1.0f / W)) runs at its largest n; a row boundary that rounds the wrong way moves a pixel by a row."""
    torch.manual_seed(W)
    x, w = _ints((cin, H, W), -4, 4, dev), _ints((cout, cin, 3, 3), -4, 4, dev)
    y, xr = _conv3(x, w, stride, 1, 1)
    P = _conv64(x, w, stride, 1)
    _same(y, P, "y")
    _same(xr, P, "x_raw")


@pytest.mark.parametrize("H,W", [(1024, 1024), (1, 4097)])
def test_conv3x3_refuses_maps_beyond_the_limit(dev, H, W):
    """H W >= 2^20 and W > 4096 are refused with an error and nothing is launched (the buffers are full-sized all the same)."""
    from cim_amd import _lib
    x, w = torch.zeros(1, H, W, device=dev), torch.ones(1, 1, 7, 7, device=dev)
    Y, ws = _Out(1, H * W, 0, dev), _Ws(H * W, dev)
    with pytest.raises(_lib.CimHipError):
        _lib.call("cim_conv3x3_nchw_f32", x.data_ptr(), w.data_ptr(), Y.ptr, 1, 1, H, W, 1, 1, None, None, None, None, None, 0.0,
                  None, 0, 1, ws.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((Y.raw == SENT).all())
    bn = [torch.ones(1, device=dev).data_ptr()] * 4
    with pytest.raises(_lib.CimHipError):
        _lib.call("cim_conv7x7_nchw_f32", x.data_ptr(), w.data_ptr(), Y.ptr, 1, 1, H, W, 1, *bn, 0.0, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((Y.raw == SENT).all())


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 6)])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv7x7_stem_tiny_maps_exact(dev, H, W, stride):
    """The 49-tap form on maps smaller than its kernel (K = 147: a K tail of 19 behind four full slabs)."""
    from cim_amd import _lib
    torch.manual_seed(H * 7 + stride)
    cin, cout = 3, 64
    x, w = _ints((cin, H, W), -4, 4, dev), _ints((cout, cin, 7, 7), -4, 4, dev)
    P = _conv64(x, w, stride, 1, 7)
    bn = _exact_bn(cout, dev)
    px, pw = _pvec(x), _pvec(w)
    bn_args, keep = _bn_ptrs(bn)
    for relu in (0, 1):
        Y = _Out(cout, P.shape[1], 0, dev)
        _lib.call("cim_conv7x7_nchw_f32", px.data_ptr(), pw.data_ptr(), Y.ptr, cin, cout, H, W, stride, *bn_args, relu, _lib.stream_ptr())
        torch.cuda.synchronize()
        _same(Y.check(), _epilogue64(P, bn, None, bool(relu)), "relu %d" % relu)


# ---- 5. 3 x 3 backward at small geometry, through the operators -----------------------------------------------------------------

def _set_exact_bn(bn):
    gamma, beta, mean, var, _ = _exact_bn(bn.num_features, bn.weight.device)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(mean); bn.running_var.copy_(var)


class _Bn64:
    """The eval-mode BatchNorm of the module `bn` in float64, written out - (x - mean) / sqrt(var + eps) * gamma + beta, what
    F.batch_norm computes from running statistics (it refuses eps == 0 itself) - with gamma / beta as autograd leaves."""

    def __init__(self, bn):
        self.weight = bn.weight.detach().double().requires_grad_(True)
        self.bias = bn.bias.detach().double().requires_grad_(True)
        self.mean, self.var, self.eps = bn.running_mean.double(), bn.running_var.double(), bn.eps

    def __call__(self, t):
        s = (1, -1, 1, 1)
        return (t - self.mean.view(s)) / torch.sqrt(self.var + self.eps).view(s) * self.weight.view(s) + self.bias.view(s)


def _conv3x3_bn_act_exact(dev, B, cin, cout, H, W, stride, relu, res):
    """conv3x3_bn_act forward + all gradients on integer data with the exact BatchNorm (nn.BatchNorm2d(eps=0.0): the fused path
    takes it) against float64 ATen (convolution, ReLU and autograd; the BatchNorm as _Bn64), bit for bit.  |x|, |w|, |dy| <= 2: the largest sum (dgamma at cin 68: 180 pixels x |dz| 2 x
    |conv| <= 2451) stays below 2^20."""
    from cim_amd.ops import conv3x3_bn_act, gemm
    conv = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(cout, eps=0.0).to(dev).eval()
    _set_exact_bn(bn)
    with torch.no_grad():
        conv.weight.copy_(_ints(tuple(conv.weight.shape), -2, 2, dev))
    x = _ints((B, cin, H, W), -2, 2, dev).requires_grad_(True)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = _ints((B, cout, ho, wo), -9, 9, dev).requires_grad_(True) if res else None
    y = conv3x3_bn_act(x, conv, bn, residual=r, relu=relu)
    up = _ints(tuple(y.shape), -2, 2, dev)
    y.backward(up)
    gemm.join_side()
    torch.cuda.synchronize()
    got = [y.detach(), x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad] + ([r.grad] if res else [])
    conv64, bn64 = copy.deepcopy(conv).double(), _Bn64(bn)
    for p_ in conv64.parameters():
        p_.grad = None
    x64 = x.detach().double().requires_grad_(True)
    r64 = r.detach().double().requires_grad_(True) if res else None
    o = bn64(conv64(x64))
    if res:
        o = o + r64
    if relu:
        o = torch.relu(o)
    o.backward(up.double())
    ref = [o.detach(), x64.grad, conv64.weight.grad, bn64.weight.grad, bn64.bias.grad] + ([r64.grad] if res else [])
    what = "B %d cin %d cout %d %d x %d stride %d relu %d res %d" % (B, cin, cout, H, W, stride, relu, res)
    for name, a, b_ in zip(("y", "dx", "dw", "dgamma", "dbeta", "dres"), got, ref):
        assert a is not None and a.shape == b_.shape, (name, what)
        _same(a, b_, name + ", " + what)


@pytest.mark.parametrize("H", [1, 2, 3, 4, 5, 6])
def test_conv3x3_stride2_backward_every_small_map_exact(dev, H):
    """conv3x3_dx2_kernel's four pixel classes at every parity of H and W, classes that are EMPTY (H == 1 or W == 1) included."""
    torch.manual_seed(H)
    for W in range(1, 7):
        for relu, res in ((True, True), (False, False)):
            _conv3x3_bn_act_exact(dev, 1, 4, 8, H, W, 2, relu, res)


@pytest.mark.parametrize("B,cin,cout,H,W,stride", [(2, 68, 8, 17, 19, 2),       # > 1 N tile per class, two M tiles, the batch's dW accumulation
                                                   (2, 8, 72, 6, 5, 2),         # K' = 72 ... 288 per class, two M tiles of the weight gradient
                                                   (1, 4, 8, 1, 1, 1), (1, 4, 8, 1, 7, 1), (2, 4, 8, 3, 3, 1)])
@pytest.mark.parametrize("relu,res", [(True, True), (False, False), (True, False)])
def test_conv3x3_backward_small_geometry_exact(dev, B, cin, cout, H, W, stride, relu, res):
    torch.manual_seed(cin + cout + H)
    _conv3x3_bn_act_exact(dev, B, cin, cout, H, W, stride, relu, res)


@pytest.mark.parametrize("H,W", [(3, 3), (9, 11)])
def test_conv3x3_bias_act_dilated_backward_exact(dev, H, W):
    """The VGG form (bias, no BatchNorm, no ReLU) with dilation 2 - on the 3 x 3 map every tap but the centre is padding."""
    from cim_amd.ops import conv3x3_bias_act, gemm
    torch.manual_seed(W)
    conv = torch.nn.Conv2d(8, 12, 3, stride=1, padding=2, dilation=2, bias=True).to(dev)
    with torch.no_grad():
        conv.weight.copy_(_ints(tuple(conv.weight.shape), -2, 2, dev))
        conv.bias.copy_(_ints((12,), -5, 5, dev))
    x = _ints((1, 8, H, W), -2, 2, dev).requires_grad_(True)
    y = conv3x3_bias_act(x, conv, relu=False)
    up = _ints(tuple(y.shape), -2, 2, dev)
    y.backward(up)
    gemm.join_side()
    torch.cuda.synchronize()
    c64 = copy.deepcopy(conv).double()
    for p_ in c64.parameters():
        p_.grad = None
    x64 = x.detach().double().requires_grad_(True)
    o = c64(x64)
    o.backward(up.double())
    for name, a, b_ in (("y", y.detach(), o.detach()), ("dx", x.grad, x64.grad), ("dw", conv.weight.grad, c64.weight.grad),
                        ("dbias", conv.bias.grad, c64.bias.grad)):
        assert a is not None and a.shape == b_.shape, name
        _same(a, b_, name)


# ---- 6. bn_act: several chunks per channel --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,C,H,W", [(2, 3, 50, 100), (2, 130, 1, 7)])
@pytest.mark.parametrize("relu,res,affine", [(True, True, True), (False, False, True), (True, False, False), (False, True, False)])
def test_bn_act_multi_chunk_exact(dev, N, C, H, W, relu, res, affine):
    """2 x 3 x 5000: the backward cuts a channel's 10000 elements into 3 chunks that meet through atomicAdd, the middle one
    covering the end of image 0 and the start of image 1; the forward takes 3 grid rows per plane.  2 x 130 x 7: C >= 128, one
    chunk, plain stores.  Integer data and the exact BatchNorm: atomics in any order give the float64 sums."""
    from cim_amd import _lib
    from cim_amd.ops import bn_act
    torch.manual_seed(C + relu + 2 * res)
    hw = H * W
    chunks = _lib.call("cim_bn_act_bwd_chunks", N, C, hw)
    if C < 128:
        per = -(-N * hw // chunks)
        assert chunks > 1 and any(0 < hw - k * per < per for k in range(chunks))     # a chunk starts in image 0 and ends in image 1
        assert -(-hw // 2048) == 3                                                    # cim_bn_act_fwd: ceil(HW / (256 * 8)) grid rows
    else:
        assert chunks == 1
    bn = torch.nn.BatchNorm2d(C, eps=0.0).to(dev).eval()
    _set_exact_bn(bn)
    if not affine:
        bn.weight.requires_grad_(False); bn.bias.requires_grad_(False)
    x = _ints((N, C, H, W), -3, 3, dev).requires_grad_(True)
    r = _ints((N, C, H, W), -9, 9, dev).requires_grad_(True) if res else None
    y = bn_act(x, bn, residual=r, relu=relu)
    up = _ints((N, C, H, W), -3, 3, dev)
    y.backward(up)
    torch.cuda.synchronize()
    bn64 = _Bn64(bn)
    x64 = x.detach().double().requires_grad_(True)
    r64 = r.detach().double().requires_grad_(True) if res else None
    o = bn64(x64)
    if res:
        o = o + r64
    if relu:
        o = torch.relu(o)
    o.backward(up.double())
    pairs = [("y", y.detach(), o.detach()), ("dx", x.grad, x64.grad)] + ([("dres", r.grad, r64.grad)] if res else [])
    if affine:
        pairs += [("dgamma", bn.weight.grad, bn64.weight.grad), ("dbeta", bn.bias.grad, bn64.bias.grad)]
    else:
        assert bn.weight.grad is None and bn.bias.grad is None
    for name, a, b_ in pairs:
        assert a is not None and a.shape == b_.shape, name
        _same(a, b_, name)
