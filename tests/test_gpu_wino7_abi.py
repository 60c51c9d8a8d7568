"""-m gpu: the Winograd stage kernels of MaskFuse's 3 x 3 convolution and the (c, h, w) flatten (cim_amd/csrc/winograd.hip: the eleven
entry points cim_wino7_* / cim_wino_* / cim_flatten_chw_*) straight at the C ABI against the DEFINITION, not against another kernel.

Every stage is linear, so it is its impulse responses.  They are measured here from the production kernels (`resp`: Tin, Tfil,
Tout, Tgd, Tadj, Tdx, Taw of tests/golden/wino7_np.py, impulses placed so that row, channel and (co, ci) order are pinned too) and
held to four identities that need no table: the forward and the weight-gradient sums give the 3 x 3 / padding 1 delta within
2^-21 K, the data-gradient stages are the forward's adjoint bit for bit, and the mask fold is Tdx resp. mask * Tdx.  With the
responses pinned, a float64 linear model built from them is the reference of every other test: on integers -3 .. 3 the dyadic
stages are EXACT (np.array_equal; the precondition is asserted on the measured responses), the two stages whose tables hold thirds
(filter, weight-gradient dy) are held to 2^-19 sum |T| |x| + the pair image's floor.  tests/test_wino7_np_cpu.py proves the
reference sound without a GPU.

Guards on every call: fp32 operands inside NaN (abi_guards._poisoned / _poisoned16: a read past the tensor shows as a NaN or an
infinite half), fp32 results inside sentinel memory (_Out), images inside fp16 NaN (_ImageOut: nothing outside [121][Rs][C]
changed, everything inside written)."""
import numpy as np
import pytest
import torch

import cases
import pair_cases as pc
import wino7_np as wn
from abi_guards import GUARD, SENT, F16_NAN2, _ImageOut, _Out, _poisoned, _poisoned16      # tests/golden/abi_guards.py
from wino7_np import F32, F64, NQ, PIX

pytestmark = pytest.mark.gpu

KIND_INPUT, KIND_FILTER, KIND_GD, KIND_ADJ = 0, 1, 2, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- one call of each entry point, guarded ---------------------------------------------------------------------------------------

def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _word(dev, value):
    """The bit pattern of a float32 as the int32 tensor an amax argument points to"""
    return _to(dev, np.array([value], F32).view(np.int32))


def _scales(dev, kind, amax):
    """cim_wino7_pair_scales for max |x| = amax, into sentinel memory -> (scale [121] on the device, the same as float64 numpy)"""
    from cim_amd import _lib
    w = _word(dev, amax)
    out = _Out(1, NQ, 0, dev, shift=0)
    _lib.call("cim_wino7_pair_scales", w.data_ptr(), 1, None, kind, out.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    s = out.check().reshape(NQ).contiguous()
    return s, s.cpu().numpy().astype(F64)


def _act_image(dev, stage, x, C, scale):
    """x [R][49][C] float32 through cim_wino7_input_pair ("input") or cim_wino7_dy_pair ("gd": adjoint 0, "adj": adjoint 1) with
    Rs = pad32(R).  -> the decoded image [121][Rs][C] float64; pad rows are asserted zero in every word"""
    from cim_amd import _lib
    R = x.shape[0]
    assert x.shape == (R, PIX, C) and x.dtype == F32
    Rs = wn.pad32(R)
    xd = _poisoned16(_to(dev, x))
    img = _ImageOut(NQ * Rs * C, dev)
    if stage == "input":
        _lib.call("cim_wino7_input_pair", xd.data_ptr(), img.ptr, scale[0].data_ptr(), R, Rs, C, _lib.stream_ptr())
    else:
        _lib.call("cim_wino7_dy_pair", xd.data_ptr(), img.ptr, scale[0].data_ptr(), R, Rs, C, int(stage == "adj"), _lib.stream_ptr())
    torch.cuda.synchronize()
    return _decoded(img, Rs, C, R, scale)


def _decoded(img, Rs, C, R, scale):
    words = img.check()
    pad = words.reshape(NQ, Rs, C)[:, R:, :]
    assert not (pad & 0x7FFF7FFF).any(), "%d words of the pad rows are not zero" % int(((pad & 0x7FFF7FFF) != 0).sum())
    return wn.decode_image(words, NQ, Rs, C, scale[1])


def _filter_image(dev, W, scale):
    """W [Cout][Cin][9] float32 through cim_wino7_filter_pair -> the decoded image [121][Cout][Cin]"""
    from cim_amd import _lib
    Cout, Cin, _ = W.shape
    wd, ld = _poisoned(_to(dev, W.reshape(Cout * Cin, 9)))
    assert ld == 9
    img = _ImageOut(NQ * Cout * Cin, dev)
    _lib.call("cim_wino7_filter_pair", wd.data_ptr(), img.ptr, scale[0].data_ptr(), Cout, Cin, _lib.stream_ptr())
    torch.cuda.synchronize()
    return wn.decode_image(img.check(), NQ, Cout, Cin, scale[1])


def _output(dev, M, bias=None, relu=0, word=None):
    """M [121][R][C] through cim_wino7_output_amax -> (y [R][49][C] float32 numpy, the amax word afterwards or None)"""
    from cim_amd import _lib
    _, R, C = M.shape
    md = _poisoned16(_to(dev, M))
    bd = None if bias is None else _poisoned16(_to(dev, bias))
    wd = None if word is None else torch.tensor([word], dtype=torch.int32, device=dev)
    out = _Out(R * PIX, C, 0, dev, shift=0)
    _lib.call("cim_wino7_output_amax", md.data_ptr(), _lib.ptr(bd), out.ptr, R, C, relu, _lib.ptr(wd), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.check().cpu().numpy().reshape(R, PIX, C), (None if wd is None else int(wd.item()))


def _dx(dev, M):
    """M [121][R][C] through cim_wino_dx_adjoint_output -> dx [R][49][C]"""
    from cim_amd import _lib
    _, R, C = M.shape
    md = _poisoned16(_to(dev, M))
    out = _Out(R * PIX, C, 0, dev, shift=0)
    _lib.call("cim_wino_dx_adjoint_output", md.data_ptr(), out.ptr, R, 7, C, 7, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.check().cpu().numpy().reshape(R, PIX, C)


def _maskfold(dev, M, masks):
    """M [121][R][2 Cb], masks [R][49] through cim_wino7_dx_maskfold -> dbox [R][49][Cb]"""
    from cim_amd import _lib
    _, R, C2 = M.shape
    md = _poisoned16(_to(dev, M))
    kd, _ = _poisoned(_to(dev, masks.astype(F32)))
    out = _Out(R * PIX, C2 // 2, 0, dev, shift=0)
    _lib.call("cim_wino7_dx_maskfold", md.data_ptr(), kd.data_ptr(), out.ptr, R, C2 // 2, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.check().cpu().numpy().reshape(R, PIX, C2 // 2)


def _wgrad(dev, dU):
    """dU [121][Cin][Cout] through cim_wino_wgrad_output -> dW [Cout][Cin][9]"""
    from cim_amd import _lib
    _, Cin, Cout = dU.shape
    ud = _poisoned16(_to(dev, dU))
    out = _Out(Cout * Cin, 9, 0, dev, shift=0)
    _lib.call("cim_wino_wgrad_output", ud.data_ptr(), out.ptr, Cout, Cin, 7, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.check().cpu().numpy().reshape(Cout, Cin, 9)


def _equal(got, want, what):
    """Bit-for-bit agreement of a result with the float64 model of exact data; names the first wrong element"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, len(bad), got.size, [int(v) for v in first], float(got[first]), float(want[first])))


_DEVIATION = {}


def _record(name, ratio):
    _DEVIATION[name] = max(float(ratio), _DEVIATION.get(name, 0.0))
    cases.record_deviation("wino7_stage_identities", dict(_DEVIATION))


# ---- the measured responses ------------------------------------------------------------------------------------------------------

class _Responses:
    """Each response is measured on first use (a stage that fails its measurement fails the tests that need it, by name)."""

    def __init__(self, dev):
        self.dev, self.done = dev, {}

    def __getitem__(self, name):
        if name not in self.done:
            self.done[name] = getattr(self, "_" + name)()
        return self.done[name]

    def _flat(self):
        """One scale for all positions, chosen here: a response does not depend on cim_wino7_pair_scales.  2^8: the largest entry
        (64, in Tadj) stays below 2^15 and the smallest (1 / 225, in Tfil) keeps its 22 bits above the fp16 subnormals' granule."""
        s = torch.full((NQ,), 256.0, device=self.dev)
        return s, s.cpu().numpy().astype(F64)

    def _act(self, stage):
        d = _act_image(self.dev, stage, wn.act_impulses(), wn.ACT_C, self._flat())
        assert d.shape[1] == wn.ACT_RS
        return wn.act_response(d)

    def _Tin(self):
        return self._act("input")

    def _Tgd(self):
        return self._act("gd")

    def _Tadj(self):
        return self._act("adj")

    def _Tfil(self):
        return wn.filter_response(_filter_image(self.dev, wn.filter_impulses(), self._flat()))

    def _Tout(self):
        return wn.pos_response(_output(self.dev, wn.pos_impulses(wn.POS_R, wn.POS_C))[0])

    def _Tdx(self):
        return wn.pos_response(_dx(self.dev, wn.pos_impulses(wn.POS_R, wn.POS_C)))

    def _taw(self, Cout, Cin):
        dW = _wgrad(self.dev, wn.pos_impulses(Cin, Cout))                      # impulse n in element (ci, co) = divmod(n, Cout)
        return wn.pos_response(np.transpose(dW, (1, 2, 0)))                    # [Cin][9][Cout]

    def _Taw(self):
        return self._taw(64, 4)               # the rows kernel

    def _Taw_fallback(self):
        return self._taw(11, 11)              # one lane per element


@pytest.fixture(scope="module")
def resp(dev):
    return _Responses(dev)


# ---- 1. the four identities ----------------------------------------------------------------------------------------------------------

def test_forward_identity_of_input_filter_and_output_stage(resp):
    """sum_q Tout[o,q] Tin[q,i] Tfil[q,t] is the 3 x 3 / padding 1 delta at all 49 x 49 x 9 triples, within 2^-21 K = 8 x 2^-24 K
    (measured on an MI355X: worst 1.50 x 2^-24 K)"""
    ratio = wn.check_identity(wn.forward_sums(resp["Tout"], resp["Tin"], resp["Tfil"]), "forward: output x input x filter stage")
    print("forward identity: worst |sum - delta| = %.2f x 2^-24 K" % ratio)
    _record("forward_identity_ratio", ratio)


def test_weight_gradient_identity_of_input_dy_and_wgrad_output_stage(resp):
    """sum_q Taw[t,q] Tin[q,i] Tgd[q,o] is the same delta (measured: worst 1.50 x 2^-24 K); the rows kernel and the one-lane
    fallback give the same Taw"""
    bad = np.argwhere(resp["Taw"] != resp["Taw_fallback"])
    assert bad.size == 0, "wgrad output: rows kernel and fallback differ at (tap, position) = %s" % bad[0].tolist()
    ratio = wn.check_identity(wn.wgrad_sums(resp["Taw"], resp["Tin"], resp["Tgd"]), "weight gradient: wgrad output x input x dy stage")
    print("weight-gradient identity: worst |sum - delta| = %.2f x 2^-24 K" % ratio)
    _record("wgrad_identity_ratio", ratio)


def test_data_gradient_stages_are_the_adjoint_of_the_forward(resp):
    """Tadj[q,o] == Tout[o,q] (dy stage, adjoint = 1) and Tdx[i,q] == Tin[q,i] (dx adjoint output), bit for bit"""
    wn.check_adjoint(resp["Tadj"], resp["Tout"], resp["Tdx"], resp["Tin"])


def test_mask_fold_impulses(dev, resp):
    """cim_wino7_dx_maskfold: an impulse in the plain half answers with Tdx, one in the masked half with mask[pixel] * Tdx"""
    R, Cb = wn.POS_R, wn.POS_C
    rng = np.random.RandomState(4)
    masks = rng.choice(np.array(wn.MASK_VALUES, F32), size=(R, PIX))
    masks[:, :5] = np.array(wn.MASK_VALUES, F32)                            # every value in every ROI
    imp = wn.pos_impulses(R, Cb)
    M = np.zeros((NQ, R, 2 * Cb), F32)
    M[:, :, :Cb] = imp
    _equal(wn.pos_response(_maskfold(dev, M, masks)), resp["Tdx"], "mask fold, plain half")
    M = np.zeros((NQ, R, 2 * Cb), F32)
    M[:, :, Cb:] = imp
    got = wn.pos_response(_maskfold(dev, M, masks))                        # [49][121]: position q sits in row q // Cb
    want = resp["Tdx"] * masks[np.arange(NQ) // Cb, :].T.astype(F64)
    _equal(got, want, "mask fold, masked half")


# ---- 2. exact data at the edges --------------------------------------------------------------------------------------------------------

def _exact(resp, *names):
    for n in names:
        wn.check_dyadic(resp[n], n)
    return [resp[n] for n in names]


@pytest.mark.parametrize("R,C", [(1, 8), (32, 64), (33, 1032)])           # two lanes; no pad rows; 31 pad rows + a second c += 1024 trip of two lanes
def test_input_and_adjoint_dy_images_exact(dev, resp, R, C):
    Tin, Tadj = _exact(resp, "Tin", "Tadj")
    rng = np.random.RandomState(R * 7 + C)
    x = wn.ints(rng, (R, PIX, C))
    for stage, kind, T in (("input", KIND_INPUT, Tin), ("adj", KIND_ADJ, Tadj)):
        d = _act_image(dev, stage, x, C, _scales(dev, kind, float(wn.INT_MAX)))
        _equal(d[:, :R, :], wn.to_positions(T, x), "%s stage, R %d C %d" % (stage, R, C))


OUTPUT_FLAGS = [(0, True, True), (1, False, True), (1, True, False), (0, False, False), (0, False, True), (1, True, True)]   # relu, bias, amax word


@pytest.mark.parametrize("i,C,R", [(i, C, R) for i, (C, R) in enumerate([(4, 1), (260, 5), (1028, 1), (4, 5), (260, 1), (1028, 5)])])
def test_output_stage_exact_and_its_amax_word(dev, resp, i, C, R):
    """One lane, a ragged last wave and a second c += 1024 trip; relu 0 / 1, bias / none, amax word / none.  Without ReLU the
    largest magnitude is planted NEGATIVE in the last row and channel: the word holds max |y|, which y.max() is not."""
    (Tout,) = _exact(resp, "Tout")
    relu, has_bias, has_word = OUTPUT_FLAGS[i]
    rng = np.random.RandomState(100 + i)
    M = wn.ints(rng, (NQ, R, C))
    bias = wn.ints(rng, (C,)) if has_bias else None
    o0 = int(np.abs(Tout).sum(axis=1).argmax())
    M[:, R - 1, C - 1] = -wn.worst_case(Tout)[o0]
    if has_bias:
        bias[C - 1] = -wn.INT_MAX
    want = wn.from_positions(Tout, M) + (0.0 if bias is None else bias.astype(F64))
    assert want[R - 1, o0, C - 1] == want.min() and -want.min() > want.max() > 0
    if relu:
        want = np.maximum(want, 0.0)
    got, word = _output(dev, M, bias, relu, 0 if has_word else None)
    _equal(got, want, "output stage, C %d R %d relu %d" % (C, R, relu))
    if has_word:
        assert word == int(pc.bits(np.abs(want).max())), "amax word %#x, max |y| = %r, max y = %r" % (word, float(np.abs(want).max()), float(want.max()))
        _, kept = _output(dev, M, bias, relu, int(pc.bits(1e9)))             # atomicMax: a larger word is kept
        assert kept == int(pc.bits(1e9))


@pytest.mark.parametrize("C", [4, 516, 2052])                              # one lane; a second grid chunk; more than four chunks
@pytest.mark.parametrize("R", [1, 3])
def test_dx_adjoint_output_exact(dev, resp, R, C):
    (Tdx,) = _exact(resp, "Tdx")
    M = wn.ints(np.random.RandomState(R + C), (NQ, R, C))
    _equal(_dx(dev, M), wn.from_positions(Tdx, M), "dx adjoint output, R %d C %d" % (R, C))


@pytest.mark.parametrize("Cb", [4, 260, 1028])
def test_dx_maskfold_exact(dev, resp, Cb):
    """dbox = dcat[..., :Cb] + mask * dcat[..., Cb:] of the float64 model, masks from {0, 0.5, 1, 2, -1}"""
    (Tdx,) = _exact(resp, "Tdx")
    assert 3 * wn.INT_MAX * np.abs(Tdx).sum(axis=1).max() * 128 < 2.0 ** 24    # (1 + max |mask|) x the row bound, in granules of 1 / 128
    R = 3
    rng = np.random.RandomState(Cb)
    M = wn.ints(rng, (NQ, R, 2 * Cb))
    masks = rng.choice(np.array(wn.MASK_VALUES, F32), size=(R, PIX))
    masks[:, :5] = np.array(wn.MASK_VALUES, F32)
    want = wn.mask_fold(wn.from_positions(Tdx, M), masks)
    _equal(_maskfold(dev, M, masks), want, "mask fold, Cb %d" % Cb)


@pytest.mark.parametrize("Cout,Cin", [(64, 4), (128, 8), (64, 6), (40, 24), (5, 3)])     # rows kernel x 2; fallback: Cin % 4, Cout % 64, both
def test_wgrad_output_exact(dev, resp, Cout, Cin):
    (Taw,) = _exact(resp, "Taw")
    dU = wn.ints(np.random.RandomState(Cout + Cin), (NQ, Cin, Cout))
    _equal(_wgrad(dev, dU), wn.wgrad_from_positions(Taw, dU), "wgrad output, Cout %d Cin %d" % (Cout, Cin))


def _relu_y(rng, shape):
    """integers -3 .. 3 with exact +0.0 and -0.0 among them"""
    y = wn.ints(rng, shape)
    y[(rng.rand(*shape) < 0.1) & (y == 0)] = -0.0
    y.flat[1], y.flat[2] = 0.0, -0.0
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    return y


@pytest.mark.parametrize("PP", [49, 64, 1])
@pytest.mark.parametrize("C", [64, 192])
@pytest.mark.parametrize("R", [1, 3])
def test_flatten_chw_bwd_bias_against_numpy(dev, R, C, PP):
    """dst[r,p,c] = src[r, c PP + p] where y > 0 (+-0.0 mask), bias_partial[r,c] = the sum over p; y and bias_partial present and NULL"""
    from cim_amd import _lib
    rng = np.random.RandomState(PP * 1000 + C + R)
    src = wn.ints(rng, (R, C * PP))
    y = _relu_y(rng, (R, PP, C))
    sd, _ = _poisoned(_to(dev, src))
    yd, _ = _poisoned(_to(dev, y.reshape(R * PP, C)))
    for has_y in (True, False):
        want, bsum = wn.flatten_chw_bwd(src, y if has_y else None, PP, C)
        for has_b in (True, False):
            dst, bp = _Out(R * PP, C, 0, dev), _Out(R, C, 0, dev)
            _lib.call("cim_flatten_chw_bwd_bias", sd.data_ptr(), yd.data_ptr() if has_y else None, dst.ptr, bp.ptr if has_b else None,
                      R, PP, C, _lib.stream_ptr())
            torch.cuda.synchronize()
            what = "flatten backward, PP %d C %d R %d, y %d bias %d" % (PP, C, R, has_y, has_b)
            _equal(dst.check().cpu().numpy().reshape(R, PP, C), want, what)
            if has_b:
                _equal(bp.check().cpu().numpy(), bsum, what + ": bias_partial")
            else:
                assert bool((bp.raw == SENT).all())


@pytest.mark.parametrize("PP", [49, 64, 1])
@pytest.mark.parametrize("C", [64, 192])
@pytest.mark.parametrize("R", [1, 3])
def test_flatten_chw_pair_against_numpy(dev, R, C, PP):
    """The image decodes to the (c, p) permutation of src, rows R .. 32 to zero"""
    from cim_amd import _lib
    rng = np.random.RandomState(PP * 1000 + C + R + 1)
    src = wn.ints(rng, (R, PP, C))
    Rs = wn.pad32(R)
    sd, _ = _poisoned(_to(dev, src.reshape(R * PP, C)))
    s = pc.natural_scale(src)
    sc = _to(dev, np.array([s], F32))
    img = _ImageOut(Rs * C * PP, dev)
    _lib.call("cim_flatten_chw_pair", sd.data_ptr(), img.ptr, sc.data_ptr(), R, Rs, PP, C, _lib.stream_ptr())
    torch.cuda.synchronize()
    words = img.check().reshape(Rs, C * PP)
    assert not (words[R:] & 0x7FFF7FFF).any()
    h, l = pc.decode(words)
    got = (h.astype(F64) + l.astype(F64)) / F64(s)
    _equal(got[:R], wn.flatten_chw(src), "flatten, PP %d C %d R %d" % (PP, C, R))
    assert np.array_equal(words[:R], pc.encode(*pc.split(wn.flatten_chw(src), s)))        # and the very words of the host split


@pytest.mark.parametrize("R,C", [(1, 256), (33, 512)])
def test_flatten_bwd_dy_pair_against_the_model(dev, resp, R, C):
    """The fused flatten backward + ReLU mask + both dy transforms: E is Tadj applied to the numpy-masked, transposed dX exactly,
    D is Tgd applied to it within the bound of the inexact stages, bias_partial the numpy sums; E alone, D alone and both"""
    from cim_amd import _lib
    (Tadj,) = _exact(resp, "Tadj")
    Tgd = resp["Tgd"]
    rng = np.random.RandomState(R + C)
    Rs = wn.pad32(R)
    dX = wn.ints(rng, (R, C * PIX))
    y = _relu_y(rng, (R, PIX, C))
    dy, bsum = wn.flatten_chw_bwd(dX, y, PIX, C)
    xd, yd = _poisoned16(_to(dev, dX)), _poisoned16(_to(dev, y))
    sE, sD = _scales(dev, KIND_ADJ, float(wn.INT_MAX)), _scales(dev, KIND_GD, float(wn.INT_MAX))
    for want_e, want_d in ((True, True), (True, False), (False, True)):
        E, D = _ImageOut(NQ * Rs * C, dev), _ImageOut(NQ * Rs * C, dev)
        bp = _Out(R, C, 0, dev, shift=0)
        _lib.call("cim_wino7_flatten_bwd_dy_pair", xd.data_ptr(), yd.data_ptr(), E.ptr if want_e else None, sE[0].data_ptr() if want_e else None,
                  D.ptr if want_d else None, sD[0].data_ptr() if want_d else None, bp.ptr, R, Rs, C, _lib.stream_ptr())
        torch.cuda.synchronize()
        what = "fused flatten backward, R %d C %d, E %d D %d" % (R, C, want_e, want_d)
        _equal(bp.check().cpu().numpy(), bsum, what + ": bias_partial")
        if want_e:
            _equal(_decoded(E, Rs, C, R, sE)[:, :R, :], wn.to_positions(Tadj, dy), what + ": E image")
        else:
            assert bool((E.raw == F16_NAN2).all())
        if want_d:
            ratio = wn.check_stage(_decoded(D, Rs, C, R, sD)[:, :R, :], wn.to_positions, Tgd, dy, sD[1], what + ": D image")
            _record("fused_dy_stage_ratio", ratio)
        else:
            assert bool((D.raw == F16_NAN2).all())


# ---- 3. the two inexact stages ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cout,Cin", [(18, 8), (5, 24), (11, 40)])         # the last two: a partly live final workgroup
def test_filter_stage_within_its_bound(dev, resp, Cout, Cin):
    """Random fp32 filters: |decoded - Tfil w| <= 2^-19 sum |Tfil| |w| + floor = 32 x 2^-24 sum ... (measured: worst 6.3 x 2^-24)"""
    W = wn.randoms(np.random.RandomState(Cout * Cin), (Cout, Cin, 9))
    sc = _scales(dev, KIND_FILTER, float(np.abs(W).max()))
    ratio = wn.check_stage(_filter_image(dev, W, sc), wn.filter_positions, resp["Tfil"], W, sc[1], "filter stage, Cout %d Cin %d" % (Cout, Cin))
    print("filter stage (%d, %d): worst error %.2f x 2^-24 sum |T||w|" % (Cout, Cin, ratio))
    _record("filter_stage_ratio", ratio)


@pytest.mark.parametrize("R,C", [(1, 8), (32, 64), (33, 1032)])
def test_weight_gradient_dy_stage_within_its_bound(dev, resp, R, C):
    """Random fp32 gradients through cim_wino7_dy_pair, adjoint = 0, under the same bound (measured: worst 6.7 x 2^-24), pad rows
    and guards as in the exact tests"""
    x = wn.randoms(np.random.RandomState(R * 11 + C), (R, PIX, C))
    sc = _scales(dev, KIND_GD, float(np.abs(x).max()))
    d = _act_image(dev, "gd", x, C, sc)
    ratio = wn.check_stage(d[:, :R, :], wn.to_positions, resp["Tgd"], x, sc[1], "weight-gradient dy stage, R %d C %d" % (R, C))
    print("weight-gradient dy stage (%d, %d): worst error %.2f x 2^-24 sum |T||x|" % (R, C, ratio))
    _record("wgrad_dy_stage_ratio", ratio)


# ---- 4. scales -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [KIND_INPUT, KIND_FILTER, KIND_GD, KIND_ADJ])
def test_scales_hold_the_worst_input_of_every_position(dev, resp, kind):
    """cim_wino7_pair_scales promises |transformed value| scale[q] < 2^15: row / element q carries amax * sign(T[q]), the input that
    maximises position q.  Powers of two, nothing infinite, and the values are the model's."""
    name, stage = {KIND_INPUT: ("Tin", "input"), KIND_FILTER: ("Tfil", None), KIND_GD: ("Tgd", "gd"), KIND_ADJ: ("Tadj", "adj")}[kind]
    T = resp[name]
    amax = float(wn.INT_MAX)
    sc = _scales(dev, kind, amax)
    assert np.all(sc[1] > 0) and wn.is_power_of_two(sc[1]), sc[1]
    worst = wn.worst_case(T, amax)                                          # [121][49 or 9]
    if kind == KIND_FILTER:
        Cout, Cin = 16, 8
        W = np.zeros((Cout * Cin, 9), F32)
        W[:NQ] = worst
        W = W.reshape(Cout, Cin, 9)
        d = _filter_image(dev, W, sc)                                       # (decode_image asserts that no half is infinite)
        peak = d.reshape(NQ, Cout * Cin)[np.arange(NQ), np.arange(NQ)]
        ratio = wn.check_stage(d, wn.filter_positions, T, W, sc[1], "filter stage on the worst inputs")
    else:
        C = 8
        x = np.repeat(worst[:, :, None], C, axis=2)                         # [121 ROIs][49][8]
        d = _act_image(dev, stage, x, C, sc)[:, :NQ, :]
        peak = d[np.arange(NQ), np.arange(NQ), 0]
        if kind == KIND_GD:
            ratio = wn.check_stage(d, wn.to_positions, T, x, sc[1], "weight-gradient dy stage on the worst inputs")
        else:
            wn.check_dyadic(T, name)
            _equal(d, wn.to_positions(T, x), "%s stage on the worst inputs" % stage)
            ratio = 0.0
    assert ratio <= wn.STAGE_RATIO
    rows = amax * np.abs(T).sum(axis=1)
    assert np.all(np.abs(peak) >= rows * (1 - 2.0 ** -18)), "the worst input does not reach the row sum at position %d" % int(
        (np.abs(peak) < rows * (1 - 2.0 ** -18)).argmax())
    over = np.abs(d) * sc[1].reshape(NQ, 1, 1) >= 2.0 ** 15
    assert not over.any(), "|value| scale >= 2^15 at (q, row, col) = %s" % np.argwhere(over)[0].tolist()


# ---- 5. rejections: the argument checks, nothing is launched ----------------------------------------------------------------------------

def test_rejections(dev):
    from cim_amd import _lib
    st = _lib.stream_ptr()
    z = torch.zeros(1 << 15, device=dev)                                     # every fp32 operand of the shapes below
    one = torch.ones(NQ, device=dev)
    word = _word(dev, 1.0)
    img = _ImageOut(NQ * 32 * 256, dev)
    out = _Out(2 * PIX, 256, 0, dev, shift=0)
    Z, S, I, O, A = z.data_ptr(), one.data_ptr(), img.ptr, out.ptr, word.data_ptr()
    base = {
        "cim_wino7_input_pair": dict(x=Z, V=I, scale=S, R=2, Rs=32, C=8),
        "cim_wino7_dy_pair": dict(dy=Z, D=I, scale=S, R=2, Rs=32, C=8, adjoint=0),
        "cim_wino7_filter_pair": dict(W=Z, U=I, scale=S, Cout=2, Cin=8),
        "cim_wino7_output_amax": dict(M=Z, bias=None, y=O, R=2, C=4, relu=0, y_amax=None),
        "cim_wino_dx_adjoint_output": dict(M=Z, dx=O, R=2, P=7, C=4, tile=7),
        "cim_wino7_dx_maskfold": dict(M=Z, masks=Z, dbox=O, R=2, Cb=4),
        "cim_wino_wgrad_output": dict(dU=Z, dW=O, Cout=2, Cin=2, tile=7),
        "cim_wino7_pair_scales": dict(amax=A, n_amax=1, amax_mul=None, kind=0, scale=O),
        "cim_wino7_flatten_bwd_dy_pair": dict(dX=Z, relu_y=Z, E=I, scale_e=S, D=None, scale_d=None, bias_partial=O, R=2, Rs=32, C=256),
        "cim_flatten_chw_pair": dict(src=Z, dst=I, scale=S, R=2, Rs=32, PP=49, C=64),
        "cim_flatten_chw_bwd_bias": dict(src=Z, relu_y=None, dst=O, bias_partial=None, R=2, PP=49, C=64),
    }
    assert 2 * 256 * PIX <= z.numel() and NQ * 2 * 8 <= z.numel()

    def run(name, **kw):
        args = dict(base[name])
        assert set(kw) <= set(args)
        args.update(kw)
        _lib.call(name, *(list(args.values()) + [st]))

    bad = [("cim_wino7_input_pair", dict(C=12)), ("cim_wino7_input_pair", dict(Rs=1)), ("cim_wino7_input_pair", dict(x=None)),
           ("cim_wino7_input_pair", dict(V=None)), ("cim_wino7_input_pair", dict(scale=None)),
           ("cim_wino7_dy_pair", dict(C=12)), ("cim_wino7_dy_pair", dict(Rs=1)), ("cim_wino7_dy_pair", dict(dy=None)),
           ("cim_wino7_dy_pair", dict(D=None)), ("cim_wino7_dy_pair", dict(scale=None)), ("cim_wino7_dy_pair", dict(C=12, adjoint=1)),
           ("cim_wino7_filter_pair", dict(Cin=12)), ("cim_wino7_filter_pair", dict(W=None)), ("cim_wino7_filter_pair", dict(U=None)),
           ("cim_wino7_filter_pair", dict(scale=None)),
           ("cim_wino7_output_amax", dict(C=6)), ("cim_wino7_output_amax", dict(M=None)), ("cim_wino7_output_amax", dict(y=None)),
           ("cim_wino_dx_adjoint_output", dict(C=6)), ("cim_wino_dx_adjoint_output", dict(tile=4)), ("cim_wino_dx_adjoint_output", dict(P=8)),
           ("cim_wino_dx_adjoint_output", dict(M=None)), ("cim_wino_dx_adjoint_output", dict(dx=None)),
           ("cim_wino7_dx_maskfold", dict(Cb=6)), ("cim_wino7_dx_maskfold", dict(M=None)), ("cim_wino7_dx_maskfold", dict(masks=None)),
           ("cim_wino7_dx_maskfold", dict(dbox=None)),
           ("cim_wino_wgrad_output", dict(tile=4)), ("cim_wino_wgrad_output", dict(dU=None)), ("cim_wino_wgrad_output", dict(dW=None)),
           ("cim_wino7_pair_scales", dict(kind=4)), ("cim_wino7_pair_scales", dict(n_amax=0)), ("cim_wino7_pair_scales", dict(amax=None)),
           ("cim_wino7_pair_scales", dict(scale=None)),
           ("cim_wino7_flatten_bwd_dy_pair", dict(C=128)), ("cim_wino7_flatten_bwd_dy_pair", dict(E=None, scale_e=None)),
           ("cim_wino7_flatten_bwd_dy_pair", dict(scale_e=None)), ("cim_wino7_flatten_bwd_dy_pair", dict(D=I)),
           ("cim_wino7_flatten_bwd_dy_pair", dict(dX=None)), ("cim_wino7_flatten_bwd_dy_pair", dict(Rs=1)),
           ("cim_flatten_chw_pair", dict(PP=65)), ("cim_flatten_chw_pair", dict(C=96)), ("cim_flatten_chw_pair", dict(Rs=1)),
           ("cim_flatten_chw_pair", dict(src=None)), ("cim_flatten_chw_pair", dict(dst=None)), ("cim_flatten_chw_pair", dict(scale=None)),
           ("cim_flatten_chw_bwd_bias", dict(PP=65)), ("cim_flatten_chw_bwd_bias", dict(C=96)), ("cim_flatten_chw_bwd_bias", dict(src=None)),
           ("cim_flatten_chw_bwd_bias", dict(dst=None))]
    for name, kw in bad:
        with pytest.raises(_lib.CimHipError):
            run(name, **kw)
    torch.cuda.synchronize()
    assert bool((out.raw == SENT).all()) and bool((img.raw == F16_NAN2).all())
    # each refusal above is due to the argument(s) it changes: the unchanged calls are accepted
    for name in base:
        run(name)
    torch.cuda.synchronize()
    assert bool((out.raw[:out.front] == SENT).all()) and bool((img.raw[:GUARD] == F16_NAN2).all())
