"""csrc/pool.hip against ATen: the max-pools of the ResNet stem / VGG16 and HRNet's nearest up-sampling (SURVEY.md a-11;
/root/reference/lib/modeling/resnet50.py:29, vgg16.py:43,50,60, HRNet.py:201).  Bit-exact: a maximum is exact, and the backward
tests use integer-valued gradients (sums of small integers are exact in fp32 whatever the order - ATen's backward scatters with
atomics) next to a random-gradient case held to 1e-6.  The second half calls the entry points at the C ABI with guarded buffers:
the geometries no body uses (stride above the kernel, k = 7, 1 x 1 maps), a plane of -inf, the accumulating up-sampling that has
no caller, and the refusals."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape,k,s,p", [((1, 64, 258, 344), 3, 2, 1), ((2, 3, 7, 9), 3, 2, 1), ((1, 5, 33, 47), 2, 2, 0),
                                         ((1, 128, 130, 173), 2, 2, 0), ((1, 2, 8, 8), 3, 1, 1), ((1, 1, 5, 6), 5, 3, 2)])
def test_max_pool_forward_backward_equal_aten(shape, k, s, p):
    from cim_amd.ops import max_pool2d
    dev = _dev()
    g = torch.Generator().manual_seed(sum(shape) + k)
    for ties in (False, True):
        x = torch.randint(-3, 4, shape, generator=g).float() if ties else torch.randn(shape, generator=g)
        x = x.to(dev).requires_grad_(True)
        xr = x.detach().clone().requires_grad_(True)
        m = nn.MaxPool2d(k, s, p)
        y = max_pool2d(x, m)
        yr = m(xr)
        assert y.shape == yr.shape and torch.equal(y, yr)
        dy = torch.randint(-4, 5, y.shape, generator=g).float().to(dev)
        y.backward(dy)
        yr.backward(dy)
        assert torch.equal(x.grad, xr.grad), (ties, float((x.grad - xr.grad).abs().max()))
    # random gradients: equal up to the order of <= 4 additions per pixel
    x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    dy = torch.randn(max_pool2d(x, m).shape, generator=g).to(dev)
    max_pool2d(x, m).backward(dy)
    m(xr).backward(dy)
    assert float((x.grad - xr.grad).abs().max()) <= 1e-6 * float(dy.abs().max()) * 4


def test_max_pool_nan_and_no_grad():
    from cim_amd.ops import max_pool2d
    dev = _dev()
    x = torch.randn(1, 4, 9, 11, device=dev)
    x[0, 1, 4, 5] = float("nan")
    m = nn.MaxPool2d(3, 2, 1)
    y, yr = max_pool2d(x, m), m(x)
    assert torch.equal(torch.isnan(y), torch.isnan(yr)) and torch.equal(torch.nan_to_num(y), torch.nan_to_num(yr))
    assert not y.requires_grad


def test_max_pool_unsupported_module_is_a_counted_fallback():
    from cim_amd import _lib
    from cim_amd.ops import fallback, max_pool2d
    x = torch.randn(1, 2, 9, 9, device=_dev())
    m = nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    with pytest.raises(_lib.CimHipError):             # a library branch is an error by default
        max_pool2d(x, m)
    with fallback.allowed("max_pool2d"):
        assert torch.equal(max_pool2d(x, m), m(x))


@pytest.mark.parametrize("shape,scale", [((1, 96, 17, 23), 2), ((1, 192, 9, 12), 4), ((2, 7, 5, 6), 8), ((1, 3, 4, 4), 1)])
def test_upsample_nearest_forward_backward_equal_aten(shape, scale):
    from cim_amd.ops import upsample_nearest
    dev = _dev()
    g = torch.Generator().manual_seed(sum(shape) + scale)
    x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    m = nn.Upsample(scale_factor=scale, mode="nearest")
    y, yr = upsample_nearest(x, m), m(xr)
    assert y.shape == yr.shape and torch.equal(y, yr)
    dy = torch.randint(-4, 5, y.shape, generator=g).float().to(dev)
    y.backward(dy)
    yr.backward(dy)
    assert torch.equal(x.grad, xr.grad)
    x.grad = None
    xr.grad = None
    dy = torch.randn(y.shape, generator=g).to(dev)
    upsample_nearest(x, m).backward(dy)
    m(xr).backward(dy)
    assert float((x.grad - xr.grad).abs().max()) <= 1e-6 * float(dy.abs().max()) * scale * scale


def test_bodies_take_no_library_pooling(monkeypatch):
    """The three bodies' forward passes (tiny inputs) must not reach F.max_pool2d / F.interpolate on a GPU tensor."""
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling.model_builder import get_func
    from cim_amd.core.config import cfg
    dev = _dev()

    def boom(*a, **k):
        raise AssertionError("library pooling / interpolation reached from a body's forward")
    for preset, size in (("resnet50_voc", (1, 3, 64, 96)), ("vgg16_voc", (1, 3, 64, 96)), ("hrnet48_voc", (1, 3, 64, 96))):
        try:
            apply_preset(preset)
        except KeyError:
            continue
        torch.manual_seed(0)
        body = get_func(cfg.MODEL.CONV_BODY)().to(dev).train()
        x = torch.randn(size, device=dev)
        with monkeypatch.context() as mp:
            mp.setattr(F, "max_pool2d", boom)
            mp.setattr(F, "interpolate", boom)
            y = body(x)
        assert torch.isfinite(y).all()
        if y.requires_grad:
            y.sum().backward()
    apply_preset("resnet50_voc")


# ---- the C ABI itself: operands inside NaN, results inside sentinel memory, ATen on the CPU in float64 as the reference ----------

def _aten_maxpool(x, dy, k, s, p):
    """x [NC, H, W] float32 on the host, dy integer-valued -> (y, idx as h * W + w, dx) of ATen's CPU kernels in float64"""
    xr = x.double().unsqueeze(0).requires_grad_(True)
    y, idx = F.max_pool2d(xr, k, s, p, return_indices=True)
    y.backward(dy.double().unsqueeze(0))
    return y[0].detach(), idx[0], xr.grad[0]


def _abi_maxpool(x, dy, k, s, p):
    """The same through cim_maxpool2d_fwd (with idx) and cim_maxpool2d_bwd -> (y, idx, dx) on the host"""
    from cim_amd import _lib
    from abi_guards import _Out, _OutInt, _poisoned16      # tests/golden/abi_guards.py
    dev = _dev()
    NC, H, W = x.shape
    Ho, Wo = (_lib.call("cim_maxpool2d_out_size", n, k, s, p) for n in (H, W))
    assert (NC, Ho, Wo) == tuple(dy.shape)
    xd, dyd = _poisoned16(x.to(dev)), _poisoned16(dy.to(dev))
    y, idx = _Out(NC * Ho, Wo, 0, dev), _OutInt(NC * Ho, Wo, 0, dev, torch.int32)
    _lib.call("cim_maxpool2d_fwd", xd.data_ptr(), y.ptr, idx.ptr, NC, H, W, k, s, p, _lib.stream_ptr())
    torch.cuda.synchronize()
    yv, iv = y.check(finite=False), idx.check()
    dx = _Out(NC * H, W, 0, dev)
    _lib.call("cim_maxpool2d_bwd", dyd.data_ptr(), iv.data_ptr(), dx.ptr, NC, H, W, k, s, p, _lib.stream_ptr())
    torch.cuda.synchronize()
    return yv.cpu().view(NC, Ho, Wo), iv.cpu().view(NC, Ho, Wo), dx.check().cpu().view(NC, H, W)


@pytest.mark.parametrize("shape,k,s,p", [((3, 8, 70), 2, 3, 0), ((3, 8, 70), 7, 1, 3), ((3, 8, 70), 7, 2, 3), ((3, 8, 70), 1, 1, 0),
                                         ((3, 7, 7), 7, 1, 3), ((2, 1, 1), 3, 1, 1), ((2, 1, 70), 3, 1, 1), ((2, 2, 130), 3, 2, 1),
                                         ((2, 1, 1), 1, 1, 0)])
def test_max_pool_abi_geometries_equal_aten(shape, k, s, p):
    """Stride above the kernel (pixels in no window: gradient exactly 0), k = 7, 1 x 1 maps, one-row maps wider than a block.
    Values and arg-max equal ATen's; gradients are integers, so the backward's sums are exact in any order."""
    g = torch.Generator().manual_seed(sum(shape) + 10 * k + s)
    NC, H, W = shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    for ties in (False, True):
        x = torch.randint(-3, 4, shape, generator=g).float() if ties else torch.randn(shape, generator=g)
        dy = torch.randint(1, 9, (NC, Ho, Wo), generator=g).float()         # positive: a window's gradient cannot cancel
        ry, ridx, rdx = _aten_maxpool(x, dy, k, s, p)
        y, idx, dx = _abi_maxpool(x, dy, k, s, p)
        assert torch.equal(y.double(), ry), ties
        assert torch.equal(idx.long(), ridx), ties
        assert torch.equal(dx.double(), rdx), ties
        if s > k:                                                            # rows / columns between the windows
            h, w = torch.arange(H), torch.arange(W)
            outside = ((h % s >= k) | (h // s >= Ho))[:, None] | ((w % s >= k) | (w // s >= Wo))[None, :]
            assert bool(outside.any()) and bool((dx[:, outside].view(torch.int32) == 0).all())


def test_max_pool_abi_plane_of_minus_infinity():
    """A plane of -inf: the value is -inf and the arg-max the window's first element, as ATen has them"""
    shape, (k, s, p) = (3, 6, 9), (3, 2, 1)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g)
    x[1] = float("-inf")
    dy = torch.randint(1, 9, (3, 3, 5), generator=g).float()
    ry, ridx, rdx = _aten_maxpool(x, dy, k, s, p)
    y, idx, dx = _abi_maxpool(x, dy, k, s, p)
    assert bool(torch.isinf(y[1]).all()) and torch.equal(y.double(), ry)
    oh, ow = torch.arange(3), torch.arange(5)
    first = (torch.clamp(oh * s - p, min=0) * 9)[:, None] + torch.clamp(ow * s - p, min=0)[None, :]
    assert torch.equal(idx[1].long(), first) and torch.equal(idx.long(), ridx)
    assert torch.equal(dx.double(), rdx)


@pytest.mark.parametrize("scale", [1, 2, 8])
def test_upsample_nearest_abi_accumulates_or_overwrites(scale):
    """accumulate = 1: y0 + upsample(x) (integers and halves: the sum is exact); accumulate = 0: a NaN-preset y is overwritten"""
    from cim_amd import _lib
    from abi_guards import _Out, _poisoned16      # tests/golden/abi_guards.py
    dev = _dev()
    NC, H, W = 3, 5, 9
    g = torch.Generator().manual_seed(scale)
    x = torch.randint(-8, 9, (NC, H, W), generator=g).float() / 2
    y0 = torch.randint(-8, 9, (NC, H * scale, W * scale), generator=g).float() / 2
    up = F.interpolate(x.double().unsqueeze(0), scale_factor=scale, mode="nearest")[0]
    xd = _poisoned16(x.to(dev))
    for accumulate, want in ((1, y0.double() + up), (0, up)):
        y = _Out(NC * H * scale, W * scale, 0, dev)                          # preset to a NaN
        if accumulate:
            y.view.copy_(y0.view(NC * H * scale, W * scale))
        _lib.call("cim_upsample_nearest_fwd", xd.data_ptr(), y.ptr, NC, H, W, scale, accumulate, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(y.check().cpu().view(NC, H * scale, W * scale).double(), want), accumulate
    assert bool((up != 0).any()) and not torch.equal(y0.double() + up, y0.double())


def test_pool_abi_refusals():
    """The CIM_CHECK_ARG lines of csrc/pool.hip: k = 8, 2 pad > k, scale = 65; nothing is written"""
    from cim_amd import _lib
    from abi_guards import SENT, _Out, _OutInt, _poisoned16      # tests/golden/abi_guards.py
    dev = _dev()
    x = _poisoned16(torch.zeros(2, 16, 16, device=dev))
    y, idx = _Out(2 * 16, 16, 0, dev), _OutInt(2 * 16, 16, 0, dev, torch.int32)
    s = _lib.stream_ptr()
    for k, st, p in ((8, 1, 3), (3, 1, 2), (2, 2, 2), (0, 1, 0), (3, 0, 1)):
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_maxpool2d_fwd", x.data_ptr(), y.ptr, idx.ptr, 2, 16, 16, k, st, p, s)
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_maxpool2d_bwd", x.data_ptr(), idx.ptr, y.ptr, 2, 16, 16, k, st, p, s)
    for scale in (65, 0):
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_upsample_nearest_fwd", x.data_ptr(), y.ptr, 2, 16, 16, scale, 0, s)
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_upsample_nearest_fwd", x.data_ptr(), y.ptr, 2, 16, 16, scale, 1, s)
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_upsample_nearest_bwd", y.ptr, x.data_ptr(), 2, 16, 16, scale, s)
    torch.cuda.synchronize()
    assert bool((y.raw == SENT).all()) and idx.untouched() and not bool(torch.isnan(x).any())
