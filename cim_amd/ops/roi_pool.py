"""RoIPool on MI355X behind the reference's operator API (FAST_RCNN.ROI_XFORM_METHOD = RoIPoolF).

Mirrors `mmcv.ops.RoIPool` / `roi_pool` as re-exported by lib/ops/__init__.py:6 and called at
lib/modeling/model_builder.py:227-228 (same constructor arguments, same NCHW tensor semantics,
autograd-enabled), plus the fused (box_x, box_x * mask) concat MaskFuse reads.  The contract of the arithmetic is in
include/cim_hip.h; tensors are kept in torch.channels_last memory format internally: the HIP kernels
(cim_amd/csrc/roi_pool.hip) run with lanes along C.  No CPU path: CPU tensors raise.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.nn.modules.utils import _pair

from .. import _lib
from . import gemm as _gemm
from .roi_align import _empty_nhwc, _nhwc


def _check(feat, rois):
    if not feat.is_cuda:
        raise _lib.CimHipError("cim_amd.ops.roi_pool: the HIP path needs CUDA/HIP tensors (no CPU fallback)")
    if feat.dtype != torch.float32:
        raise TypeError("roi_pool: float32 features expected, got %s" % feat.dtype)
    if rois.dim() != 2 or rois.size(1) != 5:
        raise ValueError("roi_pool: rois must be [K,5] (batch_idx, x1, y1, x2, y2)")


def _square(output_size):
    P, P2 = _pair(output_size)
    if P != P2:
        raise ValueError("roi_pool: square output_size expected, got %s" % (output_size,))
    return int(P)


def _argmax(ctx, feat, k, c, p):
    """The int32 [K,P,P,C] winners the backward reads - only where a gradient can be asked for (under torch.no_grad(), or with a
    feature map that does not require one, NULL: nothing is stored)."""
    if not ctx.needs_input_grad[0]:
        return None
    return torch.empty((k, p, p, c), dtype=torch.int32, device=feat.device)


def _scratch(k, b, c, h, w, p, device):
    """Per-ROI-group partial maps of the backward (a name in the caller, not a temporary inside the call: it must outlive the
    launch; the caching allocator hands the block out again in stream order)."""
    nbytes = _lib.call("cim_roi_pool_bwd_scratch", k, b, c, h, w, p)
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device) if nbytes else None


class RoIPoolFunction(Function):
    @staticmethod
    def forward(ctx, feat, rois, output_size, spatial_scale):
        _check(feat, rois)
        P = _square(output_size)
        argmax = _argmax(ctx, feat, rois.size(0), feat.size(1), P)
        feat = _nhwc(feat)
        rois = rois.to(torch.float32).contiguous()
        B, C, H, W = feat.shape
        K = rois.size(0)
        out = _empty_nhwc(K, C, P, P, feat)
        _lib.call("cim_roi_pool_fwd", feat.data_ptr(), rois.data_ptr(), out.data_ptr(), _lib.ptr(argmax), B, C, H, W, K, P,
                  float(spatial_scale), _lib.stream_ptr())
        ctx.save_for_backward(rois, argmax)
        ctx.geom = (B, C, H, W, K, P, float(spatial_scale))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rois, argmax = ctx.saved_tensors
        B, C, H, W, K, P, scale = ctx.geom
        grad_out = _nhwc(grad_out)
        grad_in = _empty_nhwc(B, C, H, W, grad_out)
        scratch = _scratch(K, B, C, H, W, P, grad_out.device)
        _lib.call("cim_roi_pool_bwd", grad_out.data_ptr(), rois.data_ptr(), argmax.data_ptr(), grad_in.data_ptr(), B, C, H, W, K, P,
                  scale, _lib.ptr(scratch), _lib.stream_ptr())
        return grad_in, None, None, None


class RoIPoolMaskCatFunction(Function):
    """Fused roi_pool -> (box_x, box_x * mask) channel concat: the input of MaskFuse.mask_branch
    (lib/modeling/resnet50.py:121-134) under ROI_XFORM_METHOD = RoIPoolF.  box_x is never stored."""

    @staticmethod
    def forward(ctx, feat, rois, masks, output_size, spatial_scale):
        _check(feat, rois)
        P = _square(output_size)
        argmax = _argmax(ctx, feat, rois.size(0), feat.size(1), P)
        feat = _nhwc(feat)
        rois = rois.to(torch.float32).contiguous()
        masks = masks.to(torch.float32).contiguous()
        B, C, H, W = feat.shape
        K = rois.size(0)
        if tuple(masks.shape) != (K, P, P):
            raise ValueError("roi_pool_maskcat: masks must be [K,P,P]")
        cat = _empty_nhwc(K, 2 * C, P, P, feat)
        _lib.call("cim_roi_pool_maskcat_fwd", feat.data_ptr(), rois.data_ptr(), masks.data_ptr(), cat.data_ptr(), _lib.ptr(argmax),
                  B, C, H, W, K, P, float(spatial_scale), _lib.stream_ptr())
        ctx.save_for_backward(rois, masks, argmax)
        ctx.geom = (B, C, H, W, K, P, float(spatial_scale))
        return cat

    @staticmethod
    def backward(ctx, grad_cat):
        rois, masks, argmax = ctx.saved_tensors
        B, C, H, W, K, P, scale = ctx.geom
        grad_cat = _nhwc(grad_cat)
        grad_in = _empty_nhwc(B, C, H, W, grad_cat)
        scratch = _scratch(K, B, C, H, W, P, grad_cat.device)
        _lib.call("cim_roi_pool_maskcat_bwd", grad_cat.data_ptr(), rois.data_ptr(), masks.data_ptr(), argmax.data_ptr(),
                  grad_in.data_ptr(), B, C, H, W, K, P, scale, _lib.ptr(scratch), _lib.stream_ptr())
        _gemm.run_postponed(grad_cat.device)        # MaskFuse's late weight gradients start behind this launch (ops/gemm.py)
        return grad_in, None, None, None, None


def roi_pool(input, rois, output_size, spatial_scale=1.0):
    return RoIPoolFunction.apply(input, rois, output_size, spatial_scale)


def roi_pool_maskcat(input, rois, masks, output_size, spatial_scale=1.0):
    return RoIPoolMaskCatFunction.apply(input, rois, masks, output_size, spatial_scale)


class RoIPool(nn.Module):
    """Same constructor as mmcv.ops.RoIPool (positional: output_size, spatial_scale), so
    `RoIPool(resolution, spatial_scale)(feat, rois)` at model_builder.py:227-228 works unchanged."""

    def __init__(self, output_size, spatial_scale=1.0):
        super().__init__()
        self.output_size = _pair(output_size)
        _square(self.output_size)
        self.spatial_scale = float(spatial_scale)

    def forward(self, input, rois):
        return roi_pool(input, rois, self.output_size, self.spatial_scale)

    def __repr__(self):
        return "%s(output_size=%s, spatial_scale=%s)" % (self.__class__.__name__, self.output_size, self.spatial_scale)
