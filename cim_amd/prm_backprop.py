"""PRM peak back-propagation on the device: the peak response maps.

Replaces what `PeakResponseMapping(...).inference()` of lib/prm/prm_model_gt.py:249-310 does behind its forward pass: every valid
peak is sent back through the network under the probability-normalised rule of lib/prm/prm_modules.py:104-140 (every nn.Conv2d:
o = min x, xs = x - o, n = conv(xs, W+), ghat = n < 1e-10 ? 0 : g / (|n| + 1e-10), dx = xs * conv_transpose(ghat, W+), W+ =
max(W, 0); everything else its ordinary adjoint), down to the image; the map of a peak is the image gradient summed over the three
channels, clamped at 0 and divided by its sum.  The reference runs P sequential batch-1 backward passes; here ONE forward pass keeps
each convolution's xs, y and n, and ONE backward walk carries all peaks of a chunk in its batch dimension:

    maps = prm.backprop(model, image, peaks)                       # image [1,3,H,W], peaks [P,3] (class, y, x) -> [P,H,W]
    out = prm.peak_response_maps(model, images, labels)            # per image: (rows, cols, classes, scores, maps)

The products are the body's own data-gradient kernels with w = W+ (ops/conv1x1.py, ops/conv3x3.py: dy_is_dconv, B = chunk); the
stages between them and the stem's data gradient are csrc/prm_backprop.hip.  Takes DEVICE tensors; a CPU tensor is an error (no
CPU fallback)."""
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .modeling.resnet50 import Bottleneck
from .ops import conv1x1 as _c1
from .ops import conv1x1_bn_act, conv3x3_bn_act, conv7x7_bn_act

CHUNK_BYTES = 256 << 20      # the largest gradient tensor of a chunk (layer1's output: 4 width (H / 4) (W / 4) floats per peak) stays under this
CHUNK_MAX = 64
_WtDesc = _lib.STRUCTS["cim_wt_desc"]


def default_chunk(width, height, width_px, peaks):
    """chunk = min(P, 64, CHUNK_BYTES // (4 width * ceil(H / 4) * ceil(W / 4) * 4 bytes)), at least 1: at width 64 and 448 x 448 one
    peak's layer1 gradient is 12.8 MB, so 20 peaks per walk."""
    per_peak = 4 * int(width) * ((int(height) + 3) // 4) * ((int(width_px) + 3) // 4) * 4
    return max(1, min(int(peaks), CHUNK_MAX, CHUNK_BYTES // max(per_peak, 1)))


def _parts(model, who):
    """(features, classifier convolution) of a PeakResponseMapping over an FC_ResNet built from ResNetBody; TypeError otherwise."""
    from . import prm
    if not isinstance(model, prm.PeakResponseMapping) or len(model) != 1 or not isinstance(model[0], prm.FC_ResNet):
        raise TypeError("cim_amd.prm.%s: a cim_amd.prm.PeakResponseMapping over a cim_amd.prm.FC_ResNet is expected" % who)
    f, cls = model[0].features, model[0].classifier[0]
    ok = (len(f) == 8 and isinstance(f[0], nn.Conv2d) and isinstance(f[1], nn.BatchNorm2d) and isinstance(f[3], nn.MaxPool2d)
          and f[0].kernel_size == (7, 7) and f[0].stride == (2, 2) and f[0].padding == (3, 3) and f[0].in_channels == 3
          and f[0].bias is None and f[0].out_channels <= 256
          and (f[3].kernel_size, f[3].stride, f[3].padding) in ((3, 2, 1), ((3, 3), (2, 2), (1, 1)))
          and f[0].dilation == (1, 1) and f[0].groups == 1
          and all(isinstance(f[i], nn.Sequential) and len(f[i]) > 0 and all(isinstance(b, Bottleneck) for b in f[i]) for i in range(4, 8))
          and all(_block_ok(b) for i in range(4, 8) for b in f[i])
          and isinstance(cls, nn.Conv2d) and _plain(cls, 1, (1, 1), 0))
    if not ok:
        raise TypeError("cim_amd.prm.%s: the body must be built from cim_amd.prm.ResNetBody (7 x 7 / 2 stem of 3 channels, 3 x 3 / 2 "
                        "max-pool, four stages of cim_amd.modeling.resnet50.Bottleneck - 1 x 1 / 1, 3 x 3 / 1 or 2, 1 x 1 / 1, the "
                        "projection 1 x 1 with the 3 x 3's stride, no dilation, no groups, no bias - and a 1 x 1 classifier)" % who)
    return f, cls


def _plain(conv, k, stride, pad, bias=True):
    """An undilated, ungrouped k x k convolution of the given stride and padding (bias=False: without a bias)."""
    return (conv.kernel_size == (k, k) and conv.stride == stride and conv.padding == (pad, pad) and conv.dilation == (1, 1)
            and conv.groups == 1 and (bias or conv.bias is None))


def _block_ok(b):
    """The geometry the walk assumes of a bottleneck: the stride sits on the 3 x 3 (the stride-2 1 x 1 of a stride_1x1 body would
    see every second pixel of xs, which `n1` and the data gradient here do not), and the projection strides with it."""
    s = b.conv2.stride
    ok = (s in ((1, 1), (2, 2)) and _plain(b.conv1, 1, (1, 1), 0, False) and _plain(b.conv2, 3, s, 1, False)
          and _plain(b.conv3, 1, (1, 1), 0, False))
    if b.downsample is None:
        return ok and s == (1, 1)
    return (ok and len(b.downsample) == 2 and isinstance(b.downsample[0], nn.Conv2d) and isinstance(b.downsample[1], nn.BatchNorm2d)
            and _plain(b.downsample[0], 1, s, 0, False))


# ---- W+ and the BatchNorm scales: made once per model, cached against the parameters' versions --------------------------------
class _Layer(object):
    """One convolution of the walk: wpos (W+ in the layout of W), a = gamma rsqrt(var + eps) of the BatchNorm behind it (None for
    the classifier), wt (3 x 3 only: W+ as [cout][3][3][cin], the data gradient's A operand)."""
    __slots__ = ("conv", "bn", "wpos", "a", "wt")

    def __init__(self, conv, bn):
        self.conv, self.bn, self.wt = conv, bn, None
        self.wpos = torch.clamp(conv.weight.detach(), min=0).contiguous()
        self.a = (bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)).contiguous() if bn is not None else None


_PLANS = {}      # id(model) -> (weak reference, signature, plan)


def _signature(model):
    return tuple((id(t), t._version, t.data_ptr()) for t in list(model.parameters()) + list(model.buffers()))


def _plan(model, f, cls):
    key, sig = id(model), _signature(model)
    e = _PLANS.get(key)
    if e is not None and e[0]() is model and e[1] == sig:
        return e[2]
    with torch.no_grad():
        plan = {"stem": _Layer(f[0], f[1]), "cls": _Layer(cls, None), "blocks": []}
        for i in range(4, 8):
            for blk in f[i]:
                plan["blocks"].append({"block": blk, "c1": _Layer(blk.conv1, blk.bn1), "c2": _Layer(blk.conv2, blk.bn2),
                                       "c3": _Layer(blk.conv3, blk.bn3),
                                       "ds": _Layer(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None})
        threes = [b["c2"] for b in plan["blocks"]]
        buf = torch.empty(sum(l.wpos.numel() for l in threes), dtype=torch.float32, device=threes[0].wpos.device)
        descs, o = (_WtDesc * len(threes))(), 0
        for i, l in enumerate(threes):
            l.wt = buf[o:o + l.wpos.numel()]
            o += l.wpos.numel()
            descs[i] = _WtDesc(l.wpos.data_ptr(), l.wt.data_ptr(), l.wpos.shape[1], l.wpos.shape[0])
        _lib.call("cim_conv3x3_wt_multi", descs, len(threes), _lib.stream_ptr())
    _PLANS[key] = (weakref.ref(model, lambda _r, key=key: _PLANS.pop(key, None)), sig, plan)
    return plan


# ---- the forward pass that keeps xs, y and n ----------------------------------------------------------------------------------
def _shift(x):
    """xs = x - min(x): two launches for the minimum into a device scalar, one for the shift; no host read."""
    n = x.numel()
    part = torch.empty(int(_lib.call("cim_prmb_min_parts", n)) + 1, dtype=torch.float32, device=x.device)
    xs = torch.empty_like(x)
    st = _lib.stream_ptr()
    _lib.call("cim_prmb_min", x.data_ptr(), n, part.data_ptr(), part.data_ptr() + 4, st)
    _lib.call("cim_prmb_shift", x.data_ptr(), part.data_ptr(), xs.data_ptr(), n, st)
    return xs


def _norm1x1(xs, wpos):
    """n = W+ . xs of one image [cin, h, w] on the small-tile GEMM with the identity epilogue."""
    cin, h, w = xs.shape
    cout, hw = wpos.shape[0], h * w
    n = torch.empty((cout, h, w), dtype=torch.float32, device=xs.device)
    _c1._gemm(wpos.reshape(cout, cin), xs, n, cout, hw, cin, cin, hw, hw, False, False)
    return n


def _norm3x3(xs, wpos, stride):
    cin, h, w = xs.shape
    cout = wpos.shape[0]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    n = torch.empty((cout, ho, wo), dtype=torch.float32, device=xs.device)
    splits = _lib.call("cim_conv3x3_nchw_splits", cin, cout, h, w, stride)
    ws = torch.empty(splits * cout * ho * wo, dtype=torch.float32, device=xs.device) if splits > 1 else None
    _lib.call("cim_conv3x3_nchw_f32", xs.data_ptr(), wpos.data_ptr(), n.data_ptr(), cin, cout, h, w, stride, 1, None, None, None, None, None,
              0.0, None, 0, splits, _lib.ptr(ws), _lib.stream_ptr())
    return n


def _norm7x7(xs, wpos):
    cin, h, w = xs.shape
    cout = wpos.shape[0]
    n = torch.empty((cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=xs.device)
    _lib.call("cim_conv7x7_nchw_f32", xs.data_ptr(), wpos.data_ptr(), n.data_ptr(), cin, cout, h, w, 2, None, None, None, None, 0.0, 0,
              _lib.stream_ptr())
    return n


class Forward(object):
    """What one forward pass of ONE image leaves for the backward walk: per convolution xs (its shifted input), n (its normaliser)
    and y (the post-activation output the ReLU gate reads); the max-pool's arg-max; `crm`, the class response maps [1, C, h, w] -
    the values `model(image)` gives, from the same launches."""

    def __init__(self, model, image, who="backprop"):
        from . import prm
        f, cls = _parts(model, who)
        plan = _plan(model, f, cls)
        self.plan, self.shape = plan, tuple(int(s) for s in image.shape)
        with torch.no_grad():
            image = image.contiguous()
            st = plan["stem"]
            self.xs0 = _shift(image[0])
            self.n0 = _norm7x7(self.xs0, st.wpos)
            self.y0 = conv7x7_bn_act(image, f[0], f[1], relu=True)
            _, c, h, w = self.y0.shape
            k, s, p = 3, 2, 1
            ho, wo = _lib.call("cim_maxpool2d_out_size", h, k, s, p), _lib.call("cim_maxpool2d_out_size", w, k, s, p)
            x = torch.empty((1, c, ho, wo), dtype=torch.float32, device=image.device)
            self.pool_idx = torch.empty((c, ho, wo), dtype=torch.int32, device=image.device)
            _lib.call("cim_maxpool2d_fwd", self.y0.data_ptr(), x.data_ptr(), self.pool_idx.data_ptr(), c, h, w, k, s, p, _lib.stream_ptr())
            self.blocks = []
            for b in plan["blocks"]:
                blk, rec = b["block"], {}
                rec["xs"] = _shift(x[0])
                rec["n1"] = _norm1x1(rec["xs"], b["c1"].wpos)
                y1 = conv1x1_bn_act(x, blk.conv1, blk.bn1)
                rec["y1"], rec["xs1"] = y1, _shift(y1[0])
                rec["n2"] = _norm3x3(rec["xs1"], b["c2"].wpos, blk.conv2.stride[0])
                y2 = conv3x3_bn_act(y1, blk.conv2, blk.bn2)
                rec["y2"], rec["xs2"] = y2, _shift(y2[0])
                rec["n3"] = _norm1x1(rec["xs2"], b["c3"].wpos)
                identity = x
                if b["ds"] is not None:
                    s = blk.downsample[0].stride[0]
                    identity = conv1x1_bn_act(x, blk.downsample[0], blk.downsample[1], relu=False)
                    # (the minimum is the whole input's; a strided 1 x 1 convolution then sees every s-th pixel of xs)
                    rec["nd"] = _norm1x1(rec["xs"][:, ::s, ::s].contiguous() if s != 1 else rec["xs"], b["ds"].wpos)
                x = conv1x1_bn_act(y2, blk.conv3, blk.bn3, residual=identity)
                rec["y3"] = x
                self.blocks.append(rec)
            self.xsf = _shift(x[0])
            self.nf = _norm1x1(self.xsf, plan["cls"].wpos)
            self.crm = prm._classify(x, cls)


# ---- the backward walk --------------------------------------------------------------------------------------------------------
def _gate(g, mul, y, a, n, want_res=False):
    """cim_prmb_gate on g [P, C, ...]: -> (dconv, dres or None)."""
    p, c = int(g.shape[0]), int(g.shape[1])
    hw = g.numel() // (p * c)
    dconv = torch.empty_like(g)
    dres = torch.empty_like(g) if want_res else None
    _lib.call("cim_prmb_gate", g.data_ptr(), _lib.ptr(mul), _lib.ptr(y), _lib.ptr(a), n.data_ptr(), dconv.data_ptr(), _lib.ptr(dres), p, c,
              hw, _lib.stream_ptr())
    return dconv, dres


def _scale(xs, dxraw, add=None):
    dx = torch.empty_like(dxraw)
    _lib.call("cim_prmb_scale", xs.data_ptr(), dxraw.data_ptr(), _lib.ptr(add), dx.data_ptr(), int(dxraw.shape[0]), xs.numel(),
              _lib.stream_ptr())
    return dx


def _dx1x1(layer, dconv, in_shape, dx_add=None, dx_add_w=0):
    """W+^T . dconv for the P images of dconv [P, cout, ...]: the body's 1 x 1 data gradient (dy_is_dconv, no weight gradient)."""
    p, cout = int(dconv.shape[0]), int(dconv.shape[1])
    cin, h, w = in_shape
    hw = h * w
    dx = torch.empty((p, cin, h, w), dtype=torch.float32, device=dconv.device)
    ws = torch.empty(_lib.call("cim_conv1x1_bwd_workspace", p, cin, cout, hw) // 4, dtype=torch.float32, device=dconv.device)
    wp = layer.wpos.data_ptr()          # (x_raw, x, gamma, mean, var are not read with dy_is_dconv and no dw: any valid pointer)
    _lib.call("cim_conv1x1_bn_act_bwd", dconv.data_ptr(), None, wp, wp, wp, wp, wp, wp, 0.0, 0, None, None, None, dx.data_ptr(), None,
              p, cin, cout, hw, ws.data_ptr(), _lib.stream_ptr(), None, None, None, 1, 1, None, None, 0.0, None, None, None,
              _lib.ptr(dx_add), int(dx_add_w))
    return dx


def _dx3x3(layer, dconv, in_shape, stride):
    p, cout = int(dconv.shape[0]), int(dconv.shape[1])
    cin, h, w = in_shape
    dx = torch.empty((p, cin, h, w), dtype=torch.float32, device=dconv.device)
    ws = torch.empty(_lib.call("cim_conv3x3_nchw_bwd_workspace", p, cin, cout, h, w, stride) // 4, dtype=torch.float32, device=dconv.device)
    wp = layer.wpos.data_ptr()
    _lib.call("cim_conv3x3_nchw_bn_act_bwd", dconv.data_ptr(), None, wp, wp, wp, wp, wp, wp, 0.0, 0, None, None, None, dx.data_ptr(), None,
              p, cin, cout, h, w, stride, 1, ws.data_ptr(), _lib.stream_ptr(), None, None, None, 1, 1, None, None, 0.0, None, None, None,
              layer.wt.data_ptr())
    return dx


def _walk(fwd, peaks_dev, factor, out):
    """One chunk: peaks_dev [P, 3] int32 on the device -> out [P, H, W] (written)."""
    plan = fwd.plan
    p = int(peaks_dev.shape[0])
    dev = out.device
    _, c, h, w = fwd.crm.shape
    dconv = torch.empty((p, c, h, w), dtype=torch.float32, device=dev)
    _lib.call("cim_prmb_seed", peaks_dev.data_ptr(), fwd.nf.data_ptr(), dconv.data_ptr(), p, c, h, w, factor, _lib.stream_ptr())
    g = _scale(fwd.xsf, _dx1x1(plan["cls"], dconv, tuple(fwd.xsf.shape)))
    for b, rec in zip(reversed(plan["blocks"]), reversed(fwd.blocks)):
        blk = b["block"]
        stride = blk.conv2.stride[0]
        # g: the gradient of the block's output y3 = relu(bn3(conv3(y2)) + identity)
        d3, dres = _gate(g, None, rec["y3"], b["c3"].a, rec["n3"], want_res=b["ds"] is None)
        dd = _gate(g, None, rec["y3"], b["ds"].a, rec["nd"])[0] if b["ds"] is not None else None
        del g
        r3 = _dx1x1(b["c3"], d3, tuple(rec["xs2"].shape))
        d2, _ = _gate(r3, rec["xs2"], rec["y2"], b["c2"].a, rec["n2"])            # (the multiply by conv3's xs rides in this gate)
        del d3, r3
        r2 = _dx3x3(b["c2"], d2, tuple(rec["xs1"].shape), stride)
        d1, _ = _gate(r2, rec["xs1"], rec["y1"], b["c1"].a, rec["n1"])
        del d2, r2
        xin = tuple(rec["xs"].shape)
        if dd is not None:
            # conv1 and the projection read the same xs: their raw data gradients are added in conv1's epilogue (a stride-2
            # projection's at the pixels (2i, 2j) it belongs to), one multiply by xs serves both
            s = blk.downsample[0].stride[0]
            rd = _dx1x1(b["ds"], dd, (xin[0], (xin[1] - 1) // s + 1, (xin[2] - 1) // s + 1))
            r1 = _dx1x1(b["c1"], d1, xin, dx_add=rd, dx_add_w=xin[2] if s == 2 else 0)
            g = _scale(rec["xs"], r1)
        else:
            g = _scale(rec["xs"], _dx1x1(b["c1"], d1, xin), add=dres)
    _, c0, h0, w0 = fwd.y0.shape
    dpool = torch.empty((p, c0, h0, w0), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr()
    for i in range(p):                       # the arg-max belongs to the image: one launch per peak, nothing replicated
        _lib.call("cim_maxpool2d_bwd", g[i].data_ptr(), fwd.pool_idx.data_ptr(), dpool[i].data_ptr(), c0, h0, w0, 3, 2, 1, st)
    d0, _ = _gate(dpool, None, fwd.y0, plan["stem"].a, fwd.n0)
    hh, ww = fwd.shape[2], fwd.shape[3]
    ws = torch.empty(_lib.call("cim_prmb_stem_workspace", p, hh, ww) // 8, dtype=torch.float64, device=dev)
    _lib.call("cim_prmb_stem", d0.data_ptr(), plan["stem"].wpos.data_ptr(), fwd.xs0.data_ptr(), out.data_ptr(), ws.data_ptr(), p, c0, hh, ww,
              1, st)


def _host_peaks(peaks, who):
    """peaks as a host int64 array [P, 3].  A host array / list / CPU tensor is checked without touching the device; a device
    tensor is read (one synchronisation)."""
    if torch.is_tensor(peaks):
        if peaks.dtype.is_floating_point or peaks.dtype == torch.bool:
            raise ValueError("cim_amd.prm.%s: peaks must be integers [P, 3] = (class, y, x), got %s" % (who, peaks.dtype))
        peaks = peaks.detach().cpu().numpy()
    a = np.asarray(peaks)
    if a.size == 0:
        return np.zeros((0, 3), dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
        raise ValueError("cim_amd.prm.%s: peaks must be integers [P, 3] = (class, y, x), got %s %s" % (who, a.shape, a.dtype))
    return a.astype(np.int64)


def _check_image(image, who, batch_one):
    """Shape and type of the image tensor; where it lives is asked last (`_check_device`), so that every other refusal is the same
    on the host and on the device."""
    if not torch.is_tensor(image):
        raise _lib.CimHipError("cim_amd.prm.%s: CUDA/HIP tensor expected (no CPU fallback)" % who)
    if image.dim() != 4 or image.shape[1] != 3 or image.dtype != torch.float32:
        raise ValueError("cim_amd.prm.%s: image must be [%s, 3, H, W] float32, got %s %s" % (who, "1" if batch_one else "B", tuple(image.shape), image.dtype))
    if batch_one and image.shape[0] != 1:
        raise ValueError("cim_amd.prm.%s: one image at a time, got a batch of %d" % (who, image.shape[0]))


def _check_device(image, who):
    if not image.is_cuda:
        raise _lib.CimHipError("cim_amd.prm.%s: CUDA/HIP tensor expected (no CPU fallback)" % who)


def _check_peaks(pk, classes, grid_h, grid_w, who):
    for i, (c, y, x) in enumerate(pk.tolist()):
        if not 0 <= c < classes:
            raise ValueError("cim_amd.prm.%s: peak %d names class %d, outside 0..%d" % (who, i, c, classes - 1))
        if not (0 <= y < grid_h and 0 <= x < grid_w):
            raise ValueError("cim_amd.prm.%s: peak %d at (%d, %d), outside the %d x %d up-sampled grid" % (who, i, y, x, grid_h, grid_w))


def _grid(f, h, w, factor):
    """The up-sampled grid of an H x W image: stem / 2, max-pool / 2, every stage's own stride, then x factor."""
    half = lambda v: (v - 1) // 2 + 1
    h, w = half(half(h)), half(half(w))
    for i in range(4, 8):
        for _ in range(f[i][0].conv2.stride[0] // 2):
            h, w = half(h), half(w)
    return h * factor, w * factor


def _run(fwd, pk, factor, chunk, who):
    _, _, hh, ww = fwd.shape
    p = pk.shape[0]
    dev = fwd.crm.device
    out = torch.empty((p, hh, ww), dtype=torch.float32, device=dev)
    if chunk is None:
        chunk = default_chunk(fwd.y0.shape[1], hh, ww, p)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("cim_amd.prm.%s: chunk = %d" % (who, chunk))
    # (pinned + non_blocking: a pageable copy would make the host wait for everything already on the stream)
    pinned = torch.from_numpy(np.ascontiguousarray(pk, dtype=np.int32)).pin_memory()
    peaks_dev = pinned.to(dev, non_blocking=True)
    with torch.no_grad():
        for lo in range(0, p, chunk):
            _walk(fwd, peaks_dev[lo:lo + chunk], factor, out[lo:lo + chunk])
    return out


def backprop(model, image, peaks, chunk=None):
    """The peak response maps of GIVEN peaks: image [1, 3, H, W] normalised fp32 on the device, peaks [P, 3] integers = (class, y,
    x) on the up-sampled grid (a host array, list or CPU tensor: checked without touching the device; a device tensor is read
    first) -> [P, H, W] fp32 on the device, one map per peak in the order given; no host synchronisation.  A peak through which
    no gradient reaches the image (a class whose classifier row has no positive weight) gives an all-NaN map (0 / 0, as the
    reference).  chunk: peaks per backward walk (default: `default_chunk`).  P = 0 returns an empty [0, H, W] without a launch.
    Refused before any launch, in this order: a body not built from ResNetBody (TypeError), a batch other than 1, a peak outside
    the classes or the up-sampled grid (ValueError), a CPU tensor (CimHipError: no CPU fallback)."""
    f, cls = _parts(model, "backprop")
    _check_image(image, "backprop", True)
    pk = _host_peaks(peaks, "backprop")
    factor = int(model.sub_pixel_locating_factor)
    hh, ww = int(image.shape[2]), int(image.shape[3])
    grid_h, grid_w = _grid(f, hh, ww, factor)
    _check_peaks(pk, cls.out_channels, grid_h, grid_w, "backprop")
    _check_device(image, "backprop")
    if pk.shape[0] == 0:
        return torch.empty((0, hh, ww), dtype=torch.float32, device=image.device)
    return _run(Forward(model, image), pk, factor, chunk, "backprop")


def peak_response_maps(model, images, labels, peak_threshold=10, image_sizes=None, chunk=None):
    """images [B, 3, S, S'] normalised fp32 on the device, labels = B lists of image-level classes -> per image (rows, cols,
    classes, scores, maps): the first four exactly what `cim_amd.prm.peaks` returns (host arrays, ascending peak score, the
    "no peak above the threshold -> the strongest peak of the class" fallback included), maps [P, S, S'] fp32 on the device,
    row-aligned with them - the order tools/pre/AGPL_label_assign.py uses after its sort.  One forward pass per image (its class
    response maps feed the peak launches), one read of the peaks per image, then the backward walk.  An image with an empty class
    list gets empty rows and an empty [0, S, S'] and costs no launch; all lists empty is the ValueError `peaks` raises."""
    from . import prm
    who = "peak_response_maps"
    _parts(model, who)
    _check_image(images, who, False)
    b = int(images.shape[0])
    if len(labels) != b:
        raise ValueError("cim_amd.prm.%s: %d class lists for %d images" % (who, len(labels), b))
    if not any(len(ls) for ls in labels):
        raise ValueError("cim_amd.prm: no (image, class) pair: every image has an empty class list")
    if image_sizes is not None and len(image_sizes) != b:
        raise ValueError("cim_amd.prm: %d image sizes for %d images" % (len(image_sizes), b))
    _check_device(images, who)
    factor = int(model.sub_pixel_locating_factor)
    res = []
    for i in range(b):
        if not len(labels[i]):                   # no class, no peak: what `peaks` returns for such an image, and no launch
            empty = np.zeros(0, dtype=np.int64)
            res.append((empty, empty.copy(), empty.copy(), np.zeros(0, dtype=np.float32),
                        torch.empty((0,) + tuple(images.shape[2:]), dtype=torch.float32, device=images.device)))
            continue
        fwd = Forward(model, images[i:i + 1], who)
        sizes = None if image_sizes is None else [image_sizes[i]]
        got, run = prm.peaks_from_crm(fwd.crm, [labels[i]], factor, sizes, peak_threshold, details=True)
        rows, cols, classes, scores = got[0]
        ys, xs = run.ys_xs[0]
        # (every class of the list has at least one valid peak - the fallback - so there is something to send back)
        res.append((rows, cols, classes, scores, _run(fwd, np.stack([classes, ys, xs], 1).astype(np.int64), factor, chunk, who)))
    return res
