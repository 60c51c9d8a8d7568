"""The PRM network and its peaks on the device: images -> the points `proposal_prep.assign_clusters` takes.

Replaces what tools/pre/AGPL_label_assign.py reads from lib/prm/prm_model_gt.py (`FC_ResNet`, `PeakResponseMapping`) and
lib/prm/prm_modules.py (`PeakStimulation`): ONE forward pass of a frozen-BatchNorm ResNet-50 with a 1 x 1 classifier - every
convolution + BatchNorm (+ residual) (+ ReLU) one launch of the kernels the detector's body runs on - and three launches of
csrc/prm.hip (bilinear up-sampling, median-filtered peaks, ascending-score order) for a BATCH of images.  The reference also
back-propagates every valid peak through the network (the peak response maps); the label assignment reads only their number,
which is the number of valid peaks, so `peaks` does not run that pass.  `backprop` and `peak_response_maps` (prm_backprop.py,
DESIGN.md 4.25) do: one backward walk whose batch dimension is the peaks.

    model = PeakResponseMapping(fc_resnet50(num_classes=20))          # state_dict keys of the reference: prm_voc.pth loads
    model.load_state_dict(torch.load("prm_voc.pth", map_location="cpu"), strict=True)
    rows, cols, classes, scores = peaks(model.cuda(), images, labels)[0]
    rows, cols, classes, scores, maps = peak_response_maps(model, images, labels)[0]     # + the peak response maps [P, S, S']

Takes DEVICE tensors; a CPU tensor is an error in `peaks` (no CPU fallback).  The modules themselves run on CPU tensors through
the ATen branch of the wrappers (host-side tests of the architecture)."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .modeling.resnet50 import Bottleneck, _make_layer
from .ops import conv7x7_bn_act, max_pool2d
from .ops import conv1x1 as _conv1x1
from .utils import blob as _blob

MAX_PEAKS = _lib.CONSTANTS["CIM_PRM_MAX_PEAKS"]
MAX_HW = _lib.CONSTANTS["CIM_PRM_MAX_HW"]
STATUS_TOO_MANY = _lib.CONSTANTS["CIM_PRM_STATUS_TOO_MANY"]
STATUS_NAN = _lib.CONSTANTS["CIM_PRM_STATUS_NAN"]
STATUS_NO_PEAK = _lib.CONSTANTS["CIM_PRM_STATUS_NO_PEAK"]
INPUT_SIZE = 448                    # prm_configs.open_transform: transforms.Resize([448, 448])


def _not_here(what):
    return NotImplementedError("cim_amd.prm: %s is not part of this package - the label assignment needs the peaks only: "
                               "use cim_amd.prm.peaks" % what)


class ResNetBody(nn.Module):
    """A torchvision-shaped ResNet-50 (conv1, bn1, relu, maxpool, layer1..layer4; width 64), the `model` FC_ResNet wraps.
    `width` thins every stage alike (tests)."""

    def __init__(self, width=64):
        super().__init__()
        w = int(width)
        if w < 4 or w % 4:
            raise ValueError("cim_amd.prm.ResNetBody: width = %d, a positive multiple of 4 is needed" % w)
        self.conv1 = nn.Conv2d(3, w, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(w)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = _make_layer(w, w, 3, 1)
        self.layer2 = _make_layer(4 * w, 2 * w, 4, 2)
        self.layer3 = _make_layer(8 * w, 4 * w, 6, 2)
        self.layer4 = _make_layer(16 * w, 8 * w, 3, 2)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")


_IDENTITY = {}      # (device, channels) -> (ones, zeros): the BatchNorm epilogue as y = x + bias exactly (ops/conv3x3.py: conv3x3_bias_act)


def _classify(x, conv):
    """The 1 x 1 classifier with its bias as ONE product per image on the small-tile GEMM: W [C, K] . x [K, hw], the bias in the
    BatchNorm epilogue with gamma = 1, mean = 0, var = 1, eps = 0 (a = 1 exactly, b = bias)."""
    if not x.is_cuda:
        return conv(x)
    x = x.contiguous()
    b, k, h, w = x.shape
    c, hw = conv.out_channels, h * w
    key = (x.device, c)
    if key not in _IDENTITY:
        _IDENTITY[key] = (torch.ones(c, device=x.device), torch.zeros(c, device=x.device))
    ones, zeros = _IDENTITY[key]
    bias = conv.bias if conv.bias is not None else zeros
    w2 = conv.weight.reshape(c, k)
    y = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device)
    for i in range(b):
        _conv1x1._gemm(w2, x[i], y[i], c, hw, k, k, hw, hw, False, False, bn=(ones, bias, zeros, ones), eps=0.0)
    return y


class FC_ResNet(nn.Module):
    """prm_model_gt.py:335-359: `features` = stem, max-pool, layer1..layer4 of `model`; `classifier` = a 1 x 1 convolution with
    bias over layer4's channels.  The forward pass is inference only (BatchNorm statistics frozen)."""

    def __init__(self, model, num_classes):
        super().__init__()
        self.features = nn.Sequential(model.conv1, model.bn1, model.relu, model.maxpool,
                                      model.layer1, model.layer2, model.layer3, model.layer4)
        num_features = model.layer4[1].conv1.in_channels
        self.classifier = nn.Sequential(nn.Conv2d(num_features, num_classes, kernel_size=1, bias=True))

    def forward(self, x):
        f = self.features
        if not (isinstance(f[4][0], Bottleneck) and isinstance(f[0], nn.Conv2d) and isinstance(f[3], nn.MaxPool2d)):
            raise TypeError("cim_amd.prm.FC_ResNet: `model` must be built from cim_amd.modeling.resnet50.Bottleneck (ResNetBody)")
        x = max_pool2d(conv7x7_bn_act(x, f[0], f[1], relu=True), f[3])
        for i in range(4, 8):
            x = f[i](x)
        return _classify(x, self.classifier[0])


def fc_resnet50(num_classes=20, width=64):
    """prm_model_gt.py:362-366 without the ImageNet download: the weights come from the PRM checkpoint."""
    return FC_ResNet(ResNetBody(width), num_classes)


class PeakResponseMapping(nn.Sequential):
    """prm_model_gt.py:52-331 as far as the label assignment uses it: an nn.Sequential over the backbone (state_dict keys
    `0.features.<i>...`, `0.classifier.0.{weight,bias}`), always in eval mode; `forward` returns the class response maps
    [B, C, h, w] under no_grad.  Peaks: `cim_amd.prm.peaks(model, images, labels)`."""

    def __init__(self, *args, **kargs):
        super().__init__(*args)
        self.win_size = kargs.pop("win_size", 3)
        self.sub_pixel_locating_factor = kargs.pop("sub_pixel_locating_factor", 8)
        self.filter_type = kargs.pop("filter_type", "median")
        if kargs:
            raise _not_here("PeakResponseMapping(%s)" % ", ".join(sorted(kargs)))
        if self.win_size != 3:
            raise _not_here("a peak window other than 3 x 3")
        if self.filter_type != "median":
            raise _not_here("filter_type %r (only 'median')" % (self.filter_type,))
        if int(self.sub_pixel_locating_factor) != self.sub_pixel_locating_factor or self.sub_pixel_locating_factor < 1:
            raise ValueError("cim_amd.prm: sub_pixel_locating_factor = %r, a positive integer is needed" % (self.sub_pixel_locating_factor,))
        super().train(False)

    def train(self, mode=True):
        if mode:
            raise _not_here("PRM's own classification training")
        return super().train(False)

    def inference(self):
        return self

    def forward(self, input):
        if input.dim() != 4:
            raise ValueError("cim_amd.prm.PeakResponseMapping: [B, 3, H, W] expected, got %s" % (tuple(input.shape),))
        with torch.no_grad():
            return super().forward(input)

    def instance_seg(self, *a, **k):
        raise _not_here("instance_seg (the proposal retrieval behind the peak response maps; the maps themselves: "
                        "cim_amd.prm.peak_response_maps)")

    def instance_nms(self, *a, **k):
        raise _not_here("instance_nms (the proposal retrieval behind the peak response maps; the maps themselves: "
                        "cim_amd.prm.peak_response_maps)")


def peak_response_mapping(backbone=None, win_size=3, sub_pixel_locating_factor=8, filter_type="median", **kargs):
    """prm_model_gt.py:369-386."""
    for name in ("enable_peak_stimulation", "enable_peak_backprop"):
        if not kargs.pop(name, True):
            raise _not_here("%s=False" % name)
    return PeakResponseMapping(backbone if backbone is not None else fc_resnet50(), win_size=win_size,
                               sub_pixel_locating_factor=sub_pixel_locating_factor, filter_type=filter_type, **kargs)


def peak_response_mapping_aff(*a, **k):
    raise _not_here("the _aff variant")


def peak_response_mapping_aff_vis(*a, **k):
    raise _not_here("the _visual variant")


def network_input(rgb_u8):
    """ToTensor + Normalize of prm_configs.open_transform on the device: rgb_u8 [S, S', 3] (or [B, S, S', 3]) uint8, host or
    device -> [B, 3, S, S'] fp32.  cim_image_prep at scale 1 on the channel-swapped array: (x / 255 - mean) / std in fp32, bit for
    bit (tests/test_gpu_prm.py).  For images that still need the antialiased transforms.Resize([448, 448]) in front of it:
    `network_input_from_images`."""
    t = rgb_u8 if torch.is_tensor(rgb_u8) else torch.from_numpy(np.ascontiguousarray(rgb_u8))
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError("cim_amd.prm.network_input: uint8 [H, W, 3] or [B, H, W, 3] (RGB) expected")
    if t.dim() == 3:
        t = t[None]
    if not t.is_cuda:
        t = t.cuda()
    bgr = t.flip(-1).contiguous()
    b, h, w, _ = bgr.shape
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=bgr.device)
    for i in range(b):
        _lib.call("cim_image_prep", bgr[i].data_ptr(), h, w, out[i].data_ptr(), h, w, out.stride(1), out.stride(2), 1.0, 0,
                  ctypes.cast(_blob._MS, ctypes.c_void_p), _lib.stream_ptr())
    return out


def network_input_from_images(images_u8, size=INPUT_SIZE, device=None):
    """prm_configs.open_transform whole - transforms.Resize([size, size]) (Pillow's antialiased bilinear resize), ToTensor,
    Normalize - on the device: images_u8 = uint8 [h_i, w_i, 3] RGB arrays of differing sizes (host NumPy or device tensors) ->
    [B, 3, size, size] fp32, bit for bit `network_input` of Pillow's resized bytes (cim_amd.resample): three
    launches for the batch, no host read.  `device`: where host images go (default: the current device)."""
    from . import resample
    return resample.pil_resize(images_u8, (int(size), int(size)), normalize=(_blob.MEAN, _blob.STD), device=device)


class _Launch(object):
    """The buffers of one call, owned by name until its results are read (never temporaries: the kernels run asynchronously)."""

    def __init__(self, labels, sizes, num_classes, device):
        self.b = len(labels)
        img, cls = [], []
        for i, ls in enumerate(labels):
            for c in ls:
                c = int(c)
                if not 0 <= c < num_classes:
                    raise ValueError("cim_amd.prm: image %d names class %d, outside 0..%d" % (i, c, num_classes - 1))
                img.append(i)
                cls.append(c)
        self.m = len(img)
        if self.m < 1:
            raise ValueError("cim_amd.prm: no (image, class) pair: every image has an empty class list")
        hs, ws = [int(s[0]) for s in sizes], [int(s[1]) for s in sizes]
        self.desc_host = np.ascontiguousarray(np.array(img + cls + hs + ws, dtype=np.int32))
        # (pinned + non_blocking: a pageable copy would make the host wait for everything already on the stream)
        self.desc_pinned = torch.from_numpy(self.desc_host).pin_memory()
        self.desc_dev = self.desc_pinned.to(device, non_blocking=True)
        b, m = self.b, self.m
        # one int32 buffer, one read: image_out [B,2] | points [B,P,5] | scores [B,P] (f32 bits) | pair_counts [M,3] | median [M]
        self.o_points, self.o_scores = 2 * b, 2 * b + 5 * MAX_PEAKS * b
        self.o_counts = self.o_scores + MAX_PEAKS * b
        self.o_median = self.o_counts + 3 * m
        self.out = torch.zeros(self.o_median + m, dtype=torch.int32, device=device)
        self.ws = None

    def workspace(self, hw, device):
        nbytes = _lib.call("cim_prm_ws_bytes", self.m, hw)
        if nbytes < 0:
            raise ValueError(_lib.load().cim_last_error().decode())
        self.ws = torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device=device)
        return self.ws

    def out_ptrs(self):
        p = self.out.data_ptr()
        return (p + 4 * self.o_median, p + 4 * self.o_counts, p + 4 * self.o_points, p + 4 * self.o_scores, p)

    def read(self, what):
        """The one device-to-host read of the call -> per image (rows, cols, classes, scores) + the details."""
        host = self.out.cpu().numpy()
        b, m = self.b, self.m
        head = host[:2 * b].reshape(b, 2)
        points = host[self.o_points:self.o_scores].reshape(b, MAX_PEAKS, 5)
        scores = host[self.o_scores:self.o_counts].view(np.float32).reshape(b, MAX_PEAKS)
        self.pair_counts = host[self.o_counts:self.o_median].reshape(m, 3)
        self.median = host[self.o_median:].view(np.float32)
        self.ys_xs = []
        res = []
        for i in range(b):
            n, status = int(head[i, 0]), int(head[i, 1])
            if status & STATUS_NAN:
                raise ValueError("%s: image %d has a NaN in a processed class response map (the reference's argmax of an empty "
                                 "peak list raises there)" % (what, i))
            if status & STATUS_NO_PEAK:
                raise ValueError("%s: image %d has a processed class response map without any peak (every value -inf)" % (what, i))
            if status & STATUS_TOO_MANY:
                raise ValueError("%s: image %d has %d valid peaks, cim_prop_assign takes at most %d" % (what, i, n, MAX_PEAKS))
            p = points[i, :n]
            res.append((p[:, 0].astype(np.int64), p[:, 1].astype(np.int64), p[:, 2].astype(np.int64), scores[i, :n].copy()))
            self.ys_xs.append((p[:, 3].astype(np.int64), p[:, 4].astype(np.int64)))
        return res


def _sizes(image_sizes, b, default):
    if image_sizes is None:
        return [default] * b
    if len(image_sizes) != b:
        raise ValueError("cim_amd.prm: %d image sizes for %d images" % (len(image_sizes), b))
    return [(int(s[0]), int(s[1])) for s in image_sizes]


def peaks_from_maps(up, labels, image_sizes=None, peak_threshold=10, num_classes=None, details=False):
    """The peak entry on GIVEN up-sampled maps: up [M, H, W] fp32 on the device, one map per (image, class) pair of `labels`
    (a list of B class lists), in that order.  Returns what `peaks` returns."""
    if not torch.is_tensor(up) or not up.is_cuda:
        raise _lib.CimHipError("cim_amd.prm.peaks_from_maps: CUDA/HIP tensor expected (no CPU fallback)")
    if up.dim() != 3 or up.dtype != torch.float32:
        raise ValueError("cim_amd.prm.peaks_from_maps: up must be [M, H, W] float32, got %s %s" % (tuple(up.shape), up.dtype))
    m, h, w = (int(s) for s in up.shape)
    c = int(num_classes) if num_classes is not None else 1 + max([int(x) for ls in labels for x in ls] + [0])
    run = _Launch(labels, _sizes(image_sizes, len(labels), (h, w)), c, up.device)
    if run.m != m:
        raise ValueError("cim_amd.prm.peaks_from_maps: %d maps for %d (image, class) pairs" % (m, run.m))
    up = up.contiguous()
    ws = run.workspace(0, up.device)
    _lib.call("cim_prm_peaks", up.data_ptr(), m, h, w, run.b, c, run.desc_host.ctypes.data_as(ctypes.c_void_p), run.desc_dev.data_ptr(),
              float(peak_threshold), *run.out_ptrs(), ws.data_ptr(), _lib.stream_ptr())
    res = run.read("cim_amd.prm.peaks_from_maps")
    return (res, run) if details else res


def upsample(crm, labels, factor, bias=None):
    """The up-sampling launch alone: crm [B, C, h, w] fp32 (+ bias [C]) -> up [M, factor h, factor w] for the pairs of `labels`."""
    if not torch.is_tensor(crm) or not crm.is_cuda:
        raise _lib.CimHipError("cim_amd.prm.upsample: CUDA/HIP tensor expected (no CPU fallback)")
    crm = crm.contiguous()
    b, c, h, w = (int(s) for s in crm.shape)
    if len(labels) != b:
        raise ValueError("cim_amd.prm.upsample: %d class lists for %d images" % (len(labels), b))
    run = _Launch(labels, [(1, 1)] * b, c, crm.device)
    f = int(factor)
    if f >= 1 and h * f * w * f > MAX_HW:
        raise ValueError("cim_amd.prm.upsample: %d x %d up-sampled pixels, at most %d" % (h * f, w * f, MAX_HW))
    up = torch.empty((run.m, h * max(f, 0), w * max(f, 0)), dtype=torch.float32, device=crm.device)
    _lib.call("cim_prm_upsample", crm.data_ptr(), _lib.ptr(bias), b, c, h, w, f, run.m, run.desc_host.ctypes.data_as(ctypes.c_void_p),
              run.desc_dev.data_ptr(), up.data_ptr(), _lib.stream_ptr())
    return up


def peaks_from_crm(crm, labels, factor=8, image_sizes=None, peak_threshold=10, details=False):
    """crm [B, C, h, w] fp32 on the device -> what `peaks` returns: the three launches of csrc/prm.hip and the one read."""
    if not torch.is_tensor(crm) or not crm.is_cuda:
        raise _lib.CimHipError("cim_amd.prm.peaks: CUDA/HIP tensor expected (no CPU fallback)")
    if crm.dim() != 4 or crm.dtype != torch.float32:
        raise ValueError("cim_amd.prm.peaks: class response maps must be [B, C, h, w] float32, got %s %s" % (tuple(crm.shape), crm.dtype))
    crm = crm.contiguous()
    b, c, h, w = (int(s) for s in crm.shape)
    if len(labels) != b:
        raise ValueError("cim_amd.prm.peaks: %d class lists for %d images" % (len(labels), b))
    f = int(factor)
    if f < 1:
        raise ValueError("cim_amd.prm.peaks: factor = %d" % f)
    hw = h * f * w * f
    if hw > MAX_HW:
        raise ValueError("cim_amd.prm.peaks: %d x %d up-sampled pixels, at most %d" % (h * f, w * f, MAX_HW))
    run = _Launch(labels, _sizes(image_sizes, b, (h * f, w * f)), c, crm.device)
    ws = run.workspace(hw, crm.device)
    _lib.call("cim_prm_points", crm.data_ptr(), None, b, c, h, w, f, run.m, run.desc_host.ctypes.data_as(ctypes.c_void_p),
              run.desc_dev.data_ptr(), float(peak_threshold), *run.out_ptrs(), ws.data_ptr(), _lib.stream_ptr())
    res = run.read("cim_amd.prm.peaks")
    return (res, run) if details else res


def peaks(model, images, labels, peak_threshold=10, image_sizes=None, details=False):
    """images [B, 3, S, S'] normalised fp32 on the device (`network_input`), labels = B lists of image-level classes (the order
    of the reference's `lables`: ascending, torch.unique) -> per image (rows, cols, classes, scores): host arrays in the order
    `proposal_prep.assign_clusters` consumes them (ascending peak score, AGPL_label_assign.py:148-161).  rows / cols are pixels
    of an image of `image_sizes[i]` = (height, width) (default: the up-sampled grid itself, i.e. the reference's y, x).
    One forward pass of batch B, three launches, no host synchronisation, then ONE device-to-host read for the batch.
    Raises ValueError naming the image for more than 256 valid peaks or a NaN in a processed map."""
    if not isinstance(model, PeakResponseMapping):
        raise TypeError("cim_amd.prm.peaks: a cim_amd.prm.PeakResponseMapping is expected")
    if not torch.is_tensor(images) or not images.is_cuda:
        raise _lib.CimHipError("cim_amd.prm.peaks: CUDA/HIP tensor expected (no CPU fallback)")
    crm = model(images)
    return peaks_from_crm(crm, labels, int(model.sub_pixel_locating_factor), image_sizes, peak_threshold, details)


from .prm_backprop import backprop, peak_response_maps  # noqa: E402,F401  (the peak back-propagation: prm_backprop.py)
