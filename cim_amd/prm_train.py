"""PRM classification training on the device: peak stimulation and the multilabel soft margin loss.

Replaces what lib/prm/prm_model.py composes for training - F.upsample(align_corners=True), the median filter,
lib/prm/prm_modules.py `PeakStimulation` (forward and backward) and F.multilabel_soft_margin_loss - by the launches of
csrc/prm_train.hip: one workgroup per (image, class) map up-samples it into LDS, finds its peaks and averages them; the backward
gathers the peaks' tap weights into a gradient of the class response map's own size.  The body runs on the kernels the
detector's body trains on.

    model = prm.PeakResponseMapping(prm.fc_resnet50(num_classes=20))     # the same object `cim_amd.prm.peaks` takes
    prm_train.freeze(model)                                              # stem and layer1, as the detector's body
    # prm_train.unfreeze(model)                                          # or: every layer trains, the reference's state
    loss = prm_train.loss(model, images, target)                         # images [B,3,S,S'] (prm.network_input*), target [B,C]
    loss.backward()

`cim_amd.prm.PeakResponseMapping` itself stays the inference object (its train() raises, its forward runs under no_grad): a
checkpoint moves between the two entries unchanged.  By default BatchNorm statistics stay frozen; `batch_stats=True` (on
`class_response_maps`, `aggregate` and `loss`) runs every BatchNorm of a stage that trains on the statistics of the batch and
updates its running buffers, as the reference's train() does (`ops.bn_act_train`): with `unfreeze` +
`batch_stats=True` the step is lib/prm/prm_model.py's, nothing left out.
A stem that trains takes `ops.conv7x7_bn_act_train` (the 7 x 7 weight gradient of csrc/conv7x7_dw.hip).
Takes DEVICE tensors; a CPU tensor is an error (no CPU fallback)."""
import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from . import prm as _prm
from .modeling.resnet50 import Bottleneck
from .ops import bn_act_train, conv1x1_bn_act, conv3x3_bn_act, conv7x7_bn_act, conv7x7_bn_act_train, max_pool2d
from .ops.conv3x3 import Conv7x7Function

STIM_MAX_HW = _lib.CONSTANTS["CIM_PRM_STIM_MAX_HW"]
STATUS_NAN, STATUS_NO_PEAK = _prm.STATUS_NAN, _prm.STATUS_NO_PEAK


def _device_f32(t, who, what, dims):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.CimHipError("cim_amd.prm_train.%s: CUDA/HIP tensor expected (no CPU fallback)" % who)
    if t.dim() != dims or t.dtype != torch.float32:
        raise ValueError("cim_amd.prm_train.%s: %s must be %d-dimensional float32, got %s %s" % (who, what, dims, tuple(t.shape), t.dtype))


class StimulationState(object):
    """What one peak_stimulation call left on the device: bitmap [B,C,ceil(H W / 32)] uint32 words (int32 storage), count,
    status [B,C] int32, median [B,C] f32.  Nothing here is read by the training step."""

    def __init__(self, shape, factor, device):
        b, c, h, w = shape
        self.shape, self.factor = (b, c, h, w), factor
        self.up_shape = (h * factor, w * factor)
        self.words = (self.up_shape[0] * self.up_shape[1] + 31) // 32
        self.bitmap = torch.empty((b, c, self.words), dtype=torch.int32, device=device)
        self.count = torch.empty((b, c), dtype=torch.int32, device=device)
        self.status = torch.empty((b, c), dtype=torch.int32, device=device)
        self.median = torch.empty((b, c), dtype=torch.float32, device=device)

    def peak_map(self):
        """The peak map [B,C,H,W] bool on the device."""
        H, W = self.up_shape
        bits = (self.bitmap[..., None] >> torch.arange(32, device=self.bitmap.device, dtype=torch.int32)) & 1
        return bits.reshape(self.shape[0], self.shape[1], -1)[..., :H * W].reshape(self.shape[:2] + (H, W)).bool()

    def peak_list(self):
        """The reference's torch.nonzero(peak_map): [P,4] int64 = (image, class, y, x), row-major.  Reads the device."""
        return torch.nonzero(self.peak_map())

    def check(self):
        """Raises ValueError naming the first (image, class) whose map had a NaN or no peak.  Reads the device."""
        status = self.status.cpu().numpy()
        for i, j in zip(*np.nonzero(status)):
            why = "a NaN in it" if status[i, j] & STATUS_NAN else "no peak (every value -inf)"
            raise ValueError("cim_amd.prm_train: the class response map of image %d, class %d has %s: its aggregation is NaN" % (i, j, why))
        return self


class PeakStimulationFunction(Function):
    @staticmethod
    def forward(ctx, crm, bias, factor, state):
        b, c, h, w = state.shape
        agg = torch.empty((b, c), dtype=torch.float32, device=crm.device)
        _lib.call("cim_prmt_stim_forward", crm.data_ptr(), _lib.ptr(bias), b, c, h, w, factor, agg.data_ptr(), state.count.data_ptr(),
                  state.median.data_ptr(), state.status.data_ptr(), state.bitmap.data_ptr(), _lib.stream_ptr())
        ctx.state, ctx.has_bias = state, bias is not None
        return agg

    @staticmethod
    def backward(ctx, grad_agg):
        state = ctx.state
        b, c, h, w = state.shape
        grad_agg = grad_agg.contiguous()
        dcrm = torch.empty(state.shape, dtype=torch.float32, device=grad_agg.device)
        dbias = torch.empty(c, dtype=torch.float32, device=grad_agg.device) if ctx.has_bias and ctx.needs_input_grad[1] else None
        _lib.call("cim_prmt_stim_backward", grad_agg.data_ptr(), state.count.data_ptr(), state.bitmap.data_ptr(), b, c, h, w, state.factor,
                  dcrm.data_ptr(), _lib.ptr(dbias), _lib.stream_ptr())
        return dcrm, dbias, None, None


def peak_stimulation(crm, factor=8, bias=None):
    """crm [B,C,h,w] fp32 on the device (+ bias [C], added before the up-sampling) -> (aggregation [B,C], state): the mean of the
    peaks of each map up-sampled by `factor` (bilinear, align_corners=True; median filter, 3 x 3 window).  The aggregation carries
    the gradient to crm and bias; one launch forward, one backward (two with a bias)."""
    _device_f32(crm, "peak_stimulation", "crm", 4)
    if bias is not None:
        _device_f32(bias, "peak_stimulation", "bias", 1)
        if bias.shape[0] != crm.shape[1]:
            raise ValueError("cim_amd.prm_train.peak_stimulation: %d bias values for %d classes" % (bias.shape[0], crm.shape[1]))
        bias = bias.contiguous()
    f = int(factor)
    b, c, h, w = (int(s) for s in crm.shape)
    if f < 1 or min(b, c, h, w) < 1:
        raise ValueError("cim_amd.prm_train.peak_stimulation: factor = %d on maps of shape %s" % (f, (b, c, h, w)))
    if h * f * w * f > STIM_MAX_HW:
        raise ValueError("cim_amd.prm_train.peak_stimulation: %d x %d up-sampled pixels, at most %d" % (h * f, w * f, STIM_MAX_HW))
    state = StimulationState((b, c, h, w), f, crm.device)
    return PeakStimulationFunction.apply(crm.contiguous(), bias, f, state), state


class MsmLossFunction(Function):
    @staticmethod
    def forward(ctx, agg, target):
        b, c = agg.shape
        loss = torch.empty(1, dtype=torch.float32, device=agg.device)
        dagg = torch.empty_like(agg)
        _lib.call("cim_prmt_msm_loss", agg.data_ptr(), target.data_ptr(), b, c, loss.data_ptr(), dagg.data_ptr(), _lib.stream_ptr())
        ctx.save_for_backward(dagg)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        dagg, = ctx.saved_tensors
        return dagg * grad, None


def multilabel_soft_margin_loss(aggregation, target):
    """torch's F.multilabel_soft_margin_loss(aggregation, target) as ONE single-workgroup launch that also writes the gradient
    (sigmoid(x) - t) / (B C): aggregation, target [B,C] fp32 on the device -> a scalar with a gradient to the aggregation."""
    _device_f32(aggregation, "multilabel_soft_margin_loss", "aggregation", 2)
    _device_f32(target, "multilabel_soft_margin_loss", "target", 2)
    if aggregation.shape != target.shape or aggregation.numel() < 1:
        raise ValueError("cim_amd.prm_train.multilabel_soft_margin_loss: aggregation %s against target %s" % (tuple(aggregation.shape), tuple(target.shape)))
    return MsmLossFunction.apply(aggregation.contiguous(), target.contiguous())


def freeze(model, at=2):
    """requires_grad = False on the stem and on layer1 .. layer{at-1} of the PeakResponseMapping `model` (at in 2..5; 2 = the
    stage up to which the detector's body freezes, ResNet.FREEZE_AT).  It only ever freezes: parameters behind `at` keep their
    state.  `unfreeze` is the way back to a network whose stem and layer1 train."""
    if at not in (2, 3, 4, 5):
        raise ValueError("cim_amd.prm_train.freeze: at = %r, one of 2, 3, 4, 5 is needed" % (at,))
    f = _features(model)
    for i in range(0, 3 + at):               # features: conv1, bn1, relu, maxpool, layer1 (index 4) ..
        for p in f[i].parameters():
            p.requires_grad = False
    return model


def unfreeze(model):
    """requires_grad = True on EVERY parameter of the PeakResponseMapping `model`: the reference's training state
    (lib/prm/prm_model.py trains every layer).  BatchNorm statistics stay frozen unless the step asks for `batch_stats=True`;
    with both, the stated difference from lib/prm/prm_model.py's train() is gone."""
    _features(model)
    for p in model.parameters():
        p.requires_grad = True
    return model


def _features(model):
    if not isinstance(model, _prm.PeakResponseMapping) or not isinstance(model[0], _prm.FC_ResNet):
        raise TypeError("cim_amd.prm_train: a cim_amd.prm.PeakResponseMapping over a cim_amd.prm.FC_ResNet is expected")
    return model[0].features


_IDENTITY_BN = {}      # (device, classes) -> a BatchNorm2d that is y = x exactly (gamma 1, beta 0, mean 0, var 1, eps 0), not trained


def _identity_bn(device, c):
    key = (device, c)
    if key not in _IDENTITY_BN:
        bn = torch.nn.BatchNorm2d(c, eps=0.0).to(device).eval()
        for p in bn.parameters():
            p.requires_grad = False
        _IDENTITY_BN[key] = bn
    return _IDENTITY_BN[key]


def _bare(wrapper, x, conv):
    """conv(x) alone on the fused launch: the identity BatchNorm, no ReLU (as the classifier below)."""
    return wrapper(x, conv, _identity_bn(x.device, conv.out_channels), relu=False)


def _stem_batch_stats(images, conv, bn):
    """relu(bn(conv(images))) with batch statistics: the bare 7 x 7 launch (its weight gradient: csrc/conv7x7_dw.hip), then
    `bn_act_train`."""
    if not (conv.kernel_size == (7, 7) and conv.padding == (3, 3) and conv.stride in ((1, 1), (2, 2)) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and 1 <= conv.in_channels <= 4 and 1 <= conv.out_channels <= 256
            and images.shape[3] <= 4096 and images.shape[2] * images.shape[3] < (1 << 20)):
        raise ValueError("cim_amd.prm_train: unsupported stem %s on an input of shape %s" % (conv, tuple(images.shape)))
    if torch.is_grad_enabled() and images.requires_grad:
        raise ValueError("cim_amd.prm_train: the images require a gradient: the stem's data gradient is not built")
    args = (images.contiguous(), conv.weight if conv.weight.is_contiguous() else conv.weight.contiguous(), conv.stride[0])
    if torch.is_grad_enabled() and conv.weight.requires_grad:
        z = Conv7x7Function.apply(*args)
    else:
        with torch.no_grad():
            z = Conv7x7Function.apply(*args)
    return bn_act_train(z, bn, relu=True)


def _bottleneck_batch_stats(block, x):
    """modeling/resnet50.py Bottleneck.forward with every BatchNorm on batch statistics: each convolution bare on its fused launch,
    `bn_act_train` behind it with the block's residual and ReLU."""
    out = bn_act_train(_bare(conv1x1_bn_act, x, block.conv1), block.bn1)
    out = bn_act_train(_bare(conv3x3_bn_act, out, block.conv2), block.bn2)
    identity = x
    if block.downsample is not None:
        identity = bn_act_train(_bare(conv1x1_bn_act, x, block.downsample[0]), block.downsample[1], relu=False)
    return bn_act_train(_bare(conv1x1_bn_act, out, block.conv3), block.bn3, residual=identity, relu=True)


def _trains(*modules):
    return any(p.requires_grad for m in modules for p in m.parameters())


def class_response_maps(model, images, batch_stats=False):
    """model[0] under the current grad mode: the stem (one fused launch when frozen, its training form when one of its parameters
    requires a gradient), layer1..layer4 and the 1 x 1 classifier on the fused launches, the classifier WITH autograd - its
    convolution bias folded into the identity BatchNorm's mean (ops/conv1x1.py), its weight and bias gradients from the small-tile
    GEMM path.

    batch_stats=True: a stage of `features` (the stem; layer1 .. layer4) with at least one parameter that requires a gradient runs
    every BatchNorm on the statistics of the batch and updates its running buffers, as lib/prm/prm_model.py's train() does - each
    convolution bare on its fused launch, `ops.bn_act_train` behind it.  A stage with nothing to train (after `freeze`) keeps its
    module call and its running statistics.  After `unfreeze` this is the reference's training forward."""
    f = _features(model)
    if batch_stats and _trains(f[0], f[1]):
        x = max_pool2d(_stem_batch_stats(images, f[0], f[1]), f[3])
    else:
        trains = torch.is_grad_enabled() and any(p.requires_grad for i in range(4) for p in f[i].parameters())
        x = max_pool2d((conv7x7_bn_act_train if trains else conv7x7_bn_act)(images, f[0], f[1], relu=True), f[3])
    for i in range(4, 8):
        if batch_stats and _trains(f[i]):
            for block in f[i]:
                if not isinstance(block, Bottleneck):
                    raise TypeError("cim_amd.prm_train: batch_stats=True walks cim_amd.modeling.resnet50.Bottleneck blocks, got %r" % (type(block),))
                x = _bottleneck_batch_stats(block, x)
        else:
            x = f[i](x)
    conv = model[0].classifier[0]
    return conv1x1_bn_act(x, conv, _identity_bn(x.device, conv.out_channels), relu=False)


def aggregate(model, images, batch_stats=False):
    """images [B,3,S,S'] normalised fp32 on the device -> (aggregation [B,C], state): class_response_maps, then peak_stimulation
    at the model's sub_pixel_locating_factor.  batch_stats: see `class_response_maps`."""
    _device_f32(images, "aggregate", "images", 4)
    return peak_stimulation(class_response_maps(model, images, batch_stats=batch_stats), int(model.sub_pixel_locating_factor))


def loss(model, images, target, batch_stats=False):
    """The PRM classification loss of a batch: `aggregate`, then `multilabel_soft_margin_loss` against target [B,C].  With
    `unfreeze(model)` and batch_stats=True this is the training step of lib/prm/prm_model.py, BatchNorm statistics included."""
    agg, _ = aggregate(model, images, batch_stats=batch_stats)
    return multilabel_soft_margin_loss(agg, target)
