"""Batch-statistics BatchNorm (+ residual) (+ ReLU) on the device (cim_amd/csrc/bn_train.hip).

`bn_act_train(x, bn, residual=None, relu=True)` == F.relu(bn.train()(x) + residual) for an nn.BatchNorm2d with affine=True: the
normalisation uses the statistics of the batch `x`, and `bn.running_mean`, `bn.running_var` and `bn.num_batches_tracked` are
updated as torch does (momentum, or the cumulative average for momentum None; nothing for track_running_stats=False) - under
no_grad too.  It does NOT look at `bn.training`: calling it is the request for batch statistics (`bn_act` is the operator on
running statistics, and it keeps refusing a module in training mode).  What lib/prm/prm_model.py's PeakResponseMapping.train()
runs in every BatchNorm of its network.

Launches: statistics (per-chunk partials, then an ordered finish that also updates the running buffers), the normalisation of
`bn_act` on the batch statistics; backward: sums (partials, ordered finish), then dx / dres.  No atomics: the same bits on every
call.  No host read, no synchronisation.  There is no second path: CPU tensors, non-fp32 data, a non-contiguous or not
4-dimensional input, affine=False and fewer than two values per channel raise ValueError."""
import torch
from torch.autograd import Function

from .. import _lib


class BnActTrainFunction(Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, bn, relu):
        n, c = x.shape[0], x.shape[1]
        hw = x.shape[2] * x.shape[3]
        dev = x.device
        y = torch.empty_like(x)
        mean, var, rstd = torch.empty((3, c), dtype=torch.float32, device=dev).unbind(0)
        ws = torch.empty(_lib.call("cim_bn_train_workspace", n, c, hw) // 4, dtype=torch.float32, device=dev)
        track = bn.track_running_stats and bn.running_mean is not None
        momentum = -1.0 if bn.momentum is None else float(bn.momentum)          # (< 0: torch's momentum None)
        _lib.call("cim_bn_train_fwd", x.data_ptr(), _lib.ptr(res), gamma.data_ptr(), beta.data_ptr(), float(bn.eps), momentum,
                  _lib.ptr(bn.running_mean if track else None), _lib.ptr(bn.running_var if track else None),
                  _lib.ptr(bn.num_batches_tracked if track else None), y.data_ptr(), mean.data_ptr(), var.data_ptr(),
                  rstd.data_ptr(), n, c, hw, int(relu), ws.data_ptr(), _lib.stream_ptr())
        ctx.save_for_backward(x, y if relu else None, gamma, mean, rstd)
        ctx.cfg = (n, c, hw, bool(relu), res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, rstd = ctx.saved_tensors
        n, c, hw, relu, has_res = ctx.cfg
        dy = dy.contiguous()
        dev = x.device
        need_res = has_res and ctx.needs_input_grad[1]
        need_affine = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dres = torch.empty_like(x) if need_res else None
        dgamma, dbeta = torch.empty((2, c), dtype=torch.float32, device=dev).unbind(0) if need_affine else (None, None)
        ws = torch.empty(_lib.call("cim_bn_train_workspace", n, c, hw) // 4, dtype=torch.float32, device=dev)
        _lib.call("cim_bn_train_bwd", dy.data_ptr(), _lib.ptr(y), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                  _lib.ptr(dx), _lib.ptr(dres), _lib.ptr(dgamma), _lib.ptr(dbeta), n, c, hw, int(relu), ws.data_ptr(),
                  _lib.stream_ptr())
        return dx, dres, (dgamma if ctx.needs_input_grad[2] else None), (dbeta if ctx.needs_input_grad[3] else None), None, None


def bn_act_train(x, bn, residual=None, relu=True):
    """relu?(bn(x) + residual) with the statistics of the batch `x` for a BatchNorm2d module `bn` (whatever `bn.training` says);
    updates the module's running buffers."""
    who = "cim_amd.ops.bn_act_train: "
    if not isinstance(bn, torch.nn.BatchNorm2d) or not bn.affine or bn.weight is None:
        raise ValueError(who + "an nn.BatchNorm2d with affine=True is expected, got %r" % (bn,))
    if not torch.is_tensor(x):
        raise ValueError(who + "a tensor is expected, got %r" % (type(x),))
    if x.dtype != torch.float32 or bn.weight.dtype != torch.float32:
        raise ValueError(who + "float32 expected, got %s" % (x.dtype,))
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(who + "a contiguous 4-dimensional input is expected, got shape %s, strides %s" % (tuple(x.shape), x.stride()))
    if x.shape[1] != bn.num_features:
        raise ValueError(who + "%d channels for a BatchNorm2d over %d" % (x.shape[1], bn.num_features))
    if x.shape[0] * x.shape[2] * x.shape[3] < 2 or x.shape[1] < 1:
        raise ValueError(who + "Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    if x.numel() > 2 ** 31 - 1:
        raise ValueError(who + "%d elements, at most 2^31 - 1" % x.numel())
    if not (x.is_cuda and bn.weight.is_cuda):
        raise ValueError(who + "CUDA/HIP tensors expected (no CPU path)")
    if residual is not None:
        if not (torch.is_tensor(residual) and residual.is_cuda and residual.dtype == torch.float32 and residual.shape == x.shape):
            raise ValueError(who + "the residual must be a float32 CUDA/HIP tensor of the input's shape %s" % (tuple(x.shape),))
        residual = residual.contiguous()
    return BnActTrainFunction.apply(x, residual, bn.weight, bn.bias, bn, relu)
