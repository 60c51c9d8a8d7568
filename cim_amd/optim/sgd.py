"""Fused multi-tensor SGD (cim_amd/csrc/sgd.hip) behind torch.optim.SGD's interface.

Drop-in for `torch.optim.SGD(params, momentum=cfg.SOLVER.MOMENTUM)` at /root/reference/tools/train.py:308-309: same
param-group keys (lr, momentum, weight_decay, dampening, nesterov), same `state[p]['momentum_buffer']` tensors (so
lib/utils/net.py:47-83 `update_learning_rate` / `_CorrectMomentum` and the checkpoint code keep working), same update
rule - but ONE kernel launch per step for all parameters instead of one multi-tensor launch per ~20 tensors.
Only what the reference uses is supported on the HIP path: fp32 CUDA/HIP parameters, dampening 0, no Nesterov,
dense gradients, one momentum value; anything else raises (there is no silent fallback).

Host cost per step: autograd hands out new gradient tensors every step and the row / column |max| arrays are fresh
storage every step, so the 64-byte record of every tensor is rebuilt and copied (one pass over the parameters, one
10 KB H2D copy; the copy is skipped only when the table happens to be byte-identical to the previous step's); the chunk
table only depends on the tensor sizes and is built once.  Matrix mode and 16-byte accesses need 16-byte aligned
parameter, gradient and history pointers: nn.DataParallel's flat gradient buffer aligns its views accordingly.

Weights of >= 2^20 elements are updated in the kernel's matrix mode, which also emits max |w_new| per row and per column:
exactly what the f16x2 contraction engine needs as operand scales of `nn.Linear` / conv weights.  They are registered with
`cim_amd.ops.gemm.register_weight_scales` under the weight's new version counter, so the next forward skips its pass over
the weight (0.29 ms per step at cfg2, mostly the 822 MB fc1 weight); any other in-place change of the weight bumps the
version and the ops fall back to their own pass.
"""
import numpy as np
import torch

from .. import _lib
from .fused import CHUNK, MATRIX_MIN, TILE_COLS, TILE_ROWS, TRAIL_MIN, FusedOptimizer, _matrix_shape, _Pass  # noqa: F401  (this module's public names)

_TENSOR = np.dtype(_lib.STRUCTS["cim_sgd_tensor"])


class SGD(FusedOptimizer):
    """The machinery around the launch - tables, fast path, step_early, overlap_update - is FusedOptimizer's (fused.py)."""
    _NAME = "cim_amd.optim.SGD"
    _RECORD = _TENSOR
    _STATE = (("buf", "momentum_buffer"),)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if dampening != 0.0 or nesterov:
            raise NotImplementedError("cim_amd.optim.SGD: dampening / Nesterov are not used by the reference and not provided")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)

    def _rule(self):
        momentum = None
        for group in self.param_groups:
            if group.get("dampening", 0.0) != 0.0 or group.get("nesterov", False):
                raise NotImplementedError("cim_amd.optim.SGD: dampening / Nesterov")
            if momentum is None:
                momentum = float(group["momentum"])
            elif float(group["momentum"]) != momentum:
                raise NotImplementedError("cim_amd.optim.SGD: one momentum value for all groups")
        return momentum

    def _new_state(self, p, st):
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _fill(self, tab, c):
        lrs = np.array([float(g["lr"]) for g in self.param_groups], dtype=np.float32)
        wds = np.array([float(g["weight_decay"]) for g in self.param_groups], dtype=np.float32)
        tab["lr"], tab["wd"] = lrs[c["group_of"]], wds[c["group_of"]]

    def _launch(self, c, ps, workgroups):
        _lib.call("cim_sgd_multi", c["table"].data_ptr(), ps.chunks.data_ptr(), ps.n_chunks, c["rule"], workgroups, _lib.stream_ptr())
