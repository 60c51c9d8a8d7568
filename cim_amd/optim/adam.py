"""Fused multi-tensor Adam (cim_amd/csrc/adam.hip) behind torch.optim.Adam's interface.

Drop-in for `torch.optim.Adam(params)` as the reference's driver constructs it under SOLVER.TYPE Adam
(tools/train.py:310-311): torch's param-group keys, `state[p]` = {step, exp_avg, exp_avg_sq} laid out as torch.optim.Adam lays
them out (`step` a CPU float32 scalar tensor, created with the two moments when the parameter's first gradient appears - every
parameter has its own count), so a state_dict() of either optimizer loads into the other - in torch's default layout: a
state dict saved by torch.optim.Adam(fused=True) or capturable=True carries `step` on the device, and the first step() after
loading it here raises NotImplementedError.  ONE kernel launch per step for all
parameters; the bias corrections are host numbers, computed in double precision per tensor as torch does,
    step_size = lr / (1 - beta1^t)      bc2_sqrt = sqrt(1 - beta2^t)
and written into the tensor's 80-byte record.  The update rule and its exact order of operations: csrc/adam.hip.

Only what the reference uses is provided: L2 weight decay, one (betas, eps) for all groups, fp32 CUDA/HIP parameters, dense
gradients; amsgrad, maximize, capturable, differentiable, decoupled weight decay raise (there is no silent fallback), and so
does a step inside a stream capture - a captured step would replay frozen bias corrections.

Everything around the launch - matrix mode and its row / column |max| by-product for the contraction ops, the cached fast
path, step_early, overlap_update - is FusedOptimizer's (fused.py) and behaves as in cim_amd.optim.SGD.
"""
import numpy as np
import torch

from .. import _lib
from .fused import FusedOptimizer

_TENSOR = np.dtype(_lib.STRUCTS["cim_adam_tensor"])
_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


class Adam(FusedOptimizer):
    _NAME = "cim_amd.optim.Adam"
    _RECORD = _TENSOR
    _STATE = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if torch.is_tensor(lr) or any(torch.is_tensor(b) for b in betas):
            raise NotImplementedError("cim_amd.optim.Adam: lr and betas as Python numbers")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("cim_amd.optim.Adam: lr, eps, weight_decay >= 0 and betas in [0, 1)")
        # (foreach / fused choose between torch's own implementations: kept as keys so that state dicts travel, never read)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self._rule()

    def _rule(self):
        rule = None
        for group in self.param_groups:
            for key in _REFUSED:
                if group.get(key, False):
                    raise NotImplementedError("cim_amd.optim.Adam: %s is not used by the reference and not provided" % key)
            mine = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            if rule is None:
                rule = mine
            elif mine != rule:
                raise NotImplementedError("cim_amd.optim.Adam: one (betas, eps) for all groups")
        return rule

    def _new_state(self, p, st):
        if "step" not in st:            # torch.optim.Adam's own layout and order of keys
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        if st["step"].is_cuda or any(st[k].dtype != torch.float32 or not st[k].is_contiguous() for k in ("exp_avg", "exp_avg_sq")):
            raise NotImplementedError("cim_amd.optim.Adam: a CPU step count and dense contiguous fp32 moments")

    def _fill(self, tab, c):
        """The two bias-correction numbers of every tensor of the launch for the step it is about to take (double, then fp32).
        The counts themselves advance in _launch, once the launch is enqueued: a step that raises is not counted."""
        beta1, beta2, _ = c["rule"]
        c["steps"] = steps = [self.state[p]["step"] for p, _, _ in c["recs"]]
        t = np.array([s.item() for s in steps], dtype=np.float64) + 1.0
        lrs = np.array([float(g["lr"]) for g in self.param_groups], dtype=np.float64)
        wds = np.array([float(g["weight_decay"]) for g in self.param_groups], dtype=np.float32)
        tab["step_size"] = lrs[c["group_of"]] / (1.0 - beta1 ** t)
        tab["bc2_sqrt"] = np.sqrt(1.0 - beta2 ** t)
        tab["wd"] = wds[c["group_of"]]

    def _launch(self, c, ps, workgroups):
        beta1, beta2, eps = c["rule"]
        _lib.call("cim_adam_multi", c["table"].data_ptr(), ps.chunks.data_ptr(), ps.n_chunks, beta1, beta2, eps, workgroups,
                  _lib.stream_ptr())
        torch._foreach_add_(c["steps"], 1)

    def _before_launches(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.CimHipError("cim_amd.optim.Adam: step() inside a stream capture - the bias corrections are host numbers, "
                                   "a replayed step would reuse this step's")
