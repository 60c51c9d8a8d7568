"""Gradient clipping by the global L2 norm on the device (cim_amd/csrc/grad_clip.hip).

`GradClipper(parameters)` is what `cim_amd.utils.net.clip_gradient` (lib/utils/net.py:15) runs on GPU gradients: one streaming
launch for the sum of squares of ALL gradients (fp64, one slot per 16384-element chunk), one single-workgroup launch that
turns the slots into the norm and the clip coefficient, one launch that scales the gradients in place - and returns at once
when the coefficient is 1.  Norm and coefficient stay on the device: no `.item()`, the host does not wait for the backward
pass.  `norm()` is the first two launches alone (the number to log when a run diverges).

The tables are the fused optimizers': the chunk table (fused.CHUNK, cim_sgd_chunk) only depends on the gradient sizes and is
built once; the per-step table - address and element count of every gradient, autograd hands out new tensors every step - is
staged in pinned memory and copied only when its bytes changed.
"""
import numpy as np
import torch

from .. import _lib
from ..ops.gemm import join_side as _join_side
from . import fused

_NAME = "cim_amd.optim.GradClipper"


def chunk_table(sizes):
    """fused.chunk_table for flat tensors of `sizes` elements."""
    return fused.chunk_table([(n, 0, 0) for n in sizes])


class GradClipper:
    def __init__(self, parameters):
        self.params = list(parameters)
        self._layout = None         # (device, gradient sizes) the device tables were built for
        self._t = None

    def _gradients(self):
        grads, dev = [], None
        for p in self.params:
            g = p.grad
            if g is None or not p.requires_grad:
                continue
            if not g.is_cuda:
                raise _lib.CimHipError(_NAME + ": CUDA/HIP gradients required (no CPU fallback)")
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous():
                raise NotImplementedError(_NAME + ": dense contiguous fp32 gradients (they are scaled in place)")
            if dev is None:
                dev = g.device
            elif g.device != dev:
                raise _lib.CimHipError(_NAME + ": gradients on %s and %s: one device per clipper" % (dev, g.device))
            if g.numel():
                grads.append(g)
        return grads, dev

    def _build(self, layout):
        dev, sizes = layout
        chunks = chunk_table(sizes)
        n = len(sizes)
        self._t = dict(
            n_chunks=int(chunks.shape[0]), chunks=torch.from_numpy(chunks.view(np.uint8).reshape(-1).copy()).to(dev),
            tab=np.zeros(2 * n, dtype=np.uint64),       # addresses [n], then element counts [n] (int64 on the device)
            staged=fused.StagedTable(16 * n, dev),
            partial=torch.empty(chunks.shape[0], dtype=torch.float64, device=dev), out=torch.empty(2, dtype=torch.float32, device=dev))
        self._t["tab"][n:] = sizes
        self._layout = layout

    @torch.no_grad()
    def _run(self, max_norm, scale):
        _join_side()            # weight gradients deferred to the side stream (cim_amd/ops/gemm.py; normally joined at the end of backward)
        grads, dev = self._gradients()
        if not grads:
            return None
        layout = (dev, tuple(g.numel() for g in grads))
        if layout != self._layout:
            self._build(layout)
        t, n = self._t, len(grads)
        t["tab"][:n] = [g.data_ptr() for g in grads]
        with torch.cuda.device(dev):
            base, stream = t["staged"].upload(t["tab"]), _lib.stream_ptr()
            args = (base, base + 8 * n, n, t["chunks"].data_ptr(), t["n_chunks"])
            _lib.call("cim_grad_norm_multi", *args, t["partial"].data_ptr(), float(max_norm), t["out"].data_ptr(), 0, stream)
            if scale:
                _lib.call("cim_grad_scale_multi", *args, t["out"].data_ptr(), 0, stream)
                torch.autograd.graph.increment_version(grads)      # written through raw pointers: tell autograd's version counters
        return t["out"]

    def clip(self, max_norm):
        """Scale all gradients in place by max_norm / max(global L2 norm, max_norm).  Returns the device tensor float32[2]
        (norm before clipping, coefficient applied) - the clipper's own buffer, overwritten by the next call - or None when no
        parameter has a gradient."""
        return self._run(max_norm, True)

    def norm(self):
        """The global L2 norm alone: the same tensor with coefficient 1, no gradient touched."""
        return self._run(float("inf"), False)
