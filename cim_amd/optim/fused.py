"""What the fused multi-tensor optimizers (sgd.py, adam.py) share: everything around the ONE launch per step that does not
depend on the update rule.

A subclass names its rule - the record layout of a tensor on the device (`_RECORD`), which fields of it are state tensors of
`optimizer.state[p]` (`_STATE`), how the shared hyper-parameters are validated (`_rule`), how missing state is created
(`_new_state`), which record fields change per step (`_fill`) and the launch itself (`_launch`) - and inherits:

the chunk table (16384-element flat chunks, 64 x 1024 matrix tiles) built once per set of tensor sizes; the cached fast path
that only refreshes gradient pointers and per-step fields, with the pointer-identity checks that catch `load_state_dict()` and
`p.data = ...`; the 16-byte alignment rule for matrix mode; fresh row / column |max| arrays per step and their registration
with `cim_amd.ops.gemm.register_weight_scales`; autograd's version counters; `step_early` (nn.DataParallel.attach_optimizer),
`overlap_update` / `trail_workgroups` (the big weights' update on the package's side stream under the next forward) and the
waits of `wait_update`, `state_dict` and `zero_grad(set_to_none=False)`.
"""
import numpy as np
import torch

from .. import _lib
from ..ops.gemm import join_side as _join_side

CHUNK = 16384          # elements per workgroup
_CHUNK = np.dtype(_lib.STRUCTS["cim_sgd_chunk"])
MATRIX_MIN = 1 << 20   # weights of at least this many elements are updated in matrix mode (row / column |max| by-product)
TRAIL_MIN = 1 << 24    # overlap_update: weights of at least this many elements are updated on the side stream (at cfg2: fc1 205 M,
                       # the MaskFuse convolution 18.9 M, fc2 16.8 M elements = 96 % of the update's 5.1 GB of traffic)
TILE_ROWS, TILE_COLS = 64, 1024


def _matrix_shape(p):
    """(rows, cols) when the parameter qualifies for the kernel's matrix mode, else None."""
    if p.dim() < 2 or p.numel() < MATRIX_MIN:
        return None
    rows = p.shape[0]
    cols = p.numel() // rows
    return (rows, cols) if cols % 4 == 0 else None


def chunk_table(layout):
    """The chunk table (cim_sgd_chunk records) of tensors with `layout` = (numel, rows, cols) each, rows = cols = 0 for a flat
    tensor: CHUNK elements per flat chunk, the last one of a tensor clamped to its end (the kernels take min(n, elements left)
    themselves, so clamped and unclamped n are the same update); 64 x 1024 tiles of a matrix-mode tensor, offset = first row,
    n = first column."""
    parts = []
    for ti, (n, rows, cols) in enumerate(layout):
        if cols > 0:
            r0, c0 = np.meshgrid(np.arange(0, rows, TILE_ROWS), np.arange(0, cols, TILE_COLS), indexing="ij")
            tab = np.empty(r0.size, dtype=_CHUNK)
            tab["offset"], tab["n"] = r0.reshape(-1), c0.reshape(-1)
        else:
            tab = np.empty((n + CHUNK - 1) // CHUNK, dtype=_CHUNK)
            tab["offset"] = np.arange(len(tab), dtype=np.int64) * CHUNK
            tab["n"] = np.minimum(CHUNK, n - tab["offset"])
        tab["tensor"] = ti
        parts.append(tab)
    return np.concatenate(parts) if parts else np.empty(0, dtype=_CHUNK)


class StagedTable:
    """A per-step host table on the device: staged in pinned memory and copied (on the current stream) only when its bytes
    differ from the previous upload's.  upload() returns the device address."""

    def __init__(self, nbytes, dev):
        self.pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._host = self.pinned.numpy()                 # the pinned buffer as the host sees it
        self._sig = self._copied = None

    def upload(self, tab):
        sig = tab.tobytes()
        if sig != self._sig:
            if self._copied is not None:
                self._copied.synchronize()               # the previous H2D copy out of the staging buffer (long done in practice)
            self._host[:] = np.frombuffer(sig, dtype=np.uint8)
            self.table.copy_(self.pinned, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            self._sig = sig
        return self.table.data_ptr()


class _Pass:
    """Device tables and cached per-parameter records of ONE fused launch over a fixed subset of the parameters."""

    def __init__(self):
        self.layout = None          # tuple of (numel, rows, cols) the chunk table on the device was built for
        self.chunks = None          # device chunk table
        self.n_chunks = 0
        self.cache = None           # records that do not change from step to step (see FusedOptimizer._scan)


class FusedOptimizer(torch.optim.Optimizer):
    _NAME = None        # "cim_amd.optim.<class>" in messages
    _RECORD = None      # numpy dtype of one tensor's device record: p, g, n, rows, cols, row_amax, col_amax + the rule's own fields
    _STATE = ()         # ((record field, key in optimizer.state[p]), ...): the rule's state tensors, updated in place by the launch

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        # Opt-in (round 6; `optimizer.overlap_update = True`, bench.py sets it): the update of the BIG weights (>= TRAIL_MIN elements)
        # leaves the caller's stream - step() enqueues it on the package's side stream, ordered behind everything the caller's stream
        # has done, and returns without making the caller's stream wait.  The next forward's backbone (~1.9 ms of small latency-bound
        # launches that leave HBM idle) then runs BESIDE the 0.8 ms HBM-bound update instead of behind it; the weights' pair images
        # (all the forward and backward ever read of these weights) are built on the same side stream behind the update, and the
        # caller's stream waits for them where MaskFuse starts - as before.  What the caller must know: between step() and the next
        # forward's box head these weights (and their state tensors: momentum buffers, Adam's two moments) are NOT ordered on the
        # caller's stream; state_dict() of the model and of this optimizer wait by themselves, any other direct read needs
        # `optimizer.wait_update()` first.
        self.overlap_update = False
        self.trail_workgroups = 256      # workgroups of the side-stream launch (one slot per CU; 0 / 256 / 512 / 1024 / 2048: 13.90 / 13.70 / 13.79 / 13.84 / 13.85 ms per step)
        self._passes = {}           # "all" | "early" | "rest" | "trail" -> _Pass
        self._early = None          # (frozenset of parameter ids updated early in this optimizer step, stream, event)
        self._check_every_step = True    # re-count the parameters with gradients every step (a parameter that starts to
                                         # receive gradients must not be skipped silently; ~20 us)

    # ------------------------------------------------------------------ the rule (subclass)
    def _rule(self):
        """Validate the param groups; return what the launch takes ONCE for all tensors (compared from step to step)."""
        raise NotImplementedError

    def _new_state(self, p, st):
        """Create the entries of `st = self.state[p]` that are missing (first gradient of `p`)."""
        raise NotImplementedError

    def _fill(self, tab, c):
        """Write the record fields that change from step to step (learning rates, ...) into `tab`."""
        raise NotImplementedError

    def _launch(self, c, ps, workgroups):
        raise NotImplementedError

    # ------------------------------------------------------------------ tables
    def _scan(self, ps, select):
        """Slow path (first step, or when the set of parameters with gradients changed): validate every selected tensor and
        cache what does not change from step to step - parameter and state pointers, sizes, matrix shapes, the device
        chunk table.  Returns False when no selected parameter has a gradient."""
        rule = self._rule()
        recs, dev = [], None
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None or not select(p):
                    continue
                if not p.is_cuda:
                    raise _lib.CimHipError(self._NAME + ": CUDA/HIP parameters required (no CPU fallback)")
                if p.dtype != torch.float32 or g.dtype != torch.float32 or g.is_sparse or not p.is_contiguous():
                    raise NotImplementedError(self._NAME + ": dense contiguous fp32 parameters and gradients")
                st = self.state[p]
                self._new_state(p, st)
                dev = p.device
                recs.append((p, tuple(st[key] for _, key in self._STATE), gi))
        if not recs:
            ps.cache = None
            return False
        n = len(recs)
        tab = np.zeros(n, dtype=self._RECORD)
        tab["p"] = [p.data_ptr() for p, _, _ in recs]
        for k, (field, _) in enumerate(self._STATE):
            tab[field] = [s[k].data_ptr() for _, s, _ in recs]
        tab["n"] = [p.numel() for p, _, _ in recs]
        amax_off, off = [], 0
        for i, (p, state, _) in enumerate(recs):
            ptrs = p.data_ptr() | p.grad.data_ptr()
            for s in state:
                ptrs |= s.data_ptr()
            ms = _matrix_shape(p) if (ptrs & 15) == 0 else None
            if ms:
                tab["rows"][i], tab["cols"][i] = ms
                amax_off.append((i, off, ms[0], ms[1]))
                off += ms[0] + ms[1]
        layout = tuple((int(tab["n"][i]), int(tab["rows"][i]), int(tab["cols"][i])) for i in range(n))
        if layout != ps.layout or ps.chunks is None or ps.chunks.device != dev:
            chunks = chunk_table(layout)
            ps.chunks, ps.n_chunks, ps.layout = torch.from_numpy(chunks.view(np.uint8).reshape(-1).copy()).to(dev), len(chunks), layout
        touched = []
        for p, state, _ in recs:
            touched += [p, *state]
        staged = StagedTable(tab.nbytes, dev)
        ps.cache = dict(recs=recs, tab=tab, amax_off=amax_off, n_amax=off, rule=rule, dev=dev, touched=touched,
                        staged=staged, table=staged.table,       # `table`: the records on the device, what _launch passes
                        group_of=np.array([gi for _, _, gi in recs]), ids=frozenset(id(p) for p, _, _ in recs))
        return True

    def _pointers_moved(self, c):
        """The cached raw pointers must still be THE tensors: load_state_dict() replaces the state tensors, .to() / .half() /
        set_() the parameter storage (one int compare per tensor)."""
        tab, state = c["tab"], self.state
        tabp = tab["p"]
        cols = [(k, key, tab[field]) for k, (field, key) in enumerate(self._STATE)]
        for i, (p, held, _) in enumerate(c["recs"]):
            if p.data_ptr() != tabp[i]:
                return True
            st = state[p]
            for k, key, col in cols:
                if st.get(key) is not held[k] or held[k].data_ptr() != col[i]:
                    return True
        return False

    def _run(self, key, select, _retry=True):
        """One fused launch over the parameters `select` accepts (on the current stream)."""
        ps = self._passes.setdefault(key, _Pass())
        c = ps.cache
        # fast path: the same parameters have gradients as last step (the usual case) - only the gradient pointers, the
        # per-step fields and the |max| arrays are refreshed; anything else re-scans
        if c is not None:
            grads = [p.grad for p, _, _ in c["recs"]]
            stale = any(g is None for g in grads) or self._rule() != c["rule"]
            stale = stale or self._pointers_moved(c)
            if not stale and self._check_every_step:
                n_sel = sum(1 for g in self.param_groups for p in g["params"] if p.grad is not None and select(p))
                stale = n_sel != len(grads)
            if stale:
                c = None
        if c is None:
            if not self._scan(ps, select):
                return
            c = ps.cache
            grads = [p.grad for p, _, _ in c["recs"]]
        tab, dev = c["tab"], c["dev"]
        keep, gp = [], []
        for g in grads:
            if g.dtype != torch.float32 or not g.is_contiguous():
                if g.dtype != torch.float32 or g.is_sparse:
                    raise NotImplementedError(self._NAME + ": dense fp32 gradients")
                g = g.contiguous()
                keep.append(g)
            gp.append(g.data_ptr())
        tab["g"] = gp
        if any(gp[i] & 15 for i, _, _, _ in c["amax_off"]):
            # a gradient view at an odd offset this step (rare): re-scan, the tensor takes flat mode
            ps.cache = None
            if not _retry:
                raise _lib.CimHipError(self._NAME + ": inconsistent gradient alignment")
            return self._run(key, select, _retry=False)
        self._fill(tab, c)
        # row / column |max| arrays of the matrix-mode tensors: fresh (zeroed) storage every step - consumers of the
        # previous step's arrays (autograd graphs kept alive) never see them change
        amax_buf = torch.zeros(max(c["n_amax"], 1), dtype=torch.int32, device=dev)
        base = amax_buf.data_ptr()
        slices = []
        for i, off, rows, cols in c["amax_off"]:
            tab["row_amax"][i], tab["col_amax"][i] = base + 4 * off, base + 4 * (off + rows)
            slices.append((c["recs"][i][0], amax_buf[off:off + rows], amax_buf[off + rows:off + rows + cols], rows, cols))
        c["staged"].upload(tab)
        self._launch(c, ps, self.trail_workgroups if key == "trail" else 0)
        # the kernel wrote parameters and state tensors through raw pointers: tell autograd's version counters, so that
        # anything keyed by Tensor._version (saved-tensor checks, caches) sees the in-place update
        torch.autograd.graph.increment_version(c["touched"])
        if slices:      # hand the by-product scales to the contraction ops (valid for exactly this version of the weight)
            from ..ops import gemm
            for p, ra, ca, rows, cols in slices:
                gemm.register_weight_scales(p, rows, cols, ra, ca)
        return c["ids"]

    def _invalidate(self):
        for ps in self._passes.values():
            ps.cache = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._invalidate()              # new state tensors: the cached pointers are dead

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_passes", {})
        self.__dict__.setdefault("_early", None)
        self.__dict__.setdefault("_check_every_step", True)
        self._invalidate()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_passes"):
            self._invalidate()

    # ------------------------------------------------------------------ the step and its placements
    def _before_launches(self):
        """Called at the top of step() and step_early(), before anything is enqueued."""

    @torch.no_grad()
    def step_early(self, params, stream):
        """Update `params` NOW, on `stream`, ahead of `step()` - called from inside the backward pass once their gradients
        are final (nn.DataParallel.attach_optimizer): the 1 GB of MaskFuse weights is updated while the backward of the
        backbone - small latency-bound launches that leave HBM idle - is still running.  The following `step()` updates
        only the remaining parameters and makes the caller's stream wait for this one."""
        self._before_launches()
        ids = frozenset(id(p) for p in params)
        cur = torch.cuda.current_stream()
        stream.wait_stream(cur)
        with torch.cuda.stream(stream):
            done = self._run("early", lambda p: id(p) in ids)
        ev = torch.cuda.Event()
        ev.record(stream)
        for p in params:                                 # the side stream reads / writes these; keep the allocator informed
            if p.grad is not None:
                p.grad.record_stream(stream)
        self._early = (done or frozenset(), stream, ev)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._before_launches()
        _join_side()            # weight gradients deferred to the side stream (cim_amd/ops/gemm.py; normally joined at the end of backward)
        if self._early is not None:
            done, stream, ev = self._early
            self._early = None
            self._run("rest", lambda p: id(p) not in done)
            torch.cuda.current_stream().wait_event(ev)  # everything after the step sees the early update too
        elif self.overlap_update and not torch.cuda.is_current_stream_capturing():
            self._step_overlapped()
        else:
            self._run("all", lambda p: True)
        return loss

    def _step_overlapped(self):
        from ..ops import gemm
        big = [p for g in self.param_groups for p in g["params"]
               if p.grad is not None and p.is_cuda and p.numel() >= TRAIL_MIN and _matrix_shape(p) is not None]
        ids = frozenset(id(p) for p in big)
        self._run("rest", lambda p: id(p) not in ids)
        if not big:
            return
        dev = big[0].device
        cur, side = torch.cuda.current_stream(dev), gemm._side_stream(dev)
        gemm.wait_pending_updates(dev)                   # (a previous trailing update nobody waited for: same stream order anyway)
        side.wait_stream(cur)                            # gradients final, the small parameters' launch enqueued
        with torch.cuda.stream(side):
            self._run("trail", lambda p: id(p) in ids)
            ev = torch.cuda.Event()
            ev.record(side)
        for p in big:                                    # zero_grad() drops these while the side stream may still read them
            p.grad.record_stream(side)
        gemm.register_pending_update(dev, ev, ids)

    def zero_grad(self, set_to_none=True):
        if not set_to_none:
            self.wait_update()          # (zeroing in place: the side stream may still read the big weights' gradients)
        return super().zero_grad(set_to_none=set_to_none)

    def wait_update(self):
        """Make the current stream wait for an update that is still running on the side stream (overlap_update)."""
        from ..ops import gemm
        gemm.wait_pending_updates()

    def state_dict(self):
        self.wait_update()              # (state tensors of the big weights may still be written on the side stream)
        return super().state_dict()
