"""Training statistics with the bookkeeping on the device (cim_amd/csrc/train_stats.hip).

A drop-in for the reference's `utils.training_stats.TrainingStats` (lib/utils/training_stats.py:36-167) and the `log_stats` it
prints with (lib/utils/logging.py:42-57).  The reference reads every loss and the total back with `.cpu()` in `UpdateIterStats`
(:81,85,110,118): five blocking reads per step between the forward and the backward pass.  Here `UpdateIterStats` is ONE
single-wave launch (`cim_stats_push`: total in the reference's order, iter_size accumulation, a ring of the last `window`
values per key) and a logging `LogIterStats` is one launch (`cim_stats_summary`: np.median's median per key) plus one copy into
pinned memory; the host waits once per logging period, or - `deferred=True` - never: records are printed by a later
`LogIterStats` call once their copy has completed, `flush()` prints the rest.

CPU tensors (CPU models exist) take a host path with the same fp32 arithmetic: a deque, np.float32 adds, np.median.  CUDA/HIP
tensors have no fallback: a failed launch raises CimHipError.
"""
import ctypes
import datetime
import time
from collections import OrderedDict, deque

import numpy as np
import torch

from .. import _lib
from ..core.config import cfg

_NAME = "cim_amd.utils.training_stats.TrainingStats"
_F32 = np.float32
_STANDARD = ("iter", "time", "eta", "loss", "lr", "head_losses")


def _pairs(items):
    return "\t\t" + ", ".join("%s: %.6f" % kv for kv in items)


def log_stats(stats, misc_args):
    """Print one record of the loss log.  The text is the reference's (lib/utils/logging.py:42-57), character for character -
    tests/golden/train_stats.npz holds one recorded record of each of its two headings: the epoch heading when `misc_args`
    carries an `epoch`, the step heading otherwise.  Values tracked through UpdateIterStats' `extra` follow on a line of their
    own, in the head losses' form; without them the record is the reference's."""
    run = "[%s][%s]" % (misc_args.run_name, misc_args.cfg_filename)
    if hasattr(misc_args, 'epoch'):
        heading = run + "[Epoch %d][Iter %d / %d]" % (misc_args.epoch, misc_args.step, misc_args.iters_per_epoch)
    else:
        heading = run + "[Step %d / %d]" % (stats['iter'], cfg.SOLVER.MAX_ITER)
    record = [heading, "\t\tloss: %.6f, lr: %.6f time: %.6f, eta: %s" % (stats['loss'], stats['lr'], stats['time'], stats['eta'])]
    for group in (stats['head_losses'].items(), [(k, v) for k, v in stats.items() if k not in _STANDARD]):
        if group:
            record.append(_pairs(group))
    print("\n".join(record))


class Timer(object):
    """Host wall clock of the iterations, with the attributes the reference's utils.timer.Timer exposes (`average_time`,
    `total_time`, `calls`, `diff`, `start_time`): drivers read them."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.start_time = self.diff = self.total_time = self.average_time = 0.0
        self.calls = 0

    def tic(self):
        self.start_time = time.time()

    def toc(self, average=True):
        self.diff = time.time() - self.start_time
        self.calls += 1
        self.total_time += self.diff
        self.average_time = self.total_time / self.calls
        return self.average_time if average else self.diff


class _HostTracker:
    """The arithmetic of csrc/train_stats.hip on the host, operation for operation in np.float32."""

    def __init__(self, n_values, window):
        self.cols, self.window = n_values + 1, window
        self.ring = [deque(maxlen=window) for _ in range(self.cols)]
        self.acc = [_F32(0)] * self.cols
        self.sum = [0.0] * self.cols
        self.count = 0
        self.first_bad = 0

    def push(self, values, n_sum, iter_size, inner):
        t = _F32(0)
        with np.errstate(all="ignore"):
            for v in values[:n_sum]:
                t = _F32(t + v)
            xs = list(values) + [t]
            if iter_size > 1:
                self.acc = [_F32((_F32(0) if inner == 0 else a) + x) for a, x in zip(self.acc, xs)]
                if inner != iter_size - 1:
                    return
                xs = [_F32(a / _F32(iter_size)) for a in self.acc]
        for k, x in enumerate(xs):
            self.ring[k].append(x)
            self.sum[k] += float(x)
        self.count += 1
        if not self.first_bad and not all(np.isfinite(x) for x in xs):
            self.first_bad = self.count

    def summary(self):
        """-> (float32 [cols][3] = median, last, global mean; first non-finite commit or 0; commits)"""
        out = np.full((self.cols, 3), np.nan, dtype=_F32)
        if self.count:
            for k, ring in enumerate(self.ring):
                with np.errstate(all="ignore"):
                    out[k] = (np.median(np.array(ring, dtype=_F32)), ring[-1], _F32(self.sum[k] / self.count))
        return out, self.first_bad, self.count


class _DeviceTracker:
    POOL = 8

    def __init__(self, n_values, window, device):
        self.cols, self.window, self.device = n_values + 1, window, device
        nbytes = _lib.call("cim_stats_bytes", n_values, window)
        if nbytes <= 0:
            raise _lib.CimHipError(_NAME + ": %d tracked values (at most %d) or a window of %d (at most %d)"
                                   % (n_values, _lib.CONSTANTS["CIM_STATS_MAX_KEYS"], window, _lib.CONSTANTS["CIM_STATS_MAX_WIN"]))
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.words = 3 * self.cols + 2
        self.out = torch.empty(self.words, dtype=torch.float32, device=device)
        self.addr = (ctypes.c_uint64 * n_values)()
        # pinned result buffers, one per record in flight.  Allocated HERE: a pinned allocation may serialise with the device,
        # which a logging call must not do; only a loop with more than POOL unprinted records allocates another one
        self.free = [torch.empty(self.words, dtype=torch.float32).pin_memory() for _ in range(self.POOL)]

    def push(self, tensors, n_sum, iter_size, inner):
        for i, t in enumerate(tensors):
            self.addr[i] = t.data_ptr()
        with torch.cuda.device(self.device):
            _lib.call("cim_stats_push", self.addr, len(tensors), n_sum, self.window, iter_size, inner, self.state.data_ptr(),
                      _lib.stream_ptr())

    def summary_async(self):
        """Launch + copy on the current stream -> (pinned float32 [words], event recorded behind the copy)."""
        pinned = self.free.pop() if self.free else torch.empty(self.words, dtype=torch.float32).pin_memory()
        with torch.cuda.device(self.device):
            _lib.call("cim_stats_summary", self.state.data_ptr(), self.cols - 1, self.window, self.out.data_ptr(), _lib.stream_ptr())
            pinned.copy_(self.out, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        return pinned, event

    def read(self, pinned):
        """The host's view of a COMPLETED copy; the buffer goes back to the pool."""
        host = pinned.numpy().copy()
        self.free.append(pinned)
        tail = host[3 * self.cols:].view(np.int32)
        return host[:3 * self.cols].reshape(self.cols, 3), int(tail[0]), int(tail[1])


class TrainingStats(object):
    """The driver's statistics object (tools/train.py:399-441) with the loss bookkeeping on the losses' device."""

    def __init__(self, misc_args, log_period=20, tensorboard_logger=None, *, deferred=False, window=20):
        self.misc_args = misc_args
        self.LOG_PERIOD = log_period
        self.tblogger = tensorboard_logger
        self.tb_ignored_keys = ['iter', 'eta']
        self.iter_timer = Timer()
        self.WIN_SZ = int(window)                       # window of the median filter
        if not 1 <= self.WIN_SZ <= _lib.CONSTANTS["CIM_STATS_MAX_WIN"]:
            raise ValueError(_NAME + ": window %d outside 1..%d" % (self.WIN_SZ, _lib.CONSTANTS["CIM_STATS_MAX_WIN"]))
        self.deferred = bool(deferred)
        self._keys = None                               # (loss keys, extra keys) of the first update: fixed from then on
        self._tracker = None
        self._pending = deque()                         # deferred records: (cur_iter, lr, time, eta, pinned, event)
        self._last_bad = 0                              # first non-finite commit as of the latest summary read

    def IterTic(self):
        self.iter_timer.tic()

    def IterToc(self):
        return self.iter_timer.toc(average=False)

    def ResetIterTimer(self):
        self.iter_timer.reset()

    # ------------------------------------------------------------------ update
    def UpdateIterStats(self, model_out, inner_iter=None, extra=None):
        """Update tracked iteration statistics.  Leaves `model_out['total_loss']` for the backward pass: the model's own when it
        supplied one, else the reference's sum of the losses (torch adds).  `extra`: dict of scalars on the losses' device that
        are tracked and logged beside the losses and are not part of the total (a gradient norm, ...)."""
        iter_size = int(getattr(self.misc_args, "iter_size", 1))
        if inner_iter is not None and iter_size > 1:
            assert 0 <= inner_iter < iter_size
            inner = int(inner_iter)
        else:
            iter_size, inner = 1, 0                     # (training_stats.py:67-71: without inner_iter every call commits)
        losses = model_out['losses']
        for k, loss in losses.items():
            assert loss.shape[0] == cfg.NUM_GPUS
        if cfg.NUM_GPUS > 1:                            # the reference's reduction over the GPUs' rows, on ATen (a rare path)
            total = 0
            for k, loss in losses.items():
                loss = loss.mean(dim=0, keepdim=True)
                total = total + loss
                losses[k] = loss
            model_out['total_loss'] = total
        elif 'total_loss' not in model_out:
            total = 0
            for loss in losses.values():
                total = total + loss
            model_out['total_loss'] = total
        extra = extra or {}
        keys = (tuple(losses), tuple(extra))
        values = [losses[k] for k in keys[0]] + [extra[k] for k in keys[1]]
        if not values:
            raise ValueError(_NAME + ": no losses to track")
        if self._keys is None:
            dup = set(keys[0]) & set(keys[1]) | (set(keys[1]) & set(_STANDARD))
            if dup:
                raise ValueError(_NAME + ": extra keys %s collide with loss or statistics keys" % sorted(dup))
            dev = values[0].device
            self._tracker = (_DeviceTracker if dev.type == "cuda" else _HostTracker)(len(values), self.WIN_SZ, *([dev] if dev.type == "cuda" else []))
            self._keys, self._device = keys, dev
        elif keys != self._keys:
            raise ValueError(_NAME + ": keys %s differ from the first update's %s" % (keys, self._keys))
        for k, v in zip(keys[0] + keys[1], values):
            if v.device != self._device or v.dtype != torch.float32 or v.numel() != 1:
                raise ValueError(_NAME + ": %s must be one float32 value on %s (got %s %s on %s)"
                                 % (k, self._device, tuple(v.shape), v.dtype, v.device))
        if self._device.type == "cuda":
            self._tracker.push(values, len(keys[0]), iter_size, inner)
        else:
            self._tracker.push([_F32(v.detach().reshape(()).item()) for v in values], len(keys[0]), iter_size, inner)

    # ------------------------------------------------------------------ logging
    def _stats(self, cur_iter, lr, avg_time, eta, summary):
        out, bad, _ = summary
        self._last_bad = bad
        stats = OrderedDict(iter=cur_iter + 1, time=avg_time, eta=eta, loss=out[-1, 0], lr=lr)      # iter: 1-indexed
        n = len(self._keys[0])
        stats['head_losses'] = OrderedDict((k, out[i, 0]) for i, k in enumerate(self._keys[0]))
        for i, k in enumerate(self._keys[1]):
            stats[k] = out[n + i, 0]
        return stats

    def _clock(self, cur_iter):
        avg = self.iter_timer.average_time
        return avg, str(datetime.timedelta(seconds=int(avg * (cfg.SOLVER.MAX_ITER - cur_iter))))

    def _require_update(self):
        if self._tracker is None:
            raise RuntimeError(_NAME + ": no UpdateIterStats call yet")

    def _emit(self, stats):
        log_stats(stats, self.misc_args)
        if self.tblogger:
            self.tb_log_stats(stats, stats['iter'] - 1)

    def _drain(self, wait):
        while self._pending and (wait or self._pending[0][5].query()):
            cur_iter, lr, avg, eta, pinned, event = self._pending.popleft()
            event.synchronize()
            self._emit(self._stats(cur_iter, lr, avg, eta, self._tracker.read(pinned)))

    def LogIterStats(self, cur_iter, lr):
        """Log the tracked statistics (every LOG_PERIOD iterations and at the last one).  Default mode waits for the summary's
        copy: the one host wait per logging period.  Deferred mode waits for nothing: it prints the records whose copy has
        completed, in order."""
        if (cur_iter % self.LOG_PERIOD == 0 or cur_iter == cfg.SOLVER.MAX_ITER - 1):
            self._require_update()
            if self._device.type != "cuda":
                self._emit(self._stats(cur_iter, lr, *self._clock(cur_iter), self._tracker.summary()))
            else:
                self._pending.append((cur_iter, lr) + self._clock(cur_iter) + self._tracker.summary_async())
                if not self.deferred:
                    self._drain(wait=True)
        if self._pending:
            self._drain(wait=False)

    def flush(self):
        """Wait for and print every queued record (deferred mode: at the end of training and before a checkpoint)."""
        self._drain(wait=True)

    def tb_log_stats(self, stats, cur_iter):
        """Every number of a record as a tensorboard scalar at `cur_iter` - nested dictionaries (the head losses) flattened,
        `tb_ignored_keys` left out."""
        for key, value in stats.items():
            if key in self.tb_ignored_keys:
                continue
            if isinstance(value, dict):
                self.tb_log_stats(value, cur_iter)
            else:
                self.tblogger.add_scalar(key, value, cur_iter)

    def GetStats(self, cur_iter, lr):
        """The reference's OrderedDict (iter, time, eta, loss, lr, head_losses; then the extra keys).  Returns numbers, so it
        waits for the device; queued records are printed first, in order."""
        self._require_update()
        if self._device.type != "cuda":
            summary = self._tracker.summary()
        else:
            self._drain(wait=True)
            pinned, event = self._tracker.summary_async()
            event.synchronize()
            summary = self._tracker.read(pinned)
        return self._stats(cur_iter, lr, *self._clock(cur_iter), summary)

    def nonfinite_step(self, wait=True):
        """1-based number of the first committed step with a non-finite value, None if there was none.  wait=False: as of the
        latest record already read (nothing is launched, nothing waits)."""
        if wait and self._tracker is not None:
            self.GetStats(0, 0.0)
        return self._last_bad or None
