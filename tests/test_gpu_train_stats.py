"""Training statistics on the device (csrc/train_stats.hip, cim_amd.utils.training_stats).

Everything here is exact: the kernels' fp32 operations are the reference's, one rounding each, so medians, last values and
totals are compared BIT FOR BIT - with the golden captured from the reference's own TrainingStats
(tests/golden/make_golden_train_stats.py) where it covers the case (window 20, the four losses), with the package's host path
(np.float32 adds, np.median; itself pinned to the golden by tests/test_train_stats_cpu.py) elsewhere.  Zeros compare by value.
The one inexact figure is the global mean: fp64 sum / count rounded to fp32 against math.fsum, 1 fp32 ulp (45 .. 225 fp64
additions of fp32 values err by < 225 * 2^-53 relative, far below half an fp32 ulp: only the final rounding remains, and a
double rounding may land on the neighbour).
"""
import contextlib
import ctypes
import io
import math
import threading
import types

import numpy as np
import pytest
import torch

import train_stats_cases as tsc

pytestmark = pytest.mark.gpu

POISON = 0x7FA5A5A5          # a NaN bit pattern: a guard word that is read poisons a result, one that is written changes its bits
GUARD = 64                   # poison words on either side of the state, of `out` and of the values
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return tsc.load()


@pytest.fixture(autouse=True)
def own_cfg():
    from cim_amd.core import config as own
    own.reset_cfg()
    yield own.cfg
    own.reset_cfg()


def _ulps(a, b):
    a, b = F32(a), F32(b)
    assert np.isfinite(a) and np.isfinite(b), (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


class Device:
    """One tracker at the C ABI: its state and `out` each between poison bands in ONE int32 image, the values between bands too."""

    def __init__(self, dev, n_values, window, values):
        from cim_amd import _lib
        self.lib, self.n_values, self.window, self.cols = _lib, n_values, window, n_values + 1
        nbytes = _lib.call("cim_stats_bytes", n_values, window)
        assert nbytes > 0 and nbytes % 4 == 0
        self.state_words, self.out_words = (nbytes // 4 + 1) & ~1, 3 * self.cols + 2
        image = np.full(3 * GUARD + self.state_words + self.out_words, POISON, dtype=np.uint32)
        self.s0, self.o0 = GUARD, 2 * GUARD + self.state_words
        image[self.s0:self.s0 + nbytes // 4] = 0                      # the caller's zero fill; `out` starts as poison (write-only)
        self.inside = np.zeros(image.shape, dtype=bool)
        self.inside[self.s0:self.s0 + nbytes // 4] = True
        self.inside[self.o0:self.o0 + self.out_words] = True
        self.buf = torch.from_numpy(image.view(np.int32)).to(dev)
        assert (self.buf.data_ptr() + 4 * self.s0) % 8 == 0
        values = np.ascontiguousarray(values, dtype=F32)
        vimg = np.full(values.size + 2 * GUARD, POISON, dtype=np.uint32)
        vimg[GUARD:GUARD + values.size] = values.reshape(-1).view(np.uint32)
        self.vimg, self.vbuf = vimg, torch.from_numpy(vimg.view(np.int32)).to(dev)
        self.addr = (ctypes.c_uint64 * 16)()

    def push(self, first, n_sum, iter_size=1, inner=0, n_values=None, window=None):
        """Values first .. first + n_values - 1 of the flat value array."""
        n = self.n_values if n_values is None else n_values
        for k in range(min(max(n, 0), 16)):
            self.addr[k] = self.vbuf.data_ptr() + 4 * (GUARD + first + k)
        self.lib.call("cim_stats_push", self.addr, n, n_sum, self.window if window is None else window, iter_size, inner,
                      self.buf.data_ptr() + 4 * self.s0, self.lib.stream_ptr())

    def image(self):
        torch.cuda.current_stream().synchronize()
        return self.buf.cpu().numpy().view(np.uint32)

    def summary(self):
        """-> (float32 [cols][3], first non-finite commit, commits); asserts every guard word and every value word unchanged."""
        self.lib.call("cim_stats_summary", self.buf.data_ptr() + 4 * self.s0, self.n_values, self.window,
                      self.buf.data_ptr() + 4 * self.o0, self.lib.stream_ptr())
        image = self.image()
        assert np.all(image[~self.inside] == POISON), "a guard word around the state or `out` was written"
        assert np.array_equal(self.vbuf.cpu().numpy().view(np.uint32), self.vimg)
        out = image[self.o0:self.o0 + self.out_words]
        assert not np.any(out == POISON), "a word of `out` was left unwritten"
        tail = out[3 * self.cols:].view(np.int32)
        return out[:3 * self.cols].view(F32).reshape(self.cols, 3).copy(), int(tail[0]), int(tail[1])


def _host(n_values, window):
    from cim_amd.utils.training_stats import _HostTracker
    return _HostTracker(n_values, window)


def _same(got, want, mean_ulps=1):
    """Device summary against the host path: median and last bit for bit, the global mean within `mean_ulps`."""
    (g, gbad, gcount), (w, wbad, wcount) = got, want
    assert (gbad, gcount) == (wbad, wcount)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    ok = ~np.isnan(w[:, :2])
    assert np.array_equal(tsc.bits(g[:, :2][ok]), tsc.bits(w[:, :2][ok])), (g, w)
    for a, b in zip(g[:, 2], w[:, 2]):
        if np.isfinite(b):
            assert _ulps(a, b) <= mean_ulps, (a, b)
        else:
            assert (np.isnan(a) and np.isnan(b)) or a == b, (a, b)


# ------------------------------------------------------------------ 1. the C ABI on the golden sequences
@pytest.mark.parametrize("it", [1, 2, 3, 4, 5])
def test_c_abi_equals_the_reference_at_window_20(dev, golden, it):
    values = golden["values/%d" % it]
    d, h = Device(dev, 4, 20, values), _host(4, 20)
    capture = [int(c) for c in golden["capture"]]
    for step in range(tsc.STEPS):
        for inner in range(it):
            row = step * it + inner
            d.push(4 * row, 4, it, inner)
            h.push(list(values[row]), 4, it, inner)
        if step + 1 in capture:
            i = capture.index(step + 1)
            out, bad, count = got = d.summary()
            print("iter_size", it, "step", step + 1, "median total", out[4, 0], "golden", golden["loss/%d" % it][i])
            assert bad == 0 and count == step + 1 and np.all(np.isfinite(out))              # (no poison was read)
            assert np.array_equal(tsc.bits(out[:4, 0]), tsc.bits(golden["heads/%d" % it][i]))
            assert tsc.bits(out[4, 0]) == tsc.bits(golden["loss/%d" % it][i])
            if it == 1:
                assert tsc.bits(out[4, 1]) == tsc.bits(golden["total/1"][step])              # the last committed total
                assert np.array_equal(tsc.bits(out[:4, 1]), tsc.bits(values[step]))
            _same(got, h.summary())


@pytest.mark.parametrize("window", [1, 2, 3, 64])
def test_other_windows_against_the_host_path(dev, golden, window):
    values = golden["values/5"]                                      # 225 rows: as iter_size 1 they wrap a window of 64 three times
    d, h = Device(dev, 4, window, values), _host(4, window)
    _same(d.summary(), h.summary())                                  # count == 0
    for step in range(len(values)):
        d.push(4 * step, 4)
        h.push(list(values[step]), 4, 1, 0)
        if step + 1 in (1, 2, 3, 4, 5, 63, 64, 65, 66, 128, 129, 225):
            _same(d.summary(), h.summary())
    mean = d.summary()[0][:, 2]
    for k in range(4):                                               # the global mean against math.fsum
        assert _ulps(mean[k], F32(math.fsum(float(x) for x in values[:, k]) / len(values))) <= 1


def test_sixteen_values_four_in_the_total(dev, golden):
    values = golden["values/4"].reshape(tsc.STEPS, 16)
    d, h = Device(dev, 16, 20, values), _host(16, 20)
    for step in range(30):                                           # 30 commits at iter_size 1 ...
        d.push(16 * step, 4)
        h.push(list(values[step]), 4, 1, 0)
        if step in (0, 9, 28, 29):
            out, _, _ = got = d.summary()
            v = values[step]
            assert tsc.bits(out[16, 1]) == tsc.bits((((F32(0) + v[0]) + v[1]) + v[2]) + v[3])        # the extras are not in it
            assert np.array_equal(tsc.bits(out[:16, 1]), tsc.bits(v))                              # ... and are tracked
            _same(got, h.summary())
    for commit in range(5):                                          # ... then 5 more through iter_size 3
        for inner in range(3):
            row = 30 + 3 * commit + inner
            d.push(16 * row, 4, 3, inner)
            h.push(list(values[row]), 4, 3, inner)
        _same(d.summary(), h.summary())
    assert d.summary()[2] == 35


# ------------------------------------------------------------------ 2. edges
def test_nan_and_inf_pass_through_the_window_and_the_first_step_sticks(dev):
    window, n = 5, 16
    values = (np.arange(2 * n, dtype=F32).reshape(n, 2) * F32(0.37) + F32(1)) * F32([1, -3])
    values[3] = (np.nan, np.inf)                                     # commit 4: a NaN in key 0, an Inf in key 1
    values[11, 1] = np.nan                                           # a later one: the sticky word must keep 4
    d, h = Device(dev, 2, window, values), _host(2, window)
    for step in range(n):
        d.push(2 * step, 2)
        h.push(list(values[step]), 2, 1, 0)
        out, bad, count = got = d.summary()
        _same(got, h.summary())
        assert bad == (0 if step < 3 else 4) and count == step + 1
        in_window = 3 <= step < 3 + window
        assert bool(np.isnan(out[0, 0])) == in_window and bool(np.isnan(out[2, 0])) == (in_window or 11 <= step)      # NaN + inf = NaN
        if step < 11:
            assert np.isfinite(out[1, 0])                            # one +inf sorts to the end of five: the median stays finite
    assert np.isfinite(d.summary()[0][0, 0])                         # finite again `window` commits later


@pytest.mark.parametrize("window", [4, 5])
def test_all_ties_and_signed_zeros(dev, window):
    values = np.array([[2.5, 0.0]] * 3 + [[2.5, -0.0]] * 4, dtype=F32)
    d, h = Device(dev, 2, window, values), _host(2, window)
    for step in range(len(values)):
        d.push(2 * step, 2)
        h.push(list(values[step]), 2, 1, 0)
        got = d.summary()
        assert got[0][0, 0] == F32(2.5) and got[0][1, 0] == 0 and got[0][2, 0] == F32(2.5)
        _same(got, h.summary())


def test_an_empty_state_gives_nan(dev):
    out, bad, count = Device(dev, 3, 20, np.zeros(3)).summary()
    assert np.all(np.isnan(out)) and (bad, count) == (0, 0)


# ------------------------------------------------------------------ 4. argument errors
def test_argument_errors_launch_nothing(dev, golden):
    from cim_amd import _lib
    values = golden["values/2"]
    d = Device(dev, 4, 20, values)
    for row in range(3):                                             # a state that is not all zero: commit 1, and inner 0 of commit 2
        d.push(4 * row, 4, 2, row % 2)
    before = d.image().copy()
    bad = [dict(n_values=0), dict(n_values=17), dict(n_sum=5), dict(window=0), dict(window=65), dict(iter_size=0),
           dict(iter_size=2, inner=-1), dict(iter_size=2, inner=2), dict(iter_size=1, inner=1)]
    for case in bad:
        kw = dict(dict(n_sum=4, iter_size=2, inner=1), **case)
        with pytest.raises(_lib.CimHipError, match="cim_stats_push: bad argument"):
            d.push(0, **kw)
    state, out = d.buf.data_ptr() + 4 * d.s0, d.buf.data_ptr() + 4 * d.o0
    for n_keys, window in ((0, 20), (17, 20), (4, 0), (4, 65)):
        with pytest.raises(_lib.CimHipError, match="cim_stats_summary: bad argument"):
            _lib.call("cim_stats_summary", state, n_keys, window, out, _lib.stream_ptr())
        assert _lib.call("cim_stats_bytes", n_keys, window) == -1
    with pytest.raises(_lib.CimHipError, match="bad argument"):
        _lib.call("cim_stats_push", d.addr, 4, 4, 20, 1, 0, None, _lib.stream_ptr())
    with pytest.raises(_lib.CimHipError, match="cim_stats_push: bad argument"):          # the fp64 sums need 8-byte alignment
        _lib.call("cim_stats_push", d.addr, 4, 4, 20, 1, 0, state + 4, _lib.stream_ptr())
    with pytest.raises(_lib.CimHipError, match="cim_stats_summary: bad argument"):
        _lib.call("cim_stats_summary", state + 4, 4, 20, out, _lib.stream_ptr())
    assert np.array_equal(d.image(), before)                         # state, `out` and the guards: untouched
    d.push(4 * 3, 4, 2, 1)                                           # and the sequence goes on as if nothing had happened
    h = _host(4, 20)
    for row in range(4):
        h.push(list(values[row]), 4, 2, row % 2)
    _same(d.summary(), h.summary())


# ------------------------------------------------------------------ 5. the class on device tensors
def _log_text(golden, it, to_tensor, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ts, totals, stats = tsc.drive(golden, it, to_tensor, capture=[int(c) for c in golden["capture"]], log_period=20,
                                      on_step=lambda ts, step: ts.LogIterStats(step, 0.00125), **kw)
        ts.flush()
    return ts, totals, stats, buf.getvalue()


@pytest.mark.parametrize("it", [1, 2, 3, 4, 5])
def test_class_equals_the_reference_in_both_modes(dev, golden, own_cfg, it):
    own_cfg.SOLVER.MAX_ITER = tsc.STEPS
    keys = [str(k) for k in golden["keys"]]
    _, _, _, host_text = _log_text(golden, it, lambda a: torch.from_numpy(a.copy()))
    for deferred in (False, True):
        ts, totals, stats, text = _log_text(golden, it, lambda a: torch.from_numpy(a.copy()).to(dev), deferred=deferred)
        assert all(t.is_cuda and t.shape == (1,) for t in totals)
        assert np.array_equal(tsc.bits(torch.cat(totals).cpu().numpy()), tsc.bits(golden["total/%d" % it]))
        for i, c in enumerate(int(c) for c in golden["capture"]):
            s = stats[c]
            assert list(s) == ["iter", "time", "eta", "loss", "lr", "head_losses"] and list(s["head_losses"]) == keys
            assert type(s["loss"]) is np.float32 and tsc.bits(s["loss"]) == tsc.bits(golden["loss/%d" % it][i])
            assert np.array_equal(tsc.bits([s["head_losses"][k] for k in keys]), tsc.bits(golden["heads/%d" % it][i]))
        heads = [ln.split("[Step ")[1] for ln in text.splitlines() if ln.startswith("[")]
        assert heads == ["1 / 45]", "21 / 45]", "41 / 45]", "45 / 45]"]                     # every record, in order
        assert text == host_text and ("loss: %.6f" % golden["loss/%d" % it][4]) in text     # (step 21 is a captured one)
        assert not ts._pending and ts.nonfinite_step() is None


def test_flush_prints_every_queued_record_in_order(dev, golden, own_cfg):
    """Deferred mode with nothing that waits (no GetStats): behind a sleep kernel of about 0.3 s all four records of the run are
    still queued when the loop ends, and flush() prints them in order - the text of the host path."""
    own_cfg.SOLVER.MAX_ITER = tsc.STEPS
    log = lambda ts, step: ts.LogIterStats(step, 0.00125)        # noqa: E731
    host = io.StringIO()
    with contextlib.redirect_stdout(host):
        tsc.drive(golden, 3, lambda a: torch.from_numpy(a.copy()), on_step=log, log_period=20)
    values = torch.from_numpy(golden["values/3"].copy()).to(dev)
    rows = iter(values.reshape(-1, 1))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        torch.cuda.synchronize()
        torch.cuda._sleep(int(0.3 / 1.4e-3 * 3000000))
        ts, _, _ = tsc.drive(golden, 3, lambda a: next(rows), on_step=log, log_period=20, deferred=True)
        queued, early = len(ts._pending), buf.getvalue()
        ts.flush()
    assert queued == 4 and early == "", "a record was printed while the sleep kernel was still in front of it"
    assert buf.getvalue() == host.getvalue() and buf.getvalue().count("[Step ") == 4 and not ts._pending


def test_backward_through_the_total_it_leaves(dev):
    from cim_amd.utils.training_stats import TrainingStats
    x = torch.tensor([3.0, -0.125, 1e3, 7e-3], device=dev)
    grads = []
    for mine in (True, False):
        w = torch.tensor([0.5, 2.0, -1.5, 4.0], device=dev, requires_grad=True)
        losses = {k: w[j:j + 1] * x[j:j + 1] for j, k in enumerate("abcd")}
        if mine:
            out = dict(losses=dict(losses))
            TrainingStats(types.SimpleNamespace(iter_size=1)).UpdateIterStats(out)
            assert all(out["losses"][k] is losses[k] for k in losses)                       # left as they are
            total = out["total_loss"]
        else:
            total = 0
            for loss in losses.values():                                                    # training_stats.py:72-83
                total += loss.mean(dim=0, keepdim=True)
        total.backward()
        grads.append(w.grad.cpu().numpy())
    assert np.array_equal(grads[0], grads[1]) and np.array_equal(grads[0], x.cpu().numpy())
    ts = TrainingStats(types.SimpleNamespace(iter_size=1))
    supplied = torch.tensor([5.0], device=dev)
    out = dict(losses={"a": torch.tensor([2.0], device=dev), "b": torch.tensor([0.25], device=dev)}, total_loss=supplied)
    ts.UpdateIterStats(out, extra={"grad_norm": torch.tensor([9.0], device=dev)[0:1]})
    assert out["total_loss"] is supplied
    s = ts.GetStats(0, 0.1)
    assert s["loss"] == F32(2.25) and s["grad_norm"] == F32(9.0) and list(s)[-2:] == ["head_losses", "grad_norm"]
    with pytest.raises(ValueError):
        ts.UpdateIterStats(dict(losses={"a": torch.tensor([2.0]), "b": torch.tensor([0.25])}))      # CPU tensors on a device tracker


# ------------------------------------------------------------------ 6. no host wait
def test_deferred_mode_never_waits_for_the_device(dev, golden, own_cfg):
    from cim_amd.utils.training_stats import TrainingStats
    own_cfg.SOLVER.MAX_ITER = 1000
    values = golden["values/1"]
    keys = [str(k) for k in golden["keys"]]
    args = types.SimpleNamespace(iter_size=1, run_name="run", cfg_filename="cfg")
    rows = [{k: torch.tensor([values[r, j]], device=dev) for j, k in enumerate(keys)} for r in range(12)]

    def calls(ts, first, tensors=rows, lr=0.01):
        for r in range(first, first + 3):
            ts.UpdateIterStats(dict(losses=dict(tensors[r])))
        ts.LogIterStats(20 * (first // 3), lr)

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ts = TrainingStats(args, deferred=True)
        calls(ts, 0)                                    # warm-up: the state, and the pinned buffer the pool hands out again
        ts.flush()
        warm = buf.getvalue()
        assert warm.count("[Step ") == 1 and len(ts._tracker.free) == ts._tracker.POOL
        torch.cuda.synchronize()
        torch.cuda._sleep(int(0.5 / 1.4e-3 * 3000000))          # about 0.5 s on the stream (3 000 000 cycles: about 1.4 ms)
        ev = torch.cuda.Event()
        ev.record()
        calls(ts, 3)
        calls(ts, 6)                                    # a second record while the first is still queued
        still_running = not ev.query()
        printed_early = buf.getvalue() != warm
        # where the build enforces it: the same calls with every synchronising call an error
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                rows[0][keys[0]].item()
                enforced = False
            except RuntimeError:
                enforced = True
            if enforced:
                calls(ts, 9)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert still_running, "the sleep kernel finished before the calls returned: they waited (or the sleep is too short)"
        assert not printed_early and len(ts._pending) == (3 if enforced else 2)
        ts.flush()
    print("sync debug mode enforced:", enforced)
    # the values: a CPU twin driven by the same calls prints the same text
    twin_buf = io.StringIO()
    with contextlib.redirect_stdout(twin_buf):
        twin = TrainingStats(args)
        cpu_rows = [{k: v.cpu() for k, v in row.items()} for row in rows]
        calls(twin, 0, cpu_rows)
        calls(twin, 3, cpu_rows)
        calls(twin, 6, cpu_rows)
        if enforced:
            calls(twin, 9, cpu_rows)
    text = buf.getvalue()
    assert text == twin_buf.getvalue() and text.count("[Step ") == (4 if enforced else 3)


# ------------------------------------------------------------------ 7. re-entrancy
def test_two_trackers_on_two_streams_from_two_threads(dev, golden):
    plans = [(2, golden["values/2"], 20), (3, golden["values/3"], 7)]

    def run(plan, barrier=None, stream=None, result=None):
        it, values, window = plan
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            d = Device(dev, 4, window, values)
            if barrier is not None:
                barrier.wait()
            outs = []
            for row in range(len(values)):
                d.push(4 * row, 4, it, row % it)
                if row % 31 == 30:
                    outs.append(d.summary())
            outs.append(d.summary())
        if result is not None:
            result.append(outs)
        return outs

    alone = [run(p) for p in plans]
    barrier, results, errors = threading.Barrier(2), [[], []], []

    def worker(i):
        try:
            torch.cuda.set_device(dev)
            run(plans[i], barrier, torch.cuda.Stream(device=dev), results[i])
        except BaseException as e:          # noqa: BLE001  (reported by the main thread)
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert len(results[i][0]) == len(alone[i])
        for (g, gb, gc), (w, wb, wc) in zip(results[i][0], alone[i]):
            assert (gb, gc) == (wb, wc) and np.array_equal(g.view(np.uint32), w.view(np.uint32))
