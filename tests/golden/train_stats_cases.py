"""Shared by tests/test_train_stats_cpu.py and tests/test_gpu_train_stats.py: the golden of make_golden_train_stats.py and the
loop that drives a TrainingStats over one of its sequences the way tools/train.py:418-441 does."""
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
STEPS = 45


def load():
    g = np.load(os.path.join(HERE, "train_stats.npz"))
    return {k: g[k] for k in g.files}


def bits(a):
    """fp32 values as bit patterns, with -0.0 folded onto +0.0 (zeros compare by value)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    return np.where(a == 0, F32(0), a).view(np.uint32)


def drive(golden, it, to_tensor, steps=STEPS, capture=None, on_step=None, **kw):
    """Run cim_amd's TrainingStats over the golden sequence of iter_size `it`.  -> (stats object, totals left in model_out
    [steps * it] as tensors, {optimizer steps done: GetStats result} for the steps in `capture`)."""
    from cim_amd.utils.training_stats import TrainingStats
    keys = [str(k) for k in golden["keys"]]
    values = golden["values/%d" % it]
    ts = TrainingStats(types.SimpleNamespace(iter_size=it, run_name="run", cfg_filename="cfg"), **kw)
    totals, stats = [], {}
    for step in range(steps):
        for inner in range(it):
            row = values[step * it + inner]
            model_out = dict(losses={k: to_tensor(row[j:j + 1]) for j, k in enumerate(keys)})
            ts.UpdateIterStats(model_out, inner)
            totals.append(model_out["total_loss"])
        if capture is not None and step + 1 in capture:
            stats[step + 1] = ts.GetStats(step, 0.00125)
        if on_step is not None:
            on_step(ts, step)
    return ts, totals, stats
