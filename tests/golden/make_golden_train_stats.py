#!/usr/bin/env python3
"""Capture the training-statistics golden by RUNNING THE REFERENCE (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_train_stats.py      # rewrites tests/golden/train_stats.npz

Runs the reference's own lib/utils/training_stats.py `TrainingStats` (UpdateIterStats with inner_iter, GetStats) on CPU
tensors, for iter_size 1..5 and 45 optimizer steps each, and its lib/utils/logging.py `log_stats` for one line of each of
its two shapes.  Nothing of the reference is written into this repository.

Inputs: the four losses in the model's order, magnitudes mixed over 1e-3 .. 1e3, half of them drawn from a small pool so
that windows hold ties.  Asserted here, because the tests would be blind otherwise: summing the four in another order changes
the fp32 total for at least one step of every sequence, and at least one captured window has a tie at its middle.
The .npz is written with fixed zip timestamps so a rerun is byte-identical.
"""
import contextlib
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402

F32 = np.float32
KEYS = ("bag_loss", "pcl_loss", "cls_loss", "iou_loss")
ITER_SIZES = (1, 2, 3, 4, 5)
STEPS = 45
CAPTURE = (1, 2, 19, 20, 21, 40, 45)          # after this many optimizer steps: part-full odd / even, full, wrapped windows
MAX_ITER = 40000
LOG_ARGS = dict(run_name="Jan01-00-00-00_node_step", cfg_filename="resnet50_voc", iter_size=1)
LOG_EPOCH = dict(epoch=3, step=120, iters_per_epoch=5011)
LOG_TIME, LOG_ETA, LOG_LR = 0.412345, "4:34:52", 0.00125


def make_values(rng, n):
    pool = (10.0 ** rng.uniform(-3, 3, size=(6, len(KEYS)))).astype(F32)
    fresh = (10.0 ** rng.uniform(-3, 3, size=(n, len(KEYS)))).astype(F32)
    pick = pool[rng.randint(0, 6, size=(n, len(KEYS))), np.arange(len(KEYS))]
    return np.where(rng.rand(n, len(KEYS)) < 0.5, pick, fresh).astype(F32)


def order_matters(values):
    a = ((F32(0) + values[:, 0] + values[:, 1]) + values[:, 2]) + values[:, 3]
    b = ((F32(0) + values[:, 3] + values[:, 2]) + values[:, 1]) + values[:, 0]
    return bool(np.any(a != b))


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps (a rerun gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    _ref_shims.install()
    np.float, np.int = float, int                      # removed NumPy aliases the reference still uses
    cfg = importlib.import_module("core.config").cfg
    ref = importlib.import_module("utils.training_stats")
    ref_logging = importlib.import_module("utils.logging")
    if cfg.is_immutable():
        cfg.immutable(False)
    cfg.NUM_GPUS = 1
    cfg.SOLVER.MAX_ITER = MAX_ITER
    rng = np.random.RandomState(20261019)
    out = dict(keys=np.array(KEYS), iter_sizes=np.int32(ITER_SIZES), capture=np.int32(CAPTURE), max_iter=np.int32(MAX_ITER))
    middle_tie = False
    last_stats = None
    for it in ITER_SIZES:
        values = make_values(rng, STEPS * it)
        assert order_matters(values), "iter_size %d: no step whose fp32 total depends on the summation order" % it
        ts = ref.TrainingStats(types.SimpleNamespace(iter_size=it))
        totals, loss, heads = [], [], []
        for step in range(STEPS):
            for inner in range(it):
                row = values[step * it + inner]
                model_out = dict(losses={k: torch.tensor([row[j]]) for j, k in enumerate(KEYS)})
                ts.UpdateIterStats(model_out, inner)
                assert model_out["total_loss"].dtype == torch.float32 and model_out["total_loss"].shape == (1,)
                totals.append(model_out["total_loss"].numpy()[0])
            if step + 1 in CAPTURE:
                stats = ts.GetStats(step, LOG_LR)
                assert list(stats) == ["iter", "time", "eta", "loss", "lr", "head_losses"] and list(stats["head_losses"]) == list(KEYS)
                assert all(type(v) is F32 for v in [stats["loss"]] + list(stats["head_losses"].values()))
                loss.append(stats["loss"])
                heads.append([stats["head_losses"][k] for k in KEYS])
                for sv in list(ts.smoothed_losses.values()) + [ts.smoothed_total_loss]:
                    w = np.sort(np.array(sv.deque, dtype=F32))
                    n = len(w)
                    if n >= 2 and n % 2 == 0:
                        middle_tie |= bool(w[n // 2 - 1] == w[n // 2])
                    elif n >= 3:
                        middle_tie |= bool(w[n // 2] == w[n // 2 - 1] or w[n // 2] == w[n // 2 + 1])
                last_stats = stats
        out.update({"values/%d" % it: values, "total/%d" % it: F32(totals), "loss/%d" % it: F32(loss), "heads/%d" % it: F32(heads)})
        print("iter_size", it, "loss medians", F32(loss))
    assert middle_tie, "no captured window with a tie at its middle"

    # one line of each shape of log_stats, from the last captured statistics with a fixed clock
    last_stats["time"], last_stats["eta"] = LOG_TIME, LOG_ETA
    lines = []
    for extra in ({}, LOG_EPOCH):
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            ref_logging.log_stats(last_stats, types.SimpleNamespace(**LOG_ARGS, **extra))
        lines.append(buf.getvalue())
        print(lines[-1], end="")
    out.update(log_step=np.array(lines[0]), log_epoch=np.array(lines[1]), log_iter=np.int32(last_stats["iter"]),
               log_clock=np.array([str(LOG_TIME), LOG_ETA, str(LOG_LR)]), log_run=np.array([LOG_ARGS["run_name"], LOG_ARGS["cfg_filename"]]),
               log_epoch_args=np.int32([LOG_EPOCH["epoch"], LOG_EPOCH["step"], LOG_EPOCH["iters_per_epoch"]]))
    save_npz(os.path.join(HERE, "train_stats.npz"), out)


if __name__ == "__main__":
    main()
