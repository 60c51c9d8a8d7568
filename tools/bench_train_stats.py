#!/usr/bin/env python3
"""What the training statistics cost in the reference's driver loop (tools/train.py:418-441), on one device.

The loop is bench.py's `reference_loop` setting - resnet50_voc, the 8-image cycle resident on the device, generator settled at
the end of backward, garbage collector not frozen, the whole optimizer update on the loop's stream, backward(retain_graph=True)
- with four ways of keeping the smoothed loss log between the forward and the backward pass:
    A        the reference's statistics restated (lib/utils/training_stats.py:65-128): .mean(0), ATen total, five .cpu() reads
             per optimizer step, np.median over deques every 20 steps
    B        cim_amd.utils.training_stats.TrainingStats, default mode: one launch per image, one host wait per 20 steps
    Bprime   the same class with deferred=True: no host wait inside the window (flush() after it)
    C        no statistics: out['total_loss'].backward() and nothing else
at iter_size 1 and 4, all in one process.  A window is --steps optimizer steps (>= 200) between two device synchronisations;
--rounds rounds in the order A, B, Bprime, C, so drift of the box spreads over all four.  Per variant: ms per image of every
window, their median and their spread (max - min).  The two claims are evaluated and written down, whatever they come to:
Bprime - C within C's own spread, and B <= A.  One JSON line; --out also writes it to a file.

    python tools/bench_train_stats.py [--steps 200] [--rounds 3] [--out profiles/r6/bench_train_stats.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types
from collections import deque

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from cim_amd import _lib, mask_iou, synthetic  # noqa: E402
from cim_amd.core.config import cfg  # noqa: E402
from cim_amd.core.presets import apply_preset  # noqa: E402
from cim_amd.modeling import heads  # noqa: E402
from cim_amd.modeling.model_builder import Generalized_RCNN  # noqa: E402
from cim_amd.nn import DataParallel  # noqa: E402
from cim_amd.utils.training_stats import TrainingStats  # noqa: E402

CONFIG = "resnet50_voc"
LOG_PERIOD, WINDOW = 20, 20
VARIANTS = ("A", "B", "Bprime", "C")


class ReferenceStats:
    """Variant A: UpdateIterStats / LogIterStats of the reference, restated (SmoothedValue: lib/utils/logging.py:60-85)."""

    def __init__(self, iter_size):
        self.iter_size, self.inner, self.smoothed = iter_size, {}, {}

    def _add(self, k, v):
        self.smoothed.setdefault(k, deque(maxlen=WINDOW)).append(v)

    def update(self, out, inner):
        total = 0
        for k, loss in out["losses"].items():
            assert loss.shape[0] == cfg.NUM_GPUS
            loss = loss.mean(dim=0, keepdim=True)
            total = total + loss
            out["losses"][k] = loss
            if self.iter_size == 1:
                self._add(k, loss.data[0].cpu())
            else:
                self.inner.setdefault(k, []).append(loss.data[0])
                if inner == self.iter_size - 1:
                    self._add(k, (sum(self.inner.pop(k)) / self.iter_size).cpu())
        out["total_loss"] = total
        if self.iter_size == 1:
            self._add("total_loss", total.data[0].cpu())
        else:
            self.inner.setdefault("total_loss", []).append(total.data[0])
            if inner == self.iter_size - 1:
                self._add("total_loss", (sum(self.inner.pop("total_loss")) / self.iter_size).cpu())

    def log(self, step, lr):
        if step % LOG_PERIOD == 0:
            print("loss: %.6f, lr: %.6f" % (np.median(self.smoothed["total_loss"]), lr))
            print(", ".join("%s: %.6f" % (k, np.median(v)) for k, v in self.smoothed.items() if k != "total_loss"))

    def flush(self):
        pass


class NewStats:
    def __init__(self, iter_size, deferred):
        args = types.SimpleNamespace(iter_size=iter_size, run_name="bench_train_stats", cfg_filename=CONFIG)
        self.ts = TrainingStats(args, log_period=LOG_PERIOD, deferred=deferred, window=WINDOW)

    def update(self, out, inner):
        self.ts.UpdateIterStats(out, inner)

    def log(self, step, lr):
        self.ts.LogIterStats(step, lr)

    def flush(self):
        self.ts.flush()


class NoStats:
    def update(self, out, inner):
        pass

    def log(self, step, lr):
        pass

    def flush(self):
        pass


def setup(dev):
    """bench.py's model, optimizer and resident image cycle (bench.run, lines up to the timed region)."""
    apply_preset(CONFIG)
    torch.manual_seed(cfg.RNG_SEED)
    model = Generalized_RCNN()
    bench.init_for_synthetic(model)
    model = model.to(dev).train()
    dp = DataParallel(model, cpu_keywords=["im_info", "roidb"], minibatch=True)
    opt = bench.make_optimizer(model, torch)
    opt.overlap_update = False
    base_n, base_t = synthetic.CONFIGS[CONFIG]["n"], synthetic.CONFIGS[CONFIG]["target"]
    dev_batches = []
    for j, (n, t) in enumerate(bench.IMAGE_MIX):
        inp = synthetic.make_image_inputs(CONFIG, seed=cfg.RNG_SEED + j, n=int(round(n * base_n / 1000.0)),
                                          target=int(round(t * base_t / 688.0)))
        iou, asy = mask_iou.mask_iou_maps(torch.from_numpy(inp["full_masks"]).to(dev))
        one = lambda a: torch.from_numpy(a).unsqueeze(0)        # noqa: E731
        b = dict(data=torch.from_numpy(inp["data"]), rois=one(inp["rois"]), masks=one(inp["masks"]), labels=one(inp["labels"]),
                 mat=one(inp["mat"]), index=one(inp["index"]))
        dev_batches.append(dict({k: v.to(dev) for k, v in b.items()}, iou_map=iou, asy_iou_map=asy))
    torch.cuda.synchronize()
    np.random.seed(cfg.RNG_SEED)
    return model, dp, opt, dev_batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="optimizer steps per window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=24, help="optimizer steps before the first window of an iter_size")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.load()
    heads.LAZY_SETTLE = False
    model, dp, opt, dev_batches = setup(dev)
    cfg.SOLVER.MAX_ITER = 10 ** 9
    state = {"i": 0}
    log = io.StringIO()

    def run_steps(stats, n_steps, it):
        for step in range(n_steps):
            opt.zero_grad()
            for inner in range(it):
                j = state["i"] % len(dev_batches)
                state["i"] += 1
                out = dp(**{k: [v] for k, v in dev_batches[j].items()}, gtrois=[None])
                stats.update(out, inner)
                loss = out["total_loss"]
                loss.backward(retain_graph=True)
            opt.step()
            stats.log(step, 0.0005)
        return loss

    def make(name, it):
        return {"A": lambda: ReferenceStats(it), "B": lambda: NewStats(it, False), "Bprime": lambda: NewStats(it, True),
                "C": NoStats}[name]()

    res = dict(config=CONFIG, steps_per_window=args.steps, rounds=args.rounds, log_period=LOG_PERIOD, device=torch.cuda.get_device_name(0),
               torch=torch.__version__)
    with contextlib.redirect_stdout(log):
        for it in (1, 4):
            dp.iter_size = it
            trackers = {name: make(name, it) for name in VARIANTS}
            for name in VARIANTS:                                   # warm-up: every variant's own buffers and shapes
                run_steps(trackers[name], max(1, args.warmup // len(VARIANTS)), it)
                trackers[name].flush()
            times = {name: [] for name in VARIANTS}
            for _ in range(args.rounds):
                for name in VARIANTS:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loss = run_steps(trackers[name], args.steps, it)
                    torch.cuda.synchronize()
                    el = time.perf_counter() - t0
                    trackers[name].flush()                          # (Bprime's queued records: after the window's clock stopped)
                    assert torch.isfinite(loss).all()
                    times[name].append(1e3 * el / (args.steps * it))
            rec = {name: dict(ms_per_image=[round(t, 4) for t in ts], median=round(float(np.median(ts)), 4),
                              spread=round(max(ts) - min(ts), 4)) for name, ts in times.items()}
            rec["Bprime_minus_C"] = round(rec["Bprime"]["median"] - rec["C"]["median"], 4)
            rec["Bprime_minus_C_within_C_spread"] = bool(abs(rec["Bprime_minus_C"]) <= rec["C"]["spread"])
            rec["B_minus_A"] = round(rec["B"]["median"] - rec["A"]["median"], 4)
            rec["B_not_slower_than_A"] = bool(rec["B"]["median"] <= rec["A"]["median"])
            res["iter_size_%d" % it] = rec
    res["log_lines_printed"] = log.getvalue().count("\n")
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
