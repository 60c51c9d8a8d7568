#!/usr/bin/env python3
"""A results file's detection post-processing: ONE batched call (cim_amd.detect.nms_limit_batch) against the per-image path
it replaces, a loop of cim_amd.detect.nms_limit + to_host, on the same device inputs.

    python tools/bench_detect_batch.py [--cases 64x1000x20,64x2000x80] [--repeats 9]

Inputs are seeded and made the way tests/golden/make_golden_detect.py makes its large cases (softmax x sigmoid scores,
half integer / half quarter-pixel boxes), one draw per image, already on the device as inference leaves them.  Both arms end
with their records in host arrays, so each time includes its device-to-host copies and the waits they imply (a host clock
around work that ends synchronised).  Every shape is warmed up first; the arms then alternate `--repeats` times and the
median of each is reported with its spread, one JSON line per case.  The two arms' records are compared before timing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cim_amd import build, detect  # noqa: E402

F32 = np.float32


def make_boxes(rng, n, size=600.0):
    x1, y1 = rng.uniform(0, size * 0.8, n), rng.uniform(0, size * 0.8, n)
    w, h = rng.uniform(4, size * 0.5, n), rng.uniform(4, size * 0.5, n)
    b = np.stack([x1, y1, x1 + w, y1 + h], 1)
    half = n // 2
    b[:half] = np.floor(b[:half])
    b[half:] = np.round(b[half:] * 4) / 4
    return b.astype(F32)


def make_scores(rng, n, c):
    logits = rng.randn(n, c) * 3
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True) / (1 + np.exp(-rng.randn(n, c) * 2))).astype(F32)


def inputs(b, n, c, seed=20261018):
    rng = np.random.RandomState(seed)
    dev = torch.device("cuda", torch.cuda.current_device())
    scores = [torch.from_numpy(make_scores(rng, n, c)).to(dev) for _ in range(b)]
    boxes = [torch.from_numpy(make_boxes(rng, n)).to(dev) for _ in range(b)]
    return scores, boxes


def per_image(scores, boxes):
    return [detect.to_host(detect.nms_limit(s, b, 1e-5, 0.3, 100)) for s, b in zip(scores, boxes)]


def batched(scores, boxes):
    return detect.nms_limit_batch(scores, boxes, 1e-5, 0.3, 100)


def same(loop, batch):
    image, idx, cls, sc, count = batch
    for k, (i, c, s, n) in enumerate(loop):
        on = image == k
        if not (np.array_equal(idx[on], i) and np.array_equal(cls[on], c) and np.array_equal(sc[on].view(np.uint32), s.view(np.uint32))
                and np.array_equal(count[k], n)):
            return False
    return True


def clock(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64x1000x20,64x2000x80", help="BxNxC, comma separated")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_detect_batch needs the GPU (there is no CPU path to time)"
    build.build()
    for case in args.cases.split(","):
        b, n, c = (int(v) for v in case.split("x"))
        scores, boxes = inputs(b, n, c)
        ok = same(per_image(scores, boxes), batched(scores, boxes))
        for _ in range(2):                                              # warm-up of both arms at this shape
            per_image(scores, boxes)
            batched(scores, boxes)
        loop_ms, batch_ms = [], []
        for _ in range(args.repeats):                                   # alternate the arms
            loop_ms.append(clock(per_image, scores, boxes))
            batch_ms.append(clock(batched, scores, boxes))
        lm, bm = float(np.median(loop_ms)), float(np.median(batch_ms))
        print(json.dumps({"B": b, "N": n, "C": c, "records_equal": bool(ok), "per_image_loop_ms": round(lm, 3),
                          "batched_ms": round(bm, 3), "loop_over_batched": round(lm / bm, 2),
                          "loop_min_max_ms": [round(min(loop_ms), 3), round(max(loop_ms), 3)],
                          "batched_min_max_ms": [round(min(batch_ms), 3), round(max(batch_ms), 3)], "repeats": args.repeats,
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
