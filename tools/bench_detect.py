#!/usr/bin/env python3
"""Device time of one image's detection post-processing (cim_amd.detect.nms_limit: overlap matrix, per-class NMS, limit),
and of CorLoc's argmax, on seeded inputs shaped like the refinement heads' scores.

    python tools/bench_detect.py [--sizes 1000x20,2000x80] [--seconds 0.5]

Warm-up first, then HIP events around back-to-back repeats on one stream for at least --seconds; prints one JSON line per
size (milliseconds per image).  The launches' kernel names are printed so that a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_detect.py` run gives the split between them.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cim_amd import build, detect  # noqa: E402

KERNELS = ("detect_overlap_kernel", "detect_nms_kernel", "detect_limit_kernel", "detect_corloc_kernel")


def inputs(n, c, seed=0):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(0, 800, n), rng.uniform(0, 600, n)
    w, h = rng.uniform(8, 400, n), rng.uniform(8, 300, n)
    boxes = np.floor(np.stack([x1, y1, x1 + w, y1 + h], 1)).astype(np.float32)
    logits = rng.randn(n, c) * 3
    e = np.exp(logits - logits.max(1, keepdims=True))
    scores = (e / e.sum(1, keepdims=True) / (1 + np.exp(-rng.randn(n, c) * 2))).astype(np.float32)
    return torch.from_numpy(scores).cuda(), torch.from_numpy(boxes).cuda()


def timed(fn, seconds):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    reps, total_ms = 16, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total_ms = a.elapsed_time(b)
        if total_ms >= seconds * 1000:
            return total_ms / reps, reps
        reps *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x20,2000x80")
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    build.build()
    print("kernels:", ", ".join(KERNELS))
    for size in args.sizes.split(","):
        n, c = (int(v) for v in size.split("x"))
        s, b = inputs(n, c)
        ms, reps = timed(lambda: detect.nms_limit(s, b, 1e-5, 0.3, 100), args.seconds)
        ms_c, _ = timed(lambda: detect.corloc(s), args.seconds)
        kept = int(detect.to_host(detect.nms_limit(s, b, 1e-5, 0.3, 100))[3].sum())
        print(json.dumps({"N": n, "C": c, "nms_limit_ms": round(ms, 4), "corloc_ms": round(ms_c, 4), "repeats": reps,
                          "kept": kept, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
