#!/usr/bin/env python3
"""Device time of one image's post-processing with TEST.SOFT_NMS / TEST.BBOX_VOTE (cim_amd.detect.postprocess: soft-NMS or
greedy NMS, box voting, limit), on seeded inputs shaped like the refinement heads' scores, beside the host time of the
NumPy restatement of the compiled reference (tests/golden/softvote_np.py).

    python tools/bench_detect_soft.py [--sizes 1000x20,1000x80,2000x20,2000x80,8192x20,8192x80] [--seconds 0.2]
                                      [--host-classes 2]

Warm-up first, then HIP events around back-to-back repeats on one stream for at least --seconds; prints one JSON line per
(size, NMS kind, voting) in milliseconds per image.  The host restatement runs on the first --host-classes classes and is
reported per class (C = 20 and N <= 2000 only: it takes seconds per class beyond; 0: skip it).  The last line is the worst
case of the soft-NMS kernel: linear on a disjoint grid of 8192 boxes, where nothing decays and nothing is removed - 8192
selection steps in one workgroup per class.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import softvote_np  # noqa: E402
from bench_detect import inputs, timed  # noqa: E402
from cim_amd import build, detect  # noqa: E402

KERNELS = ("softvote_soft_nms_kernel", "detect_overlap_kernel", "detect_nms_kernel", "softvote_from_keep_kernel",
           "softvote_vote_kernel", "softvote_limit_kernel")
KINDS = (None, "hard", "linear", "gaussian")                          # None: the greedy pass


def host_ms_per_class(scores, boxes, kind, vote, classes):
    if classes <= 0:
        return None
    s = scores[:, :classes].cpu().numpy()
    t = time.perf_counter()
    softvote_np.postprocess(s, boxes.cpu().numpy(), 1e-5, 0.3, 0, soft=None if kind is None else (kind, 0.5),
                            vote=(0.8, "AVG", 1.0) if vote else None)
    return (time.perf_counter() - t) * 1000 / s.shape[1]


def run(s, b, kind, vote, seconds, host_classes, label):
    soft = None if kind is None else dict(method=kind, sigma=0.5)
    bv = dict(thresh=0.8, scoring_method="AVG") if vote else None
    fn = lambda: detect.postprocess(s, b, 1e-5, 0.3, 100, soft_nms=soft, box_vote=bv)          # noqa: E731
    ms, reps = timed(fn, seconds)
    count = detect.softvote_to_host(fn())[3]
    host = host_ms_per_class(s, b, kind, vote, host_classes)
    print(json.dumps({"case": label, "N": s.shape[0], "C": s.shape[1], "nms": kind or "greedy", "vote": bool(vote),
                      "device_ms": round(ms, 4), "repeats": reps, "kept": int(count.sum()),
                      "host_restatement_ms_per_class": None if host is None else round(host, 2),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x20,1000x80,2000x20,2000x80,8192x20,8192x80")
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--host-classes", type=int, default=2)
    args = ap.parse_args()
    build.build()
    print("kernels:", ", ".join(KERNELS))
    for size in args.sizes.split(","):
        n, c = (int(v) for v in size.split("x"))
        s, b = inputs(n, c)
        for kind in KINDS:
            for vote in (False, True):
                if kind is None and not vote:
                    continue                                           # plain greedy NMS: tools/bench_detect.py
                run(s, b, kind, vote, args.seconds, args.host_classes if c == 20 and n <= 2000 else 0, "heads")
    n = 8192
    k = np.arange(n)
    grid = np.stack([(k % 128) * 20.0, (k // 128) * 20.0, (k % 128) * 20.0 + 9, (k // 128) * 20.0 + 9], 1).astype(np.float32)
    sc = np.random.RandomState(0).uniform(0.01, 1, (n, 2)).astype(np.float32)
    run(torch.from_numpy(sc).cuda(), torch.from_numpy(grid).cuda(), "linear", False, args.seconds, args.host_classes,
        "worst case: linear, disjoint grid")


if __name__ == "__main__":
    main()
