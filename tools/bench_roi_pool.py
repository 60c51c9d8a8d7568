#!/usr/bin/env python3
"""Micro-benchmark of the four RoIPool kernels (csrc/roi_pool.hip) alone, next to the ROIAlign mask-cat
forward and backward of the same library at the same geometry: ms per launch and the bytes each launch must move.

    python tools/bench_roi_pool.py [--out profiles/roi_pool_bench.json] [--iters 20]

Geometries: resnet50_voc (1024 channels, 33 x 43 map, 1/16) with 800 and 1200 proposals, vgg16 (512 channels, 1/8) and hrnet
(2048 channels, 1/32) with 1200, P 7, seeded boxes on a 528 x 688 image.  One JSON line per geometry."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cim_amd import _lib  # noqa: E402

IMAGE_HW = (528, 688)
P = 7
GEOMETRIES = [("resnet50_voc", 1024, 16, 800), ("resnet50_voc", 1024, 16, 1200), ("vgg16", 512, 8, 1200), ("hrnet", 2048, 32, 1200)]


def boxes(k, seed=3):
    """k seeded proposals (batch 0) inside the image, 24 to 400 pixels a side - the spread of the synthetic proposals."""
    rs = np.random.RandomState(seed)
    h, w = IMAGE_HW
    bw, bh = rs.uniform(24, 400, k), rs.uniform(24, 400, k)
    x1, y1 = rs.uniform(0, w - bw), rs.uniform(0, h - bh)
    return np.stack([np.zeros(k), x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)


def timeit(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def words(nbytes, dev):
    return torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=dev)


def run(name, C, stride, K, iters, dev):
    H, W = -(-IMAGE_HW[0] // stride), -(-IMAGE_HW[1] // stride)
    scale, st = 1.0 / stride, _lib.stream_ptr()
    rois = torch.from_numpy(boxes(K)).to(dev)
    masks = (torch.rand(K, P, P, device=dev) > 0.4).float()
    feat = torch.randn(1, H, W, C, device=dev)
    out, cat = torch.empty(K, P, P, C, device=dev), torch.empty(K, P, P, 2 * C, device=dev)
    arg = torch.empty(K, P, P, C, dtype=torch.int32, device=dev)
    gout, gcat, gin = torch.randn(K, P, P, C, device=dev), torch.randn(K, P, P, 2 * C, device=dev), torch.empty(1, H, W, C, device=dev)
    scratch = words(_lib.call("cim_roi_pool_bwd_scratch", K, 1, C, H, W, P), dev)
    ws = words(_lib.call("cim_roi_align_bwd_workspace", K, P, H, W), dev)
    ascratch = words(_lib.call("cim_roi_align_bwd_scratch", K, 1, C, H, W), dev)
    p = lambda t: t.data_ptr()
    calls = {
        "pool_fwd": lambda: _lib.call("cim_roi_pool_fwd", p(feat), p(rois), p(out), p(arg), 1, C, H, W, K, P, scale, st),
        "pool_fwd_no_argmax": lambda: _lib.call("cim_roi_pool_fwd", p(feat), p(rois), p(out), None, 1, C, H, W, K, P, scale, st),
        "pool_maskcat_fwd": lambda: _lib.call("cim_roi_pool_maskcat_fwd", p(feat), p(rois), p(masks), p(cat), p(arg), 1, C, H, W, K, P, scale, st),
        "pool_bwd": lambda: _lib.call("cim_roi_pool_bwd", p(gout), p(rois), p(arg), p(gin), 1, C, H, W, K, P, scale, p(scratch), st),
        "pool_maskcat_bwd": lambda: _lib.call("cim_roi_pool_maskcat_bwd", p(gcat), p(rois), p(masks), p(arg), p(gin), 1, C, H, W, K, P, scale,
                                              p(scratch), st),
        "align_maskcat_fwd": lambda: _lib.call("cim_roi_align_maskcat_fwd_ws", p(feat), p(rois), p(masks), p(cat), 1, C, H, W, K, P, scale, 0, 1,
                                               p(ws), st),
        "align_maskcat_bwd": lambda: _lib.call("cim_roi_align_maskcat_bwd_ws", p(gcat), p(rois), p(masks), p(gin), 1, C, H, W, K, P, scale, 0, 1,
                                               p(ws), 0, p(ascratch), st),
    }
    fmap, bins, small = 4.0 * C * H * W, 4.0 * K * P * P * C, 4.0 * (5 * K + K * P * P)
    must_move = {                       # bytes a launch cannot avoid: every input read once, every output written once
        "pool_fwd": fmap + 2 * bins + small, "pool_fwd_no_argmax": fmap + bins + small, "pool_maskcat_fwd": fmap + 3 * bins + small,
        "pool_bwd": 2 * bins + fmap + small, "pool_maskcat_bwd": 3 * bins + fmap + small,
        "align_maskcat_fwd": fmap + 2 * bins + small, "align_maskcat_bwd": 2 * bins + fmap + small,
    }
    ms = {k: timeit(fn, iters) for k, fn in calls.items()}
    res = dict(geometry=name, C=C, H=H, W=W, K=K, P=P, scale=scale, iters=iters,
               pool_bwd_groups=max(1, _lib.call("cim_roi_pool_bwd_scratch", K, 1, C, H, W, P) // (4 * C * H * W)),
               ms={k: round(v, 4) for k, v in ms.items()}, must_move_MB={k: round(v / 1e6, 1) for k, v in must_move.items()},
               TB_per_s={k: round(must_move[k] / ms[k] / 1e9, 2) for k in ms},
               ratio_to_align={"maskcat_fwd": round(ms["pool_maskcat_fwd"] / ms["align_maskcat_fwd"], 2),
                               "maskcat_bwd": round(ms["pool_maskcat_bwd"] / ms["align_maskcat_bwd"], 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_roi_pool: needs the GPU (a time taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    results = [run(*g, args.iters, dev) for g in GEOMETRIES]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
