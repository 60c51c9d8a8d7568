#!/usr/bin/env python3
"""Time of the device instance-segmentation evaluator (cim_amd.segm_eval): add_image per image (packing of the proposal
masks, IoU, sort, matching) and accumulate (gather, merge rounds, precision / recall), at VOC-val size (1449 images of
375 x 500, 20 categories) and at a COCO-val shape (5000 images of 480 x 640, 80 categories, crowd ground truths), against
the NumPy restatement of pycocotools (tests/golden/segm_eval_np.py) on one CPU thread.

    python tools/bench_segm_eval.py [--voc 1449] [--coco 5000] [--pool 24] [--ref-images 60]

The images cycle through a pool of --pool seeded synthetic images (cim_amd.synthetic.make_segm_image; up to 100
detections per image) kept on the device, each added under its own image id.  Device times: a host clock around the
whole loop, closed by a device synchronise, after a warm-up evaluator.  The restatement runs --ref-images images
(computeIoU + evaluateImg per image) and its accumulate at that size; its per-image time is what the reference's
evaluation pays per image in one process.  Prints one JSON line per shape.
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

from cim_amd import build, segm_eval, synthetic  # noqa: E402

SHAPES = {"voc": (375, 500, 20, 0.0, 0), "coco": (480, 640, 80, 0.1, 64)}


def pool_images(shape, n, seed):
    h, w, cats, crowd, levels = SHAPES[shape]
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        n_gt = int(rs.randint(1, 8))
        d = synthetic.make_segm_image(rs, h, w, cats, n_gt, n_gt + 40, int(rs.randint(20, 101)), crowd, levels)
        d["gt_ids"] = np.arange(n_gt) + 100 * i
        d["dev"] = torch.from_numpy(d["masks"]).cuda()
        out.append(d)
    return out


def run_device(pool, n, cats):
    ev = segm_eval.SegmEvaluator(range(n), cats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        d = pool[i % len(pool)]
        g = len(d["gt_cat"])
        ev.add_image(i, d["dev"][:g], d["gt_cat"], d["gt_crowd"], d["gt_area"], d["gt_ids"], (d["dev"], d["dt_idx"]),
                     d["dt_cat"], d["dt_score"])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = ev.accumulate()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    dets = sum(len(pool[i % len(pool)]["dt_idx"]) for i in range(n))
    return (t1 - t0) / n, t2 - t1, dets, ev, res


def run_reference(pool, n, cats):
    import segm_eval_np as sen
    ev = sen.SegmEvalNp(list(range(n)), cats)
    t0 = time.perf_counter()
    for i in range(n):
        d = pool[i % len(pool)]
        g = len(d["gt_cat"])
        ev.add_image(i, d["masks"][:g], d["gt_cat"], d["gt_crowd"], d["gt_area"], d["gt_ids"], d["masks"][d["dt_idx"]],
                     d["dt_cat"], d["dt_score"])
    ev.evaluate()
    t1 = time.perf_counter()
    ev.accumulate()
    t2 = time.perf_counter()
    return (t1 - t0) / n, t2 - t1, ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voc", type=int, default=1449)
    ap.add_argument("--coco", type=int, default=5000)
    ap.add_argument("--pool", type=int, default=24)
    ap.add_argument("--ref-images", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segm_eval: needs the GPU (no CPU timing is reported)")
    build.build()
    torch.set_num_threads(1)
    for shape, n in (("voc", args.voc), ("coco", args.coco)):
        if n <= 0:
            continue
        cats = list(range(1, SHAPES[shape][2] + 1))
        pool = pool_images(shape, args.pool, 7)
        run_device(pool, min(n, 2 * args.pool), cats)                  # warm-up
        add_s, acc_s, dets, ev, res = run_device(pool, n, cats)
        m = min(args.ref_images, n)
        ref_add_s, ref_acc_s, ref = run_reference(pool, m, cats)
        # the same images at the restatement's size: the device agrees bit for bit
        _, _, _, ev_m, res_m = run_device(pool, m, cats)
        same = all(np.array_equal(segm_eval.to_host(res_m)[k].view(np.uint64), ref.eval[k].view(np.uint64))
                   for k in ("precision", "recall", "scores"))
        print(json.dumps({"shape": shape, "images": n, "detections": dets, "add_image_ms_per_image": round(add_s * 1e3, 4),
                          "accumulate_ms": round(acc_s * 1e3, 3), "ref_images": m,
                          "ref_evaluate_ms_per_image": round(ref_add_s * 1e3, 3), "ref_accumulate_ms": round(ref_acc_s * 1e3, 3),
                          "bit_identical_at_ref_size": bool(same), "stats": [round(float(s), 6) for s in ev.summarize(res)]}),
              flush=True)


if __name__ == "__main__":
    main()
