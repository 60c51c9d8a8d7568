#!/usr/bin/env python3
"""Time of the device box evaluators (cim_amd.box_eval) against the NumPy restatement on the host
(tests/golden/box_eval_np.py, one CPU thread), at two sizes:

  voc   VocBoxEvaluator: 1449 images x 20 classes x <= 100 detections per image - add_image (the text round trip and the
        host staging), evaluate (one match launch, the sort rounds and the AP kernel) and corloc;
  coco  BoxEvaluator: 5000 images x 80 categories, crowd ground truths - add_image per image and accumulate.

    python tools/bench_box_eval.py [--voc 1449] [--coco 5000] [--pool 24] [--ref-images 60]

Images cycle through a pool of --pool seeded synthetic images, each added under its own id.  Device times: a host clock
around the whole phase, closed by a device synchronise, after a warm-up evaluator.  The restatement runs --ref-images images
and is compared bit for bit at that size (the area AP within its summation bound).  Prints one JSON line per size.
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

from cim_amd import box_eval, build  # noqa: E402


def pool_images(n, cats, size, crowd, seed):
    """Per image: 1-7 ground truths (integer xyxy, 0-based), 20-100 detections (jittered ground truths and stray boxes,
    quarter-pixel fp32 xyxy), scores on 1000 levels."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        g = int(rs.randint(1, 8))
        xy = rs.randint(0, size - 120, (g, 2))
        wh = rs.randint(16, 120, (g, 2))
        gt = np.hstack([xy, xy + wh - 1]).astype(np.float64)
        d = int(rs.randint(20, 101))
        src = rs.randint(0, g, d)
        det = gt[src] + np.round(rs.uniform(-0.25, 0.25, (d, 4)) * wh[src].repeat(2, 0).reshape(d, 4)[:, [0, 1, 0, 1]] * 4) / 4
        stray = rs.rand(d) < 0.3
        sxy, swh = rs.uniform(0, size - 100, (d, 2)), rs.uniform(8, 100, (d, 2))
        det[stray] = np.round(np.hstack([sxy, sxy + swh])[stray] * 4) / 4
        gcat = rs.randint(1, cats + 1, g)
        dcat = np.where(stray, rs.randint(1, cats + 1, d), gcat[src])
        out.append(dict(gt=gt, gcat=gcat, crowd=(rs.rand(g) < crowd).astype(int), diff=(rs.rand(g) < 0.15).astype(int),
                        det=np.clip(det, 0, size - 1).astype(np.float32), dcat=dcat,
                        score=(rs.randint(1, 1001, d) / 1000.0).astype(np.float32)))
    return out


# ---- VOC -------------------------------------------------------------------------------------------------------------------------
def voc_dets(d, K):
    return [np.hstack([d["det"][d["dcat"] == k + 1], d["score"][d["dcat"] == k + 1, None]]) for k in range(K)]


def run_voc_device(pool, n, K, use_07):
    ev = box_eval.VocBoxEvaluator(["c%d" % k for k in range(K)], use_07_metric=use_07)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        d = pool[i % len(pool)]
        ev.add_image(i, d["gt"] + 1, d["gcat"] - 1, d["diff"], voc_dets(d, K))
    t1 = time.perf_counter()
    res = ev.evaluate()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    cl = ev.corloc()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return (t1 - t0) / n, t2 - t1, t3 - t2, res, cl


def run_voc_reference(pool, n, K):
    import box_eval_np as ben
    gt_img, dt_img = [], []
    for i in range(n):
        d = pool[i % len(pool)]
        gt_img += [i] * len(d["gcat"])
        dt_img += [i] * len(d["dcat"])
    P = [pool[i % len(pool)] for i in range(n)]
    dcls = np.concatenate([d["dcat"] - 1 for d in P])
    order = np.lexsort((np.arange(len(dcls)), np.asarray(dt_img), dcls))                 # class-major, image-minor: the files' order
    case = dict(classes=["c%d" % k for k in range(K)], imagenames=list(range(n)), gt_img=np.asarray(gt_img),
                gt_cls=np.concatenate([d["gcat"] - 1 for d in P]), gt_box=np.concatenate([d["gt"] + 1 for d in P]),
                gt_diff=np.concatenate([d["diff"] for d in P]), dt_img=np.asarray(dt_img)[order], dt_cls=dcls[order],
                dets=np.hstack([np.concatenate([d["det"] for d in P]), np.concatenate([d["score"] for d in P])[:, None]])[order])
    t0 = time.perf_counter()
    out = ben.voc_dataset_np(case)
    return time.perf_counter() - t0, out


def bench_voc(n, pool_n, ref_n):
    K = 20
    pool = pool_images(pool_n, K, 500, 0.0, 7)
    run_voc_device(pool, min(n, 2 * pool_n), K, True)                                   # warm-up
    add_s, eval_s, corloc_s, (res, mean_ap), (_, mean_cl) = run_voc_device(pool, n, K, True)
    m = min(ref_n, n)
    ref_s, ref = run_voc_reference(pool, m, K)
    _, _, _, (res_m, _), (cl_m, _) = run_voc_device(pool, m, K, True)
    _, _, _, (area_m, _), _ = run_voc_device(pool, m, K, False)
    same = True
    for k in range(K):
        a, b = ref["cls_off"][k], ref["cls_off"][k + 1]
        r, p, ap = res_m["c%d" % k]
        if b > a:
            same &= np.array_equal(r, ref["rec"][a:b], equal_nan=True) and np.array_equal(p, ref["prec"][a:b])
            same &= np.array_equal(ap, ref["ap07"][k]) and np.array_equal(cl_m["c%d" % k], ref["corloc"][k], equal_nan=True)
            same &= bool(abs(area_m["c%d" % k][2] - ref["ap"][k]) <= 2 * (b - a + 2) * 2.0 ** -53 or np.isnan(ref["ap"][k]))
    dets = sum(len(pool[i % pool_n]["dcat"]) for i in range(n))
    print(json.dumps({"shape": "voc", "images": n, "classes": K, "detections": dets, "add_image_ms_per_image": round(add_s * 1e3, 4),
                      "evaluate_ms": round(eval_s * 1e3, 3), "corloc_ms": round(corloc_s * 1e3, 3), "ref_images": m,
                      "ref_total_ms": round(ref_s * 1e3, 3), "identical_at_ref_size": bool(same),
                      "mean_ap07": round(mean_ap, 6), "mean_corloc": round(mean_cl, 6)}), flush=True)


# ---- COCO ------------------------------------------------------------------------------------------------------------------------
def xywh(b):
    b = np.asarray(b, np.float64)
    return np.hstack([b[:, :2], b[:, 2:] - b[:, :2] + 1])


def run_coco_device(pool, n, cats):
    ev = box_eval.BoxEvaluator(range(n), cats)
    dev = [torch.from_numpy(d["det"]).cuda() for d in pool]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        d = pool[i % len(pool)]
        g = xywh(d["gt"])
        ev.add_image(i, g, d["gcat"], d["crowd"], g[:, 2] * g[:, 3], np.arange(len(g)) + 10 * i + 1, dev[i % len(pool)], d["dcat"],
                     d["score"])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = ev.accumulate()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / n, t2 - t1, ev, res


def run_coco_reference(pool, n, cats):
    import box_eval_np as ben
    ev = ben.BoxEvalNp(list(range(n)), cats)
    t0 = time.perf_counter()
    for i in range(n):
        d = pool[i % len(pool)]
        g = xywh(d["gt"])
        ev.add_image(i, g, d["gcat"], d["crowd"], g[:, 2] * g[:, 3], np.arange(len(g)) + 10 * i + 1, xywh(d["det"]), d["dcat"],
                     d["score"])
    ev.evaluate()
    t1 = time.perf_counter()
    ev.accumulate()
    t2 = time.perf_counter()
    return (t1 - t0) / n, t2 - t1, ev


def bench_coco(n, pool_n, ref_n):
    cats = list(range(1, 81))
    pool = pool_images(pool_n, 80, 640, 0.1, 8)
    run_coco_device(pool, min(n, 2 * pool_n), cats)                                     # warm-up
    add_s, acc_s, ev, res = run_coco_device(pool, n, cats)
    m = min(ref_n, n)
    ref_add_s, ref_acc_s, ref = run_coco_reference(pool, m, cats)
    _, _, _, res_m = run_coco_device(pool, m, cats)
    same = all(np.array_equal(box_eval.to_host(res_m)[k].view(np.uint64), ref.eval[k].view(np.uint64))
               for k in ("precision", "recall", "scores"))
    dets = sum(len(pool[i % pool_n]["dcat"]) for i in range(n))
    print(json.dumps({"shape": "coco", "images": n, "categories": 80, "detections": dets,
                      "add_image_ms_per_image": round(add_s * 1e3, 4), "accumulate_ms": round(acc_s * 1e3, 3), "ref_images": m,
                      "ref_evaluate_ms_per_image": round(ref_add_s * 1e3, 3), "ref_accumulate_ms": round(ref_acc_s * 1e3, 3),
                      "bit_identical_at_ref_size": bool(same), "stats": [round(float(s), 6) for s in ev.summarize(res)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voc", type=int, default=1449)
    ap.add_argument("--coco", type=int, default=5000)
    ap.add_argument("--pool", type=int, default=24)
    ap.add_argument("--ref-images", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_eval: needs the GPU (no CPU timing is reported)")
    build.build()
    torch.set_num_threads(1)
    if args.voc > 0:
        bench_voc(args.voc, args.pool, args.ref_images)
    if args.coco > 0:
        bench_coco(args.coco, args.pool, args.ref_images)


if __name__ == "__main__":
    main()
