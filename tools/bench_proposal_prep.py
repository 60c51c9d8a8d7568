#!/usr/bin/env python3
"""Training inputs from raw proposal masks (cim_amd.proposal_prep) at cfg2 and cfg4 sizes: HIP-event ms per
image of `prepare` alone, `assign_clusters` alone (P = 6 and 12), and prepare + maps() + assign_clusters, warm, median of
--repeats; beside them, in the same run on the same device, the existing pack_masks + maps_from_packed pair that
prepare + maps() replaces, and the NumPy restatement on the host (the stated baseline, never credited as a speed-up).
Bytes are what each stage has to move: the byte masks once (pack), the packed words once per later stage.

    python tools/bench_proposal_prep.py [--repeats 20] [--no-host]"""
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
from cim_amd import mask_iou, proposal_prep, synthetic  # noqa: E402

HBM_GBS = 8000.0


def median_ms(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def points_for(masks, p, classes, rng):
    n = masks.shape[0]
    rows, cols = [], []
    for _ in range(p):
        ys, xs = np.nonzero(masks[rng.randint(0, n)])
        k = rng.randint(0, ys.size)
        rows.append(int(ys[k])), cols.append(int(xs[k]))
    return rows, cols, [int(c) for c in rng.randint(0, classes, size=p)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy restatement's timing")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for cfgname in ("resnet50_voc", "resnet50_coco2017"):
        inp = synthetic.make_image_inputs(cfgname, seed=3, with_image=False)
        full = inp["full_masks"]
        classes = synthetic.CONFIGS[cfgname]["classes"]
        masks = torch.from_numpy(full).to(dev)
        n, h, w = masks.shape
        hw = h * w
        words = (hw + 63) // 64
        packed_bytes = n * words * 8
        rec = dict(config=cfgname, N=n, H=h, W=w, repeats=args.repeats)
        prep = proposal_prep.prepare(masks)

        def put(key, fn, nbytes):
            med, lo, hi = median_ms(fn, args.repeats)
            rec[key + "_ms"] = round(med, 4)
            rec[key + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
            rec[key + "_bytes"] = int(nbytes)
            rec[key + "_hbm_frac_of_8TBs"] = round(nbytes / med / 1e6 / HBM_GBS, 4)

        # pack: bytes in + words out; extents: words in; resize: 49 words per proposal (noise)
        put("prepare", lambda: proposal_prep.prepare(masks), n * hw + 2 * packed_bytes)
        put("pack_masks", lambda: mask_iou.pack_masks(masks), n * hw + packed_bytes)
        put("maps_from_packed", lambda: mask_iou.maps_from_packed(prep.packed), 2 * packed_bytes + 4 * n * n)
        put("pack_plus_maps_existing", lambda: mask_iou.maps_from_packed(mask_iou.pack_masks(masks)), n * hw + 3 * packed_bytes + 4 * n * n)
        put("prepare_plus_maps", lambda: proposal_prep.prepare(masks).maps(), n * hw + 4 * packed_bytes + 4 * n * n)
        for p in (6, 12):
            rows, cols, cls = points_for(full, p, classes, np.random.RandomState(11))
            # average masks: the words once per 4 points (neighbouring waves share a column) + the points' columns;
            # intersections: the words once per 8 points
            nbytes = packed_bytes * ((p + 3) // 4) + packed_bytes * ((p + 7) // 8) + 2 * words * p * 8 + 4 * n * (classes + 1)
            put("assign_P%d" % p, lambda: proposal_prep.assign_clusters(prep, rows, cols, cls, classes), nbytes)
            put("all_P%d" % p, lambda: (lambda q: (q.maps(), proposal_prep.assign_clusters(q, rows, cols, cls, classes)))(
                proposal_prep.prepare(masks)), n * hw + 4 * packed_bytes + 4 * n * n + nbytes)
            if not args.no_host and p == 6:
                import proposal_prep_np as ppn
                t0 = time.perf_counter()
                ppn.boxes_and_small(full)
                t1 = time.perf_counter()
                ppn.assign_clusters(full, rows, cols, cls, classes)
                t2 = time.perf_counter()
                rec["host_numpy_boxes_small_ms"] = round((t1 - t0) * 1e3, 1)
                rec["host_numpy_assign_P6_ms"] = round((t2 - t1) * 1e3, 1)
        rec["prepare_plus_maps_minus_existing_ms"] = round(rec["prepare_plus_maps_ms"] - rec["pack_plus_maps_existing_ms"], 4)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
