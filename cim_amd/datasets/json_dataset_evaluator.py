"""COCO box AP of lib/datasets/json_dataset_evaluator.py:38-151 on the device: COCOeval(gt, results, 'bbox') evaluate /
accumulate / summarize in cim_amd.box_eval on the small COCO reader of json_inference, without pycocotools.

`evaluate_boxes(gt_json, all_boxes_or_results_json)` takes the annotation file (a path or the loaded dict) and either the
reference's all_boxes (all_boxes[1 + k][i]: fp32 [n, 5] (x1, y1, x2, y2, score) of category k - the file's categories in
order - in image i of the sorted image ids, or an empty list) or a bbox results JSON (a path or the loaded list:
image_id, category_id, bbox [x, y, w, h], score).  Scores are compared in fp32, the precision all_boxes holds them in.
Unlike the reference's _log_detection_eval_metrics, which indexes the category axis by the class index that still counts
__background__ (so every line is the next category's AP and the last one fails), the per-category lines index categories
correctly.
"""
import json
import logging

import numpy as np

from .. import box_eval
from .json_inference import CocoJson

logger = logging.getLogger(__name__)


def _results_by_image(ds, results):
    """-> {image id: (xywh f64 [n, 4], category ids, scores f32)} from all_boxes or a results list."""
    by_img = {}
    if isinstance(results, str):
        with open(results) as f:
            results = json.load(f)
    if results and isinstance(results[0], dict):
        for r in results:
            by_img.setdefault(int(r["image_id"]), []).append(r)
        out = {}
        for img_id, rs in by_img.items():
            scores = np.asarray([float(r["score"]) for r in rs], np.float64)
            s32 = scores.astype(np.float32)
            if not np.array_equal(s32.astype(np.float64), scores):
                raise ValueError("image %d: a score that is not an fp32 value (the device evaluator compares fp32 scores)" % img_id)
            out[img_id] = (np.asarray([r["bbox"] for r in rs], np.float64).reshape(-1, 4), [int(r["category_id"]) for r in rs], s32)
        return out
    image_ids = sorted(ds.getImgIds())
    cat_ids = ds.getCatIds()
    parts = {}
    for k, cat_id in enumerate(cat_ids):
        if k + 1 >= len(results):
            break
        if len(results[k + 1]) != len(image_ids):
            raise ValueError("all_boxes[%d] has %d images, the annotation file %d" % (k + 1, len(results[k + 1]), len(image_ids)))
        for i, img_id in enumerate(image_ids):
            dets = results[k + 1][i]
            if isinstance(dets, list) and len(dets) == 0:
                continue
            d = box_eval._host_f32(dets, "all_boxes[%d][%d]" % (k + 1, i), 5)
            parts.setdefault(img_id, []).append((box_eval.xyxy_to_xywh64(d[:, :4]), [cat_id] * d.shape[0], d[:, 4]))
    return {i: (np.concatenate([p[0] for p in ps]), sum((p[1] for p in ps), []), np.concatenate([p[2] for p in ps]))
            for i, ps in parts.items()}


def evaluate_boxes(gt_json, all_boxes_or_results_json):
    """-> the BoxEvaluator after accumulate (`.eval`: host precision / recall / scores, `.stats`: the 12 summary numbers);
    logs the per-category AP at IoU 0.50:0.95, area all, maxDets 100, and the summary."""
    ds = gt_json if isinstance(gt_json, CocoJson) else CocoJson(gt_json)
    res = _results_by_image(ds, all_boxes_or_results_json)
    assert set(res) <= set(ds.getImgIds()), "Results do not correspond to current coco set"
    ev = box_eval.BoxEvaluator(ds.getImgIds(), ds.getCatIds())
    empty = (np.zeros((0, 4)), [], np.zeros(0, np.float32))
    for img_id in ev.img_ids:
        anns = ds.img_to_anns.get(img_id, [])
        boxes, cats, scores = res.get(img_id, empty)
        if not anns and not len(cats):
            continue
        ev._add_xywh(img_id, [a["bbox"] for a in anns], [a["category_id"] for a in anns], [a.get("iscrowd", 0) for a in anns],
                     [a["area"] for a in anns], [a["id"] for a in anns], boxes, cats, scores)      # (results are xywh already)
    ev.eval = box_eval.to_host(ev.accumulate())
    ev.stats = ev.summarize(ev.eval)
    _log_detection_eval_metrics(ds, ev)
    return ev


def _log_detection_eval_metrics(ds, ev):
    lo = int(np.argmin(np.abs(ev.iou_thrs - 0.5)))
    hi = int(np.argmin(np.abs(ev.iou_thrs - 0.95)))
    assert np.isclose(ev.iou_thrs[lo], 0.5) and np.isclose(ev.iou_thrs[hi], 0.95)
    m = ev.max_dets.index(100) if 100 in ev.max_dets else len(ev.max_dets) - 1
    precision = ev.eval["precision"][lo:hi + 1, :, :, 0, m]
    mean = lambda p: float(np.mean(p[p > -1])) if (p > -1).any() else float("nan")
    logger.info("~~~~ Mean and per-category AP @ IoU=[%.2f,%.2f] ~~~~", 0.5, 0.95)
    logger.info("%.1f", 100 * mean(precision))
    ev.category_ap = {}
    for k, cat_id in enumerate(ev.cat_ids):                              # category k of the axis, no __background__ offset
        ev.category_ap[cat_id] = mean(precision[:, :, k])
        logger.info("%s: %.1f", ds.cats[cat_id].get("name", cat_id) if cat_id in ds.cats else cat_id, 100 * ev.category_ap[cat_id])
    logger.info("~~~~ Summary metrics ~~~~")
    for name, v in zip(("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"), ev.stats):
        logger.info("%-5s %.3f", name, v)
