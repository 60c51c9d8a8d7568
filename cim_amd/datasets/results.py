"""The reference's two dataset-level post-processing loops on the device:

  instance_predictions   tools/evaluation.py:72-138 - detections + proposal masks -> the instance predictions that
                         coco_inst_seg_eval scores;
  pseudo_labels          tools/generate_mask_for_MaskRCNN.py:79-190 with lib/datasets/pycococreatortools.py
                         create_image_info / create_annotation_info_v1 - detections + proposal masks + image-level labels ->
                         the COCO-format pseudo-label file stage 2 (Mask R-CNN) trains on.

Both walk the roidb in order, `images_per_call` images per batched detection call (cim_amd.detect.nms_limit_batch: score
threshold, per-class NMS, the limit over all classes, the proposal index), then encode each image's selected masks
(cim_amd.segm_eval.pack_masks / rle_counts; the compressed string by cim_amd.utils.rle).  No multiprocessing: the
reference's 24 processes split the roidb and concatenate in roidb order, which is the order here.  SCORE_THRESH and NMS come
from cfg.TEST as in the reference, the limit from the argument.  Scores and boxes are NumPy arrays or device tensors, masks
[N, H, W] bool / uint8 NumPy arrays or device tensors; CPU tensors are refused (no CPU fallback).

Deliberate differences from the reference: a mask whose shape is not the entry's (height, width) is refused
(NotImplementedError; the reference's create_annotation_info_v1 would PIL-resize it - COB masks are at image size, and
json_inference.coco_encode refuses alike); a zero-area mask consumes an annotation id but is not appended (the reference
appends None); `date_captured` is the entry's, or "" (the reference stamps its import time).
"""
import os

import numpy as np
import torch

from .. import detect, segm_eval
from ..core import test as _test
from ..core.config import cfg
from ..utils import rle as _rle


def _class_columns(num_classes):
    num_classes = int(num_classes)
    if num_classes < 1:
        raise ValueError("results: num_classes must be >= 1, got %d" % num_classes)
    return num_classes


def _blocks(all_boxes, roidb, num_classes, max_det, images_per_call, area_bounds=None, class_mask=None):
    """Per block of the roidb: (entries, per-image record slices (idx, cls, score)) of one batched detection call."""
    _test._post_check(cfg)
    thr, nms = _test._post_cfg(cfg, "SCORE_THRESH"), _test._post_cfg(cfg, "NMS")
    for i0 in range(0, len(roidb), int(images_per_call)):
        entries = roidb[i0:i0 + int(images_per_call)]
        dets = [all_boxes[e["image"]] for e in entries]
        image, idx, cls, sc, _ = detect.nms_limit_batch(
            [d["scores"] for d in dets], [d["boxes"] for d in dets], thr, nms, max_det, num_classes=num_classes,
            area_bounds=None if area_bounds is None else area_bounds[i0:i0 + len(entries)],
            class_mask=None if class_mask is None else class_mask[i0:i0 + len(entries)])
        cut = np.searchsorted(image, np.arange(len(entries) + 1))
        yield entries, [(idx[cut[k]:cut[k + 1]], cls[cut[k]:cut[k + 1]], sc[cut[k]:cut[k + 1]]) for k in range(len(entries))]


def _selected_counts(masks, idx, entry):
    """Run counts of masks[idx] (host uint32, offsets [len(idx) + 1]); the masks must be [N, height, width] of the entry."""
    shape = tuple(int(s) for s in masks.shape)
    h, w = int(entry["height"]), int(entry["width"])
    if len(shape) != 3 or shape[1:] != (h, w):
        raise NotImplementedError("results: image %s: masks of shape %s, the image is %d x %d - resizing masks is not supported"
                                  % (entry.get("id", "?"), shape, h, w))
    if len(idx) == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64)
    if torch.is_tensor(masks):
        packed = segm_eval.pack_masks(masks, idx)                        # (a CPU tensor is refused there)
    else:
        a = np.asarray(masks)
        if a.dtype != np.bool_ and a.dtype != np.uint8:
            raise TypeError("results: masks must be bool or uint8, got %s" % a.dtype)
        sel = np.ascontiguousarray(a[idx]).view(np.uint8)
        packed = segm_eval.pack_masks(torch.from_numpy(sel).to(torch.device("cuda", torch.cuda.current_device())))
    return segm_eval.rle_counts(packed, h, w)


def _category(cls, category_ids):
    return int(cls) + 1 if category_ids is None else category_ids[int(cls)]


def instance_predictions(all_boxes, roidb, masks_of, num_classes, category_ids=None, proposal_filter=False, max_det=100,
                         images_per_call=256):
    """tools/evaluation.py:72-138.  all_boxes[entry['image']] = {'scores' [N, >= num_classes] f32, 'boxes' [N, 4]};
    masks_of(entry) -> that image's [N, H, W] proposal masks.  Returns the list of dict(image_id, score, category_id,
    segmentation={'size': [h, w], 'counts': str}) - per image the classes 1..num_classes in order, instances in ascending
    proposal order.  category_id is the class index (1-based) or category_ids[cls - 1] (coco_nummap_id).  proposal_filter:
    TEST.PROPOSAL_FILTER with the reference's limits (0.00002, 0.85) of the image area."""
    C = _class_columns(num_classes)
    bounds = None
    if proposal_filter:
        area = np.array([e["height"] * e["width"] for e in roidb], dtype=np.float64)
        bounds = np.stack([(0.00002 * area).astype(np.float32), (0.85 * area).astype(np.float32)], 1).reshape(-1, 2)
    predictions = []
    for entries, records in _blocks(all_boxes, roidb, C, max_det, images_per_call, area_bounds=bounds):
        for entry, (idx, cls, sc) in zip(entries, records):
            counts, off = _selected_counts(masks_of(entry), idx, entry)
            size = [int(entry["height"]), int(entry["width"])]
            for k in range(len(idx)):
                predictions.append(dict(image_id=int(entry["id"]), score=float(sc[k]), category_id=_category(cls[k], category_ids),
                                        segmentation={"size": list(size), "counts": _rle.counts_to_string(counts[off[k]:off[k + 1]])}))
    return predictions


def rle_area_bbox(counts, h):
    """pycocotools' area and rleToBbox of one run-count array (column-major runs, height h): (area, [x, y, w, h]) as ints."""
    c = np.asarray(counts, dtype=np.int64)
    area = int(c[1::2].sum())
    m = c.size // 2 * 2
    if m == 0:
        return area, [0, 0, 0, 0]
    t = np.cumsum(c[:m]) - (np.arange(m) & 1)                           # first pixel of each run of ones, then its last pixel
    y, x = t % h, t // h
    ys, ye = int(y.min()), int(y.max())
    if (x[0::2] < x[1::2]).any():                                        # a run that crosses a column boundary
        ys, ye = 0, h - 1
    xs, xe = int(x.min()), int(x.max())
    return area, [xs, ys, xe - xs + 1, ye - ys + 1]


def image_info(entry):
    """pycococreatortools.create_image_info's fields from a roidb entry."""
    return {"id": int(entry["id"]), "file_name": os.path.basename(entry["image"]), "width": int(entry["width"]),
            "height": int(entry["height"]), "date_captured": entry.get("date_captured", ""), "license": 1, "coco_url": "",
            "flickr_url": ""}


def pseudo_labels(all_boxes, roidb, masks_of, num_classes, categories, category_ids=None, is_best=False, max_det=100,
                  images_per_call=256):
    """tools/generate_mask_for_MaskRCNN.py:79-190.  Inputs as for instance_predictions; entry['gt_classes'][0][c] > 0 marks
    the image-level classes, applied after the limit over all classes.  Within a present class the instances are written by
    descending score, equal scores higher position first (np.argsort(kind="stable")[::-1], the tie rule of DESIGN.md 4.11);
    with is_best only those whose score equals the class's best.  Returns {'images', 'annotations', 'categories'}; annotation
    ids run from 1 in roidb order (what the reference's merge of its per-process files produces)."""
    C = _class_columns(num_classes)
    present = np.stack([np.asarray(e["gt_classes"][0])[:C] > 0 for e in roidb]).astype(np.uint8).reshape(-1, C) if len(roidb) else None
    out = {"images": [], "annotations": [], "categories": categories}
    instance_id = 1
    for entries, records in _blocks(all_boxes, roidb, C, max_det, images_per_call, class_mask=present):
        for entry, (idx, cls, sc) in zip(entries, records):
            counts, off = _selected_counts(masks_of(entry), idx, entry)
            h, w = int(entry["height"]), int(entry["width"])
            out["images"].append(image_info(entry))
            for c in np.unique(cls):                                     # ascending classes; absent ones have no records
                at = np.flatnonzero(cls == c)
                order = at[np.argsort(sc[at], kind="stable")[::-1]]
                best = sc[order[0]]
                for k in order:
                    if is_best and sc[k] != best:
                        continue
                    run = counts[off[k]:off[k + 1]]
                    area, bbox = rle_area_bbox(run, h)
                    ann_id = instance_id
                    instance_id += 1
                    if area < 1:
                        continue
                    out["annotations"].append({
                        "id": ann_id, "image_id": int(entry["id"]), "category_id": _category(c, category_ids), "iscrowd": 0,
                        "area": area, "bbox": bbox, "segmentation": {"counts": [int(v) for v in run], "size": [h, w]},
                        "width": w, "height": h, "score": float(sc[k])})
    return out
