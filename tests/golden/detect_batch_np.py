"""NumPy restatement of the batched detection post-processing and of the two dataset-level drivers built on it
(cim_amd.detect.nms_limit_batch, cim_amd/datasets/results.py).  Paths are under the reference checkout.

Per image it is detect_np.nms_limit (pinned to the reference's goldens by tests/test_detect_cpu.py) plus
  - TEST.PROPOSAL_FILTER        tools/evaluation.py:108-115
  - the class mask AFTER the limit   tools/generate_mask_for_MaskRCNN.py:124-136
and the two record -> dict builders (tools/evaluation.py:119-134; generate_mask_for_MaskRCNN.py:127-190 with
lib/datasets/pycococreatortools.py:30-38, 67-81, 136-170).  The run lengths, areas and boxes here are plain NumPy on the
mask itself (not on run counts, as the product derives them); the compressed string is cim_amd.utils.rle.
"""
import os

import numpy as np

import detect_np
from cim_amd.utils import rle as rle_string

F32 = np.float32
SIZE_LIMIT = (0.00002, 0.85)                                          # evaluation.py:199 proposal_size_limit


def area_bounds(height, width):
    """evaluation.py:109-114: the two scalars the fp32 box areas are compared with (a Python float against an fp32 array
    compares in fp32)."""
    image_area = height * width
    return F32(SIZE_LIMIT[0] * image_area), F32(SIZE_LIMIT[1] * image_area)


def filter_scores(scores, boxes, bounds):
    """evaluation.py:108-115: scores[invalid] = 0 for area > hi, then for area < lo; fp32, no + 1, strict compares."""
    scores = np.array(scores, dtype=F32, copy=True)
    boxes = np.asarray(boxes, dtype=F32)
    lo, hi = F32(bounds[0]), F32(bounds[1])
    with np.errstate(invalid="ignore", over="ignore"):
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        scores[area > hi] = 0
        scores[area < lo] = 0
    return scores


def nms_limit_image(scores, boxes, score_thr, nms_thr, max_det, bounds=None, class_mask=None, mask_first=False):
    """One image: (idx, cls, score, count [C]).  class_mask [C] drops the records of absent classes after the limit
    (generate_mask_for_MaskRCNN.py:124-136); mask_first=True is the WRONG order (absent classes zeroed before the limit), kept
    so that a test can show the two differ."""
    scores = np.asarray(scores, dtype=F32)
    if bounds is not None:
        scores = filter_scores(scores, boxes, bounds)
    if class_mask is not None and mask_first:
        scores = np.where(np.asarray(class_mask)[None, :] > 0, scores, F32(0)).astype(F32)
    idx, cls, sc, count = detect_np.nms_limit(scores, boxes, score_thr, nms_thr, max_det)
    if class_mask is not None and not mask_first:
        on = np.asarray(class_mask)[cls] > 0
        idx, cls, sc = idx[on], cls[on], sc[on]
        count = np.where(np.asarray(class_mask) > 0, count, 0).astype(np.int32)
    return idx, cls, sc, count


def nms_limit_batch(scores, boxes, score_thr, nms_thr, max_det, area_bounds=None, class_mask=None):
    """Lists of per-image arrays -> (image, idx, cls, score, count [B, C]) in (image, class, proposal) order."""
    out = [nms_limit_image(s, b, score_thr, nms_thr, max_det, None if area_bounds is None else area_bounds[k],
                           None if class_mask is None else class_mask[k]) for k, (s, b) in enumerate(zip(scores, boxes))]
    image = np.concatenate([np.full(len(o[0]), k, np.int64) for k, o in enumerate(out)])
    return (image, np.concatenate([o[0] for o in out]).astype(np.int64), np.concatenate([o[1] for o in out]).astype(np.int32),
            np.concatenate([o[2] for o in out]).astype(F32), np.stack([o[3] for o in out]))


def run_lengths(mask):
    """pycococreatortools.py:30-38 (= pycocotools' rleEncode): the runs of mask.ravel(order='F'), a leading 0 when pixel
    (0, 0) is set."""
    flat = (np.asarray(mask).ravel(order="F") != 0).astype(np.int8)
    edges = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], edges, [flat.size]]))
    return ([0] if flat.size and flat[0] else []) + [int(r) for r in runs]


def bbox_of(mask):
    """pycocotools' toBbox of a mask = its tight box [x, y, w, h] (a run that crosses a column boundary spans the full
    height, which is then the tight extent too)."""
    ys, xs = np.nonzero(np.asarray(mask))
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def _category(c, category_ids):
    return int(c) + 1 if category_ids is None else category_ids[int(c)]


def instance_predictions(all_boxes, roidb, masks_of, num_classes, score_thr, nms_thr, category_ids=None,
                         proposal_filter=False, max_det=100):
    """evaluation.py:80-134."""
    preds = []
    for entry in roidb:
        d = all_boxes[entry["image"]]
        bounds = area_bounds(entry["height"], entry["width"]) if proposal_filter else None
        idx, cls, sc, _ = nms_limit_image(np.asarray(d["scores"])[:, :num_classes], d["boxes"], score_thr, nms_thr, max_det, bounds)
        masks = np.asarray(masks_of(entry))
        for p, c, s in zip(idx, cls, sc):                                # classes ascending, proposals ascending (:119-121)
            m = masks[p]
            preds.append(dict(image_id=int(entry["id"]), score=float(s), category_id=_category(c, category_ids),
                              segmentation={"size": [int(m.shape[0]), int(m.shape[1])],
                                            "counts": rle_string.counts_to_string(run_lengths(m))}))
    return preds


def pseudo_labels(all_boxes, roidb, masks_of, num_classes, score_thr, nms_thr, categories, category_ids=None, is_best=False,
                  max_det=100):
    """generate_mask_for_MaskRCNN.py:87-190; ids as its merge step leaves them (sequential over the roidb)."""
    out = {"images": [], "annotations": [], "categories": categories}
    instance_id = 1
    for entry in roidb:
        d = all_boxes[entry["image"]]
        present = np.asarray(entry["gt_classes"][0])[:num_classes] > 0
        idx, cls, sc, _ = nms_limit_image(np.asarray(d["scores"])[:, :num_classes], d["boxes"], score_thr, nms_thr, max_det,
                                          class_mask=present)
        masks = np.asarray(masks_of(entry))
        out["images"].append({"id": int(entry["id"]), "file_name": os.path.basename(entry["image"]),
                              "width": int(entry["width"]), "height": int(entry["height"]),
                              "date_captured": entry.get("date_captured", ""), "license": 1, "coco_url": "", "flickr_url": ""})
        for c in range(num_classes):                                     # :135-136
            if not present[c]:
                continue
            at = np.flatnonzero(cls == c)
            if len(at) == 0:                                             # :139
                continue
            order = at[np.argsort(sc[at], kind="stable")[::-1]]          # :137-138 (tie rule: higher position first)
            best = sc[order[0]]
            for k in order:
                if is_best and sc[k] != best:                            # :176-177
                    continue
                m = masks[idx[k]]
                ann_id = instance_id
                instance_id += 1
                area = int(np.count_nonzero(m))
                if area < 1:                                             # pycococreatortools.py:143-145 (None in the reference)
                    continue
                out["annotations"].append({
                    "id": ann_id, "image_id": int(entry["id"]), "category_id": _category(c, category_ids), "iscrowd": 0,
                    "area": area, "bbox": bbox_of(m), "segmentation": {"counts": run_lengths(m), "size": [int(m.shape[0]), int(m.shape[1])]},
                    "width": int(m.shape[1]), "height": int(m.shape[0]), "score": float(s_py(sc[k]))})
    return out


def s_py(v):
    return np.float32(v).item()                                          # np.asscalar of the fp32 score
