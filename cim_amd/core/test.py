"""Inference with test-time augmentation on the device (f-2).

Same entry points and argument meaning as /root/reference/lib/core/test.py:48-281 (`im_detect_all`, `im_detect_bbox`,
`im_detect_bbox_aug`, `im_detect_bbox_hflip`, `im_detect_bbox_scale`): per image the reference runs 10 sequential
forward passes (TEST.SCALE flipped + 4 BBOX_AUG.SCALES x {plain, flipped} + TEST.SCALE plain, configs/*.yaml TEST
section), each preparing the image on the host (cv2), and averages the `refine_score` of the three refinement heads
over heads and passes (test.py:131-135, 219-221).

Here the image stays on the device as the BGR uint8 array (`cim_amd.utils.blob`), every pass's network input is one
HIP launch, and the plain + flipped passes of a scale run as ONE forward with batch 2: one backbone call on
[2,3,H,W], ONE ROIAlign launch over the 2N rois (batch index column), one MaskFuse / heads pass over 2N proposals
(`im_detect_bbox_aug`: 5 forwards instead of 10).  The eval branch of `Generalized_RCNN.forward` only uses the per-row
refinement scores (model_builder.py:60-68), so batching images changes nothing per proposal.
Results are device tensors (scores [N, C+... see below]); `.cpu().numpy()` gives the reference's arrays.
"""
import numpy as np
import torch

from .. import detect
from ..utils import blob as blob_utils
from .config import cfg

_TEST_DEFAULTS = dict(SCALE=600, MAX_SIZE=1000, NMS=0.3, DETECTIONS_PER_IM=100, SCORE_THRESH=1e-5)   # lib/core/config.py:123-145
_AUG_DEFAULTS = dict(ENABLED=False, SCORE_HEUR="AVG", COORD_HEUR="ID", H_FLIP=False, SCALES=(), MAX_SIZE=4000,
                     SCALE_H_FLIP=False, SCALE_SIZE_DEP=False, ASPECT_RATIOS=(), ASPECT_RATIO_H_FLIP=False)   # :167-201


def _test_cfg(key):
    t = cfg.TEST if "TEST" in cfg else {}
    return t[key] if key in t else _TEST_DEFAULTS[key]


def _aug_cfg(key):
    t = cfg.TEST if "TEST" in cfg else {}
    a = t["BBOX_AUG"] if "BBOX_AUG" in t else {}
    return a[key] if key in a else _AUG_DEFAULTS[key]


def flip_boxes(boxes, im_width):
    """lib/utils/boxes.py:252-257."""
    out = boxes.clone() if torch.is_tensor(boxes) else boxes.copy()
    out[:, 0::4] = im_width - boxes[:, 2::4] - 1
    out[:, 2::4] = im_width - boxes[:, 0::4] - 1
    return out


def _scores(return_dict):
    """mean over the refinement heads (test.py:131-135)."""
    s = return_dict["refine_score"][0].clone()
    for r in return_dict["refine_score"][1:]:
        s += r
    return s / len(return_dict["refine_score"])


def _forward(model, im, target_scale, target_max_size, boxes, masks, flips, flag):
    """One forward over len(flips) views of `im` at one scale.  Returns ([scores per view], im_scale, blob_conv)."""
    dev = next(model.parameters()).device
    flag = flag or cfg.transform_mode
    im_w = int(im.shape[1])
    boxes_t = torch.as_tensor(np.asarray(boxes), dtype=torch.float32, device=dev) if not torch.is_tensor(boxes) else boxes.to(dev)
    masks_t = torch.as_tensor(np.asarray(masks), dtype=torch.float32, device=dev) if not torch.is_tensor(masks) else masks.to(dev, torch.float32)
    src = blob_utils._as_device_u8(im, dev)
    views, rois, mks = [], [], []
    im_scale = None
    for b, hf in enumerate(flips):
        ims, scales = blob_utils.prep_im_for_blob(src, None, [target_scale], target_max_size, flag, hflip=hf, device=dev)
        im_scale = scales[0]
        views.append(ims[0])
        bx = flip_boxes(boxes_t, im_w) if hf else boxes_t                    # test.py:252
        rois.append(blob_utils.project_im_rois(bx, im_scale, batch_index=b, device=dev))
        mks.append(torch.flip(masks_t, dims=(2,)) if hf else masks_t)        # test.py:256
    data = torch.stack(views, 0)                                             # same size: same image, same scale
    out = model(data=data, rois=torch.cat(rois, 0), masks=torch.cat(mks, 0), labels=None, gtrois=None, mat=None)
    n = boxes_t.shape[0]
    s = _scores(out)
    return [s[i * n:(i + 1) * n] for i in range(len(flips))], im_scale, out["blob_conv"]


def im_detect_bbox(model, im, target_scale, target_max_size, boxes=None, masks=None, mat=None, path=None, flag=None,
                   labels=None):
    """test.py:83-146: one pass.  Returns (scores [N,C], pred_boxes, im_scale, blob_conv)."""
    if cfg.DEDUP_BOXES > 0:
        raise NotImplementedError("DEDUP_BOXES > 0 (no shipped config uses it: configs/*.yaml set 0)")
    scores, im_scale, blob_conv = _forward(model, im, target_scale, target_max_size, boxes, masks, [False], flag)
    return scores[0], boxes, im_scale, blob_conv


def im_detect_bbox_hflip(model, im, target_scale, target_max_size, box_proposals=None, masks=None, mat=None, path=None,
                         flag=None, labels=None):
    """test.py:244-264: the horizontally flipped image; boxes come back in the original frame."""
    scores, im_scale, _ = _forward(model, im, target_scale, target_max_size, box_proposals, masks, [True], flag)
    return scores[0], box_proposals, im_scale


def im_detect_bbox_scale(model, im, target_scale, target_max_size, box_proposals=None, masks=None, mat=None, hflip=False,
                         path=None, flag=None, labels=None):
    """test.py:267-281."""
    scores, _, _ = _forward(model, im, target_scale, target_max_size, box_proposals, masks, [bool(hflip)], flag)
    return scores[0], box_proposals


def im_detect_bbox_aug(model, im, box_proposals=None, masks=None, mat=None, path=None, flag=None, labels=None, batched=True):
    """test.py:149-241 with the plain and flipped pass of every scale in one forward (batched=False: one by one, in
    the reference's order - same result up to fp32 summation order of the average)."""
    assert not _aug_cfg("SCALE_SIZE_DEP"), "Size dependent scaling not implemented"
    if len(_aug_cfg("ASPECT_RATIOS")):
        raise NotImplementedError("aspect-ratio augmentation (no shipped config uses it)")
    heur, coord = _aug_cfg("SCORE_HEUR"), _aug_cfg("COORD_HEUR")
    # test.py:154-160: the two heuristics are UNION together or not at all
    assert not heur == "UNION" or coord == "UNION", "Coord heuristic must be union whenever score heuristic is union"
    assert not coord == "UNION" or heur == "UNION", "Score heuristic must be union whenever coord heuristic is union"
    if heur not in ("ID", "AVG", "UNION"):
        raise NotImplementedError("Score heur {} not supported".format(heur))
    if coord not in ("ID", "AVG", "UNION"):
        raise NotImplementedError("Coord heur {} not supported".format(coord))
    scale0, max0 = _test_cfg("SCALE"), _test_cfg("MAX_SIZE")
    # views in the REFERENCE's order (test.py:171-216): flipped @ SCALE, then per scale (plain, flipped), identity LAST;
    # `order` = position of a (scale slot, flip) view in that order
    order, views = {}, []
    if _aug_cfg("H_FLIP"):
        order[(-1, True)] = len(order)
    for si, _ in enumerate(_aug_cfg("SCALES")):
        order[(si, False)] = len(order)
        if _aug_cfg("SCALE_H_FLIP"):
            order[(si, True)] = len(order)
    order[(-1, False)] = len(order)
    plan = []                                            # (scale slot, scale, max_size, [flips]): one forward each
    if batched:
        plan.append((-1, scale0, max0, [True, False] if _aug_cfg("H_FLIP") else [False]))
        for si, scale in enumerate(_aug_cfg("SCALES")):
            plan.append((si, scale, _aug_cfg("MAX_SIZE"), [False, True] if _aug_cfg("SCALE_H_FLIP") else [False]))
    else:
        if _aug_cfg("H_FLIP"):
            plan.append((-1, scale0, max0, [True]))
        for si, scale in enumerate(_aug_cfg("SCALES")):
            plan.append((si, scale, _aug_cfg("MAX_SIZE"), [False]))
            if _aug_cfg("SCALE_H_FLIP"):
                plan.append((si, scale, _aug_cfg("MAX_SIZE"), [True]))
        plan.append((-1, scale0, max0, [False]))
    scores_i = im_scale_i = blob_conv_i = None
    for slot, scale, max_size, flips in plan:
        scores, im_scale, blob_conv = _forward(model, im, scale, max_size, box_proposals, masks, flips, flag)
        for k, f in enumerate(flips):
            views.append((order[(slot, f)], scores[k]))
            if slot == -1 and not f:                     # the identity view (test.py:211-216)
                scores_i, im_scale_i = scores[k], im_scale
                blob_conv_i = blob_conv[k:k + 1]
    scores_ts = [sc for _, sc in sorted(views, key=lambda v: v[0])]
    if heur == "ID":
        scores_c = scores_i
    elif heur == "AVG":
        scores_c = torch.stack(scores_ts, 0).mean(0)
    else:
        scores_c = torch.cat(scores_ts, 0)
    # every view scores the SAME proposals (no box regression on this path: im_detect_bbox returns the proposals), so
    # ID and AVG give the proposals themselves and UNION repeats them once per view (np.vstack(boxes_ts), test.py:236)
    boxes_c = box_proposals
    if coord == "UNION" and box_proposals is not None:
        rep = len(scores_ts)
        boxes_c = (box_proposals.repeat(rep, 1) if torch.is_tensor(box_proposals)
                   else np.vstack([box_proposals] * rep))
    return scores_c, boxes_c, im_scale_i, blob_conv_i


def im_detect_all(model, im, box_proposals=None, masks=None, mat=None, timers=None, path=None, flag=None, labels=None):
    """test.py:48-80."""
    if _aug_cfg("ENABLED"):
        scores, boxes, _, _ = im_detect_bbox_aug(model, im, box_proposals, masks, mat, path=path, flag=flag, labels=labels)
    else:
        scores, boxes, _, _ = im_detect_bbox(model, im, _test_cfg("SCALE"), _test_cfg("MAX_SIZE"), box_proposals, masks, mat,
                                             path=path, flag=flag, labels=labels)
    return {"scores": scores, "boxes": boxes}


# ---------------------------------------------------------------- detections from scores (test.py:320-420) on the device
def _post_cfg(c, key):
    t = c.TEST if "TEST" in c else {}
    return t[key] if key in t else _TEST_DEFAULTS[key]


def _post_check(c):
    t = c.TEST if "TEST" in c else {}
    for k in ("SOFT_NMS", "BBOX_VOTE"):                                  # config.py:150-165: both off by default
        if k in t and "ENABLED" in t[k] and t[k]["ENABLED"]:
            raise NotImplementedError("TEST.%s.ENABLED (no shipped config enables it)" % k)


_SOFT_NMS_DEFAULTS = dict(ENABLED=False, METHOD="linear", SIGMA=0.5)                          # lib/core/config.py:206-212
_BBOX_VOTE_DEFAULTS = dict(ENABLED=False, VOTE_TH=0.8, SCORING_METHOD="ID")                   # :218-229


def _soft_vote_cfg(c):
    """TEST.SOFT_NMS / TEST.BBOX_VOTE of cfg `c` as cim_amd.detect.postprocess's (soft_nms, box_vote); None where off.
    The reference's call fixes the soft-NMS minimum score at 0.0001 and leaves box_voting's beta at 1.0 (test.py:379-396)."""
    t = c.TEST if "TEST" in c else {}

    def get(group, defaults, key):
        g = t[group] if group in t else {}
        return g[key] if key in g else defaults[key]

    soft = vote = None
    if get("SOFT_NMS", _SOFT_NMS_DEFAULTS, "ENABLED"):
        soft = dict(method=get("SOFT_NMS", _SOFT_NMS_DEFAULTS, "METHOD"), sigma=get("SOFT_NMS", _SOFT_NMS_DEFAULTS, "SIGMA"),
                    min_score=0.0001)
    if get("BBOX_VOTE", _BBOX_VOTE_DEFAULTS, "ENABLED"):
        vote = dict(thresh=get("BBOX_VOTE", _BBOX_VOTE_DEFAULTS, "VOTE_TH"),
                    scoring_method=get("BBOX_VOTE", _BBOX_VOTE_DEFAULTS, "SCORING_METHOD"), beta=1.0)
    return soft, vote


def _nms_limit_records(c, scores, boxes, max_det):
    """The reference's per-class threshold + NMS + limit of cfg `c`, on the device: host (idx, cls, score, count, boxes)."""
    _post_check(c)
    num_classes = c.MODEL.NUM_CLASSES
    s, b, boxes_h = detect.device_inputs(scores, boxes)
    det = detect.nms_limit(s, b, _post_cfg(c, "SCORE_THRESH"), _post_cfg(c, "NMS"), max_det, num_classes=num_classes)
    return detect.to_host(det) + (boxes_h,)


def _per_class(values, count):
    """Records in class order -> one array per class (lengths `count`)."""
    return np.split(values, np.cumsum(count)[:-1])


def _shift(per_class):
    """test.py:405-409: cls_boxes[0] = [] and class j at j + 1."""
    return [[]] + list(per_class)


def _flat(cls_boxes, num_classes):
    """test.py:415-418 - np.vstack over j in range(1, num_classes): the LAST class is not in the flat arrays."""
    im_results = np.vstack([cls_boxes[j] for j in range(1, num_classes)])
    return im_results[:, -1], im_results[:, :-1]


def _dets(boxes_h, idx, score):
    return np.hstack((boxes_h[idx], score[:, None])).astype(np.float32, copy=False)


def box_results_with_nms_and_limit(scores, boxes):
    """test.py:355-420: (scores, boxes, cls_boxes) with cls_boxes of length NUM_CLASSES + 1, cls_boxes[0] == [] and
    float32 [k, 5] arrays (x1, y1, x2, y2, score) in ascending proposal order.  scores [N, C] f32 and boxes [N, 4]: device
    tensors (im_detect_all's) or NumPy arrays.  TEST.SOFT_NMS.ENABLED: rows in selection order with the decayed scores;
    TEST.BBOX_VOTE.ENABLED: voted boxes and, by SCORING_METHOD, scores; the limit comes after both (test.py:378-408)."""
    soft, vote = _soft_vote_cfg(cfg)
    if soft is None and vote is None:
        idx, cls, sc, count, boxes_h = _nms_limit_records(cfg, scores, boxes, _post_cfg(cfg, "DETECTIONS_PER_IM"))
        rows = _dets(boxes_h, idx, sc)
    else:
        # test.py:378-396: rows in selection order with the decayed scores under soft-NMS, voted boxes / scores under voting
        s, b, _ = detect.device_inputs(scores, boxes)
        det = detect.postprocess(s, b, _post_cfg(cfg, "SCORE_THRESH"), _post_cfg(cfg, "NMS"),
                                 _post_cfg(cfg, "DETECTIONS_PER_IM"), soft_nms=soft, box_vote=vote,
                                 num_classes=cfg.MODEL.NUM_CLASSES)
        _, _, sc, count, bx = detect.softvote_to_host(det)
        rows = np.hstack((bx, sc[:, None])).astype(np.float32, copy=False)
    cls_boxes = _shift(_per_class(rows, count))
    out_scores, out_boxes = _flat(cls_boxes, cfg.MODEL.NUM_CLASSES)
    return out_scores, out_boxes, cls_boxes


def box_results_for_corloc(scores, boxes):
    """test.py:320-352: per class the highest-scoring proposal (np.argmax), same structures as above (one row a class)."""
    num_classes = cfg.MODEL.NUM_CLASSES
    s, _, boxes_h = detect.device_inputs(scores, boxes, boxes_on_device=False)
    idx, sc = detect.corloc_host(s, num_classes)
    cls_boxes = _shift(_dets(boxes_h, idx[j:j + 1], sc[j:j + 1]) for j in range(num_classes))
    out_scores, out_boxes = _flat(cls_boxes, num_classes)
    return out_scores, out_boxes, cls_boxes
