"""lib/utils/mask_eval_utils.py:6-108 of the reference on the device: which proposals (and so which COB masks) become the
instance-segmentation predictions of an image.  Same names, signatures and returned structures; the per-class threshold,
NMS and limit run in cim_amd.detect.  scores [N, C] f32 and boxes [N, 4]: device tensors or NumPy arrays.
"""
import numpy as np
import torch

from ..core import test as _test


def mask_results_with_nms_and_limit(cfg, scores, boxes, masks):
    """mask_eval_utils.py:6-50: (scores, boxes, cls_boxes, cls_masks); cls_masks[j + 1] = masks of class j's kept
    proposals (indexed on the masks' own device when they are a tensor)."""
    assert len(boxes) == len(masks)
    idx, cls, sc, count, boxes_h = _test._nms_limit_records(cfg, scores, boxes, _test._post_cfg(cfg, "DETECTIONS_PER_IM"))
    cls_boxes = _test._shift(_test._per_class(_test._dets(boxes_h, idx, sc), count))
    if torch.is_tensor(masks):
        sel = masks[torch.from_numpy(idx).to(masks.device)]
        cls_masks = _test._shift(torch.split(sel, [int(k) for k in count]))
    else:
        cls_masks = _test._shift(_test._per_class(np.asarray(masks)[idx], count))
    out_scores, out_boxes = _test._flat(cls_boxes, cfg.MODEL.NUM_CLASSES)
    return out_scores, out_boxes, cls_boxes, cls_masks


def mask_results_with_nms_and_limit_get_index(cfg, scores, boxes, DETECTIONS_PER_IM=100):
    """mask_eval_utils.py:54-108: (scores, boxes, cls_boxes, cls_inds), cls_inds[j + 1] = the kept proposal indices of
    class j (int64, ascending).  The limit is the argument, not cfg.TEST.DETECTIONS_PER_IM, as in the reference."""
    idx, cls, sc, count, boxes_h = _test._nms_limit_records(cfg, scores, boxes, DETECTIONS_PER_IM)
    cls_boxes = _test._shift(_test._per_class(_test._dets(boxes_h, idx, sc), count))
    cls_inds = _test._shift(_test._per_class(idx, count))
    out_scores, out_boxes = _test._flat(cls_boxes, cfg.MODEL.NUM_CLASSES)
    return out_scores, out_boxes, cls_boxes, cls_inds


def coco_encode(mask):
    """mask_eval_utils.py:113-116: pycocotools' COCOMask.encode(np.asfortranarray(mask)) with the counts decoded to str -
    {'size': [h, w], 'counts': str}.  mask [h, w]: a bool / uint8 NumPy array (0 / 1 values) or device tensor (nonzero = 1);
    the runs are found on the device (cim_amd.segm_eval), the string is built on the host (cim_amd.utils.rle)."""
    from .. import segm_eval
    if torch.is_tensor(mask):
        m = mask
    else:
        a = np.asarray(mask)
        if a.dtype != np.bool_:
            if a.dtype != np.uint8:
                raise TypeError("coco_encode: mask must be bool or uint8 (pycocotools encodes uint8), got %s" % a.dtype)
            if a.size and a.max() > 1:
                raise ValueError("coco_encode: uint8 mask with values other than 0 and 1")
        m = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(torch.device("cuda", torch.cuda.current_device()))
    if m.dim() != 2:
        raise ValueError("coco_encode: mask must be [h, w], got %s" % (tuple(m.shape),))
    return segm_eval.rle_encode(m.unsqueeze(0))[0]
