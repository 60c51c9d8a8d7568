"""lib/datasets/json_inference.py:17-55 of the reference on the device: COCO mask AP of a predictions JSON against a COCO
annotation file.  Same names, arguments and return structures; COCOeval(..., 'segm') runs in cim_amd.segm_eval
 instead of pycocotools, and the JSON files are read by the small COCO reader below.

Ground truth and predictions are RLE segmentations (compressed or uncompressed counts).  Polygon ground truth is not
supported (pycocotools rasterises it with its own polygon fill): NotImplementedError.  Scores are taken in fp32, the
precision the reference writes them in (tools/evaluation.py:121-131); a score that is not an fp32 value is refused.
"""
import json

import numpy as np

from .. import segm_eval
from ..utils import mask_eval_utils


def coco_encode(mask, width, height):
    """json_inference.py:17-22 without its cv2 resize: the mask must already be [height, width]."""
    shape = tuple(int(s) for s in mask.shape)
    if shape != (int(height), int(width)):
        raise NotImplementedError("coco_encode: mask of shape %s, asked for %d x %d - resizing (cv2.INTER_NEAREST) is not "
                                  "supported" % (shape, height, width))
    return mask_eval_utils.coco_encode((np.asarray(mask) > 0).astype(np.uint8) if not hasattr(mask, "is_cuda") else mask != 0)


class CocoJson(object):
    """The parts of pycocotools.coco.COCO the evaluator uses: images, categories, annotations per image (file order)."""

    def __init__(self, source):
        if isinstance(source, dict):
            self.dataset = source
        else:
            with open(source) as f:
                self.dataset = json.load(f)
        self.imgs = {int(im["id"]): im for im in self.dataset.get("images", [])}
        self.cats = {int(c["id"]): c for c in self.dataset.get("categories", [])}
        self.img_to_anns = {}
        for a in self.dataset.get("annotations", []):
            self.img_to_anns.setdefault(int(a["image_id"]), []).append(a)

    def getImgIds(self):
        return list(self.imgs)

    def getCatIds(self):
        return [int(c["id"]) for c in self.dataset.get("categories", [])]

    def loadCats(self, ids):
        return [self.cats[int(i)] for i in ids]


def _rle(ann, what):
    seg = ann.get("segmentation")
    if isinstance(seg, list):
        raise NotImplementedError("%s %s: polygon segmentation is not supported (RLE only)" % (what, ann.get("id", "?")))
    if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
        raise ValueError("%s %s: segmentation must be a COCO RLE" % (what, ann.get("id", "?")))
    return seg


class InstanceEvaluator(object):
    """json_inference.py:24-52: COCO mask AP at IoU 0.25 / 0.5 / 0.7 / 0.75, per class and averaged."""

    def __init__(self, dataset_json, preds_json):
        self.dataset = CocoJson(dataset_json)
        self.object_classes = [v["name"] for v in self.dataset.loadCats(self.dataset.getCatIds())]
        if isinstance(preds_json, (list, tuple)):
            preds = list(preds_json)
        else:
            with open(preds_json) as f:
                preds = json.load(f)
        ids = {int(p["image_id"]) for p in preds}
        assert ids == (ids & set(self.dataset.getImgIds())), "Results do not correspond to current coco set"
        self.preds = preds
        self.iou_thrs = np.asarray([0.25, 0.5, 0.7, 0.75])
        self.evaluator = None

    def _run(self):
        ds = self.dataset
        ev = segm_eval.SegmEvaluator(ds.getImgIds(), ds.getCatIds(), iou_thrs=self.iou_thrs)
        by_img = {}
        for p in self.preds:
            by_img.setdefault(int(p["image_id"]), []).append(p)
        for img_id in ev.img_ids:
            anns = ds.img_to_anns.get(img_id, [])
            dts = by_img.get(img_id, [])
            if not anns and not dts:
                continue
            scores = np.asarray([float(d["score"]) for d in dts], dtype=np.float64)
            s32 = scores.astype(np.float32)
            if not np.array_equal(s32.astype(np.float64), scores):
                raise ValueError("image %d: a score that is not an fp32 value (the device evaluator compares fp32 scores)" % img_id)
            ev.add_image(img_id, [_rle(a, "annotation") for a in anns], [a["category_id"] for a in anns],
                         [a.get("iscrowd", 0) for a in anns], [a["area"] for a in anns], [a["id"] for a in anns],
                         [_rle(d, "prediction") for d in dts], [d["category_id"] for d in dts], s32)
        self.evaluator = ev
        self.eval = segm_eval.to_host(ev.accumulate())
        self.stats = ev.summarize(self.eval)
        return self.eval

    def evaluate(self):
        precision = self._run()["precision"]
        mAP = dict()
        my_cls_ap = dict()
        for thr_ind, thr in enumerate(self.iou_thrs):
            ap_by_class = []
            for cls_ind, cls_name in enumerate(self.object_classes):
                cls_precision = precision[thr_ind, :, cls_ind, 0, -1]
                tmp = cls_precision[cls_precision > -1]
                if len(tmp) != 0:
                    cls_ap = np.mean(tmp)
                else:
                    cls_ap = 0
                ap_by_class.append(cls_ap)
            mAP['%.2f' % thr] = np.asarray(ap_by_class).mean()
            my_cls_ap['%.2f' % thr] = ap_by_class
        return mAP, my_cls_ap, self.object_classes


def coco_inst_seg_eval(gt_file, pred_file):
    evaluator = InstanceEvaluator(gt_file, pred_file)
    return evaluator.evaluate()
