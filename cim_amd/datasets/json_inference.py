"""lib/datasets/json_inference.py:17-55 of the reference on the device: COCO mask AP of a predictions JSON against a COCO
annotation file.  Same names, arguments and return structures; COCOeval(..., 'segm') runs in cim_amd.segm_eval
 instead of pycocotools, and the JSON files are read by the small COCO reader below.

Ground truth and predictions are RLE segmentations (compressed or uncompressed counts).  Polygon ground truth is refused
by default (NotImplementedError); with polygons="rasterize" it is filled on the device by COCO's rule
(cim_amd.segm_eval.poly_masks), or `rasterize_polygons` converts an annotation file once.  Predictions stay RLE-only.
Scores are taken in fp32, the precision the reference writes them in (tools/evaluation.py:121-131); a score that is not an
fp32 value is refused.
"""
import json

import numpy as np

from .. import segm_eval
from ..utils import mask_eval_utils
from ..utils import rle as rle_string


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

    def annToRLE(self, ann):
        """pycocotools' COCO.annToRLE: the annotation's segmentation as a compressed RLE on its image's height x width -
        a polygon list filled and merged on the device, uncompressed counts compressed, a compressed RLE as it is."""
        im = self.imgs[int(ann["image_id"])]
        h, w = int(im["height"]), int(im["width"])
        seg = ann["segmentation"]
        if isinstance(seg, list):
            counts, _ = segm_eval.rle_counts(segm_eval.poly_masks([seg], h, w), h, w)
            return {"size": [h, w], "counts": rle_string.counts_to_string(counts)}
        if isinstance(seg["counts"], list):
            return {"size": [h, w], "counts": rle_string.counts_to_string(seg["counts"])}
        return seg


def rasterize_polygons(dataset_json, out_file=None):
    """The annotation file (a path or the loaded dict) with every polygon segmentation replaced by its compressed RLE: one
    fill launch pair and one run-length pass per image, the strings by cim_amd.utils.rle.  Returns the new dataset dict (the
    input is not modified; RLE annotations are passed through) and writes it to out_file if given, so that a file is
    converted once and evaluated through the default path afterwards."""
    ds = CocoJson(dataset_json)
    new = {}
    for img_id, anns in ds.img_to_anns.items():
        todo = [a for a in anns if isinstance(a.get("segmentation"), list)]
        if not todo:
            continue
        if img_id not in ds.imgs:
            raise ValueError("annotation %s: image %d is not in the file" % (todo[0].get("id", "?"), img_id))
        h, w = int(ds.imgs[img_id]["height"]), int(ds.imgs[img_id]["width"])
        counts, off = segm_eval.rle_counts(segm_eval.poly_masks([a["segmentation"] for a in todo], h, w), h, w)
        for j, a in enumerate(todo):
            new[id(a)] = dict(a, segmentation={"size": [h, w], "counts": rle_string.counts_to_string(counts[off[j]:off[j + 1]])})
    out = dict(ds.dataset)
    out["annotations"] = [new.get(id(a), a) for a in ds.dataset.get("annotations", [])]
    if out_file is not None:
        with open(out_file, "w") as f:
            json.dump(out, f)
    return out


def _rle(ann, what, polygons="refuse"):
    seg = ann.get("segmentation")
    if isinstance(seg, list):
        if polygons == "rasterize":
            return seg
        raise NotImplementedError("%s %s: polygon segmentation is not supported (RLE only)" % (what, ann.get("id", "?")))
    if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
        raise ValueError("%s %s: segmentation must be a COCO RLE" % (what, ann.get("id", "?")))
    return seg


class InstanceEvaluator(object):
    """json_inference.py:24-52: COCO mask AP at IoU 0.25 / 0.5 / 0.7 / 0.75, per class and averaged."""

    def __init__(self, dataset_json, preds_json, polygons="refuse"):
        if polygons not in ("refuse", "rasterize"):
            raise ValueError("polygons must be 'refuse' or 'rasterize', got %r" % (polygons,))
        self.polygons = polygons                                         # what to do with polygon ground truth
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
            size = None
            if any(isinstance(a.get("segmentation"), list) for a in anns) and self.polygons == "rasterize":
                size = (int(ds.imgs[img_id]["height"]), int(ds.imgs[img_id]["width"]))       # polygons are filled on the image record's size
            ev.add_image(img_id, [_rle(a, "annotation", self.polygons) for a in anns], [a["category_id"] for a in anns],
                         [a.get("iscrowd", 0) for a in anns], [a["area"] for a in anns], [a["id"] for a in anns],
                         [_rle(d, "prediction") for d in dts], [d["category_id"] for d in dts], s32, size=size)
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


def coco_inst_seg_eval(gt_file, pred_file, polygons="refuse"):
    evaluator = InstanceEvaluator(gt_file, pred_file, polygons=polygons)
    return evaluator.evaluate()
