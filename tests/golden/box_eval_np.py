"""NumPy restatement of box evaluation, written from the published algorithms - the oracle of tests/test_box_eval_cpu.py and
tests/test_gpu_box_eval.py.

COCO side: COCOeval(..., 'bbox') is SegmEvalNp (segm_eval_np.py) with maskApi.c's bbIou in place of the mask IoU and w * h
(what COCO.loadRes stores for a bbox result) in place of the pixel count; nothing else is overridden.  pycocotools is not
available to this project, so this side is pinned to the published algorithm only.

VOC side: the PASCAL VOC devkit's matching, precision / recall and AP and the CorLoc rule as the reference's voc_eval.py /
dis_eval.py state them, with the stable tie rule (equal confidences in ascending input position).  It is pinned by
box_eval_voc.npz, captured by running the reference itself (make_golden_box_eval.py).

`write_voc_files` writes the XML annotations, the image-set file and the per-class detection files of a case in the
formats the reference reads and writes; the golden maker and the drop-in tests share it.
"""
import os

import numpy as np

from segm_eval_np import SegmEvalNp


# ---- COCO 'bbox' --------------------------------------------------------------------------------------------------------------
def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: [D, 4], [G, 4] boxes (x, y, w, h) -> [D, G]."""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    out = np.zeros((len(dt), len(gt)))
    for g in range(len(gt)):
        G = gt[g]
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d in range(len(dt)):
            D = dt[d]
            da = D[2] * D[3]
            out[d, g] = 0
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            out[d, g] = i / u
    return out


class BoxEvalNp(SegmEvalNp):
    """add_image takes boxes (x, y, w, h; fp64) where SegmEvalNp takes masks."""

    def add_image(self, img_id, gt_boxes, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, dt_boxes, dt_cat_ids, dt_scores):
        dt_boxes = np.asarray(dt_boxes, np.float64).reshape(-1, 4)
        SegmEvalNp.add_image(self, img_id, np.asarray(gt_boxes, np.float64).reshape(-1, 4), gt_cat_ids, gt_iscrowd, gt_area,
                             gt_ids, dt_boxes, dt_cat_ids, dt_scores)
        for (i, c), dts in self._dts.items():                            # loadRes: ann['area'] = bb[2] * bb[3]
            if i == img_id:
                for d in dts:
                    b = dt_boxes[d["id"] - 1]
                    d["area"] = b[2] * b[3]

    def _compute_iou(self, imgId, catId, dboxes, gboxes):
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        d = [dboxes[i] for i in inds]
        if len(d) > self.maxDets[-1]:
            d = d[0:self.maxDets[-1]]
        if len(d) == 0 or len(gboxes) == 0:
            return []
        return bb_iou(d, gboxes, [int(o["iscrowd"]) for o in gt])


# ---- VOC ----------------------------------------------------------------------------------------------------------------------
def text_round_trip(dets):
    """fp32 [n, 5] (x1, y1, x2, y2, score), 0-based -> (boxes f64 [n, 4], conf f64 [n]) as the results file carries them."""
    d = np.asarray(dets, np.float32).reshape(-1, 5)
    boxes = np.array([[float("%.1f" % (float(v) + 1.0)) for v in row[:4]] for row in d], np.float64).reshape(-1, 4)
    conf = np.array([float("%.3f" % float(row[4])) for row in d], np.float64)
    return boxes, conf


def box_area1(b):
    """Area of an inclusive-pixel box (x1, y1, x2, y2): both sides count their end pixel."""
    return (b[2] - b[0] + 1.) * (b[3] - b[1] + 1.)


def pair_overlap(det, gt):
    """The devkit's overlap of one detection with one ground truth, both (x1, y1, x2, y2) with inclusive ends: the common
    rectangle's sides (clamped at 0) give the intersection, the two areas less it the union.  fp64, one rounding per step."""
    side_x = min(det[2], gt[2]) - max(det[0], gt[0]) + 1.
    side_y = min(det[3], gt[3]) - max(det[1], gt[1]) + 1.
    common = (side_x if side_x > 0. else 0.) * (side_y if side_y > 0. else 0.)
    union = box_area1(det) + box_area1(gt) - common
    return np.float64(common) / np.float64(union)


def best_overlap(det, gts):
    """-> (largest overlap, its first position); a NaN counts as the largest, as NumPy's max / argmax treat it."""
    best, at = -np.inf, -1
    for j, g in enumerate(gts):
        v = pair_overlap(det, g)
        if at < 0 or (v > best and not np.isnan(best)) or (np.isnan(v) and not np.isnan(best)):
            best, at = v, j
    return best, at


def voc_match_np(dt_box, dt_conf, gt_box, gt_difficult, groups, ovthresh=0.5, mode=0):
    """Per (class, image) group (det_start, n_det, gt_start, n_gt): detections by descending confidence, ties in input order.
    -> tp, fp uint8 [D], ovmax f64 [D], jmax int32 [D] by input position.  mode 1: dis_eval's rule, fp = 1 - tp."""
    D = len(dt_conf)
    tp, fp = np.zeros(D, np.uint8), np.zeros(D, np.uint8)
    ovm, jm = np.full(D, -np.inf), np.full(D, -1, np.int32)
    for ds, n, gs, ng in np.asarray(groups).reshape(-1, 4):
        gts = [[float(v) for v in row] for row in np.asarray(gt_box[gs:gs + ng], np.float64).reshape(-1, 4)]
        diff = gt_difficult[gs:gs + ng]
        claimed = [False] * ng
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in np.argsort(-np.asarray(dt_conf[ds:ds + n], np.float64), kind="stable"):
                d = ds + i
                ovmax, jmax = best_overlap([float(v) for v in dt_box[d]], gts)
                ovm[d], jm[d] = ovmax, jmax
                if mode == 1:
                    tp[d] = ovmax > ovthresh
                    fp[d] = 1 - tp[d]
                elif ovmax > ovthresh:
                    if not diff[jmax]:
                        if not claimed[jmax]:
                            tp[d] = 1
                            claimed[jmax] = True
                        else:
                            fp[d] = 1
                else:
                    fp[d] = 1
    return tp, fp, ovm, jm


def voc_ap_np(rec, prec, use_07_metric=False):
    """The devkit's AP from recall / precision in detection order.  11-point form: the best precision among the points whose
    recall reaches each of the 11 levels 0, 0.1, ..., 1 (0 where none does), each divided by 11 and added up in that order.
    Area form: the curve starts at recall 0 and ends at recall 1 with precision 0; precision is replaced by its running
    maximum from the right, and every step of recall contributes its width times the precision at its right end.  The steps
    are added left to right (the reference adds them pairwise: DESIGN.md 4.14 bounds the difference)."""
    rec, prec = np.asarray(rec, np.float64), np.asarray(prec, np.float64)
    if use_07_metric:
        total = 0.
        for level in np.arange(0., 1.1, 0.1):
            reached = rec >= level
            total = total + (prec[reached].max() if reached.any() else 0) / 11.
        return total
    envelope = np.maximum(np.maximum.accumulate(prec[::-1])[::-1], 0.) if len(prec) else prec
    total, before = np.float64(0.), np.float64(0.)
    for j in range(len(rec)):
        if rec[j] != before:
            total = total + (rec[j] - before) * envelope[j]
        before = rec[j]
    if before != 1.:
        total = total + (np.float64(1.) - before) * 0.
    return total


def voc_pr_np(dt_conf, tp, fp, class_off, npos):
    """Per class: stable sort by descending confidence, cumulative tp / fp -> rec, prec [D] in sorted order at the class's
    offsets."""
    D = len(dt_conf)
    rec, prec = np.zeros(D), np.zeros(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(len(npos)):
            a, b = int(class_off[k]), int(class_off[k + 1])
            o = a + np.argsort(-np.asarray(dt_conf[a:b], np.float64), kind="stable")
            ctp = np.cumsum(np.asarray(tp)[o].astype(np.float64))
            cfp = np.cumsum(np.asarray(fp)[o].astype(np.float64))
            rec[a:b] = ctp / float(npos[k])
            prec[a:b] = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
    return rec, prec


def voc_dataset_np(case, ovthresh=0.5):
    """A whole case (see make_golden_box_eval.cases) through the text round trip -> dict(rec, prec [D], cls_off [K + 1],
    ap07, ap, corloc [K]); a class without detections has rec = prec = nothing and ap = 0."""
    K, n_img = len(case["classes"]), len(case["imagenames"])
    dbox, dconf = text_round_trip(case["dets"])
    gt_box, gt_diff, groups, class_off, npos, nimgs = [], [], [], [0], np.zeros(K), np.zeros(K)
    order = []
    for k in range(K):
        for i in range(n_img):
            g = np.flatnonzero((case["gt_cls"] == k) & (case["gt_img"] == i))
            d = np.flatnonzero((case["dt_cls"] == k) & (case["dt_img"] == i))
            gs = sum(len(b) for b in gt_box)
            if g.size:
                gt_box.append(case["gt_box"][g].astype(np.float64))
                gt_diff.append(case["gt_diff"][g].astype(np.uint8))
                npos[k] += np.count_nonzero(case["gt_diff"][g] == 0)
                nimgs[k] += 1.0
            if d.size:
                groups.append((len(order), d.size, gs, g.size))
                order.extend(d.tolist())
        class_off.append(len(order))
    order = np.asarray(order, np.int64)
    dbox, dconf = dbox[order], dconf[order]
    gb = np.concatenate(gt_box) if gt_box else np.zeros((0, 4))
    gd = np.concatenate(gt_diff) if gt_diff else np.zeros(0, np.uint8)
    tp, fp, _, _ = voc_match_np(dbox, dconf, gb, gd, groups, ovthresh, 0)
    rec, prec = voc_pr_np(dconf, tp, fp, class_off, npos)
    tp1 = voc_match_np(dbox, dconf, gb, gd, groups, ovthresh, 1)[0]
    out = dict(rec=rec, prec=prec, cls_off=np.asarray(class_off, np.int64), ap07=np.zeros(K), ap=np.zeros(K), corloc=np.zeros(K))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            a, b = class_off[k], class_off[k + 1]
            if b > a:
                out["ap07"][k] = voc_ap_np(rec[a:b], prec[a:b], True)
                out["ap"][k] = voc_ap_np(rec[a:b], prec[a:b], False)
            out["corloc"][k] = np.float64(np.sum(tp1[a:b].astype(np.float64))) / np.float64(nimgs[k])
    return out


# ---- the files of a case ------------------------------------------------------------------------------------------------------
def write_voc_files(root, case):
    """-> (detpath, annopath, imagesetfile) templates under `root`, in the formats the reference reads: one XML per image,
    the image-set list, and per class the results file '<image> <conf %.3f> <x1 + 1 %.1f> ...' in (image, detection) order."""
    anno = os.path.join(root, "Annotations")
    os.makedirs(anno, exist_ok=True)
    for i, name in enumerate(case["imagenames"]):
        objs = []
        for g in np.flatnonzero(case["gt_img"] == i):
            b = case["gt_box"][g]
            objs.append("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
                        "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                        % (case["classes"][case["gt_cls"][g]], case["gt_diff"][g], b[0], b[1], b[2], b[3]))
        with open(os.path.join(anno, name + ".xml"), "w") as f:
            f.write("<annotation><filename>%s.jpg</filename>%s</annotation>\n" % (name, "".join(objs)))
    imageset = os.path.join(root, "val.txt")
    with open(imageset, "w") as f:
        f.write("".join(n + "\n" for n in case["imagenames"]))
    for k, cls in enumerate(case["classes"]):
        with open(os.path.join(root, "det_val_%s.txt" % cls), "w") as f:
            for j in np.flatnonzero(case["dt_cls"] == k):                # (stored class-major, image-minor)
                d = case["dets"][j]
                f.write("{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n".format(case["imagenames"][case["dt_img"][j]], d[4], d[0] + 1,
                                                                          d[1] + 1, d[2] + 1, d[3] + 1))
    return os.path.join(root, "det_val_{:s}.txt"), os.path.join(anno, "{:s}.xml"), imageset
