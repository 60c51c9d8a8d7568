"""NumPy restatement of pycocotools' RLE codec (rleEncode, rleToString, rleFrString) and of COCOeval(..., 'segm')'s
computeIoU / evaluateImg / accumulate / summarize, written from the published algorithm - the oracle of
tests/test_segm_eval_cpu.py and tests/test_gpu_segm_eval.py.  pycocotools itself is not available to this project, so no
golden was captured by running it; the hand-derived cases of test_segm_eval_cpu.py pin this file.

Written as literal loops, one statement per statement of the published code, so that a reader can hold the two side by side.
Masks are dense [H, W] arrays here; IoUs are taken when an image is added, so only scores, areas and ids are kept.
"""
from collections import defaultdict

import numpy as np


# ---- RLE -----------------------------------------------------------------------------------------------------------------------
def encode_counts(mask):
    """rleEncode on the column-major pixel sequence (np.asfortranarray): alternating runs, starting with a zero-run."""
    seq = (np.asarray(mask).T.ravel() != 0).astype(np.int8)
    trans = np.flatnonzero(np.diff(np.concatenate([[0], seq])) != 0)
    return np.diff(np.concatenate([[0], trans, [seq.size]])).astype(np.uint32)


def counts_to_string(cnts):
    """rleToString."""
    s = []
    for i in range(len(cnts)):
        x = int(cnts[i])
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return "".join(s)


def string_to_counts(s):
    """rleFrString."""
    cnts = []
    p = 0
    while p < len(s):
        x = 0
        k = 0
        more = True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xFFFFFFFF)
    return np.asarray(cnts, dtype=np.uint32)


def decode_counts(cnts, h, w):
    flat = np.zeros(h * w, np.uint8)
    pos, v = 0, 0
    for c in cnts:
        flat[pos:pos + int(c)] = v
        pos += int(c)
        v = 1 - v
    return flat.reshape(w, h).T.copy()


def encode(mask):
    mask = np.asarray(mask)
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": counts_to_string(encode_counts(mask))}


# ---- maskUtils.iou on dense masks ---------------------------------------------------------------------------------------------
def mask_iou(d, g, iscrowd):
    """[D, H, W], [G, H, W] -> [D, G]: rleIou's value (the bbox pre-check only ever turns inter == 0 into 0)."""
    D, G = len(d), len(g)
    if D == 0 or G == 0:
        return []
    df = np.asarray(d).reshape(D, -1).astype(np.float32)
    gf = np.asarray(g).reshape(G, -1).astype(np.float32)
    inter = np.rint(df @ gf.T).astype(np.int64)
    ad = df.sum(1).astype(np.int64)
    ag = gf.sum(1).astype(np.int64)
    out = np.zeros((D, G))
    for i in range(D):
        for j in range(G):
            if inter[i, j] == 0:
                continue
            u = ad[i] if iscrowd[j] else ad[i] + ag[j] - inter[i, j]
            out[i, j] = float(inter[i, j]) / float(u)
    return out


# ---- COCOeval ------------------------------------------------------------------------------------------------------------------
class SegmEvalNp(object):
    def __init__(self, img_ids, cat_ids, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=(1, 10, 100)):
        self.imgIds = list(np.unique(img_ids))
        self.catIds = list(np.unique(cat_ids))
        self.iouThrs = (np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None
                        else np.asarray(iou_thrs, dtype=np.float64))
        self.recThrs = (np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True) if rec_thrs is None
                        else np.asarray(rec_thrs, dtype=np.float64))
        self.areaRng = ([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]] if area_rng is None
                        else [list(a) for a in area_rng])
        self.areaRngLbl = ["all", "small", "medium", "large"][:len(self.areaRng)] if area_rng is None else \
            ["a%d" % i for i in range(len(self.areaRng))]
        self.maxDets = sorted(max_dets)
        self._gts = defaultdict(list)
        self._dts = defaultdict(list)
        self.ious = {}

    def add_image(self, img_id, gt_masks, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, dt_masks, dt_cat_ids, dt_scores):
        """dt ids are the input positions + 1 (loadRes numbers results from 1; evaluateImg tests gtm > 0)."""
        cats = set(int(c) for c in self.catIds)
        gm, dm = defaultdict(list), defaultdict(list)
        for j in range(len(gt_cat_ids)):
            c = int(gt_cat_ids[j])
            if c not in cats:
                continue
            self._gts[img_id, c].append({"iscrowd": int(bool(gt_iscrowd[j])), "ignore": int(bool(gt_iscrowd[j])),
                                         "area": float(gt_area[j]), "id": int(gt_ids[j])})
            gm[c].append(gt_masks[j])
        for j in range(len(dt_cat_ids)):
            c = int(dt_cat_ids[j])
            if c not in cats:
                continue
            m = np.asarray(dt_masks[j])
            self._dts[img_id, c].append({"score": float(np.float32(dt_scores[j])), "area": int(np.count_nonzero(m)), "id": j + 1})
            dm[c].append(m)
        for c in set(gm) | set(dm):
            self.ious[img_id, c] = self._compute_iou(img_id, c, dm[c], gm[c])

    def _compute_iou(self, imgId, catId, dmasks, gmasks):
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        d = [dmasks[i] for i in inds]
        if len(d) > self.maxDets[-1]:
            d = d[0:self.maxDets[-1]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        return mask_iou(d, gmasks, iscrowd)

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g["ignore"] or (g["area"] < aRng[0] or g["area"] > aRng[1]):
                g["_ignore"] = 1
            else:
                g["_ignore"] = 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T = len(self.iouThrs)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g["_ignore"] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(self.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < aRng[0] or d["area"] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"image_id": imgId, "category_id": catId, "aRng": aRng, "maxDet": maxDet,
                "dtIds": [d["id"] - 1 for d in dt], "gtIds": [g["id"] for g in gt], "dtMatches": dtm, "gtMatches": gtm,
                "dtScores": [d["score"] for d in dt], "gtIgnore": gtIg, "dtIgnore": dtIg}

    def evaluate(self):
        maxDet = self.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet)
                         for catId in self.catIds for areaRng in self.areaRng for imgId in self.imgIds]
        return self.evalImgs

    def accumulate(self):
        T = len(self.iouThrs)
        R = len(self.recThrs)
        K = len(self.catIds)
        A = len(self.areaRng)
        M = len(self.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        I0 = len(self.imgIds)
        A0 = len(self.areaRng)
        for k in range(K):
            Nk = k * A0 * I0
            for a in range(A):
                Na = a * I0
                for m, maxDet in enumerate(self.maxDets):
                    E = [self.evalImgs[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind="mergesort")
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp = np.array(tp)
                        fp = np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        ss = np.zeros((R,))
                        if nd:
                            recall[t, k, a, m] = rc[-1]
                        else:
                            recall[t, k, a, m] = 0
                        pr = pr.tolist()
                        q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, self.recThrs, side="left")
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {"precision": precision, "recall": recall, "scores": scores}
        return self.eval

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
            aind = [i for i, aRng in enumerate(self.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(self.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval["precision"]
                if iouThr is not None:
                    t = np.where(iouThr == self.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval["recall"]
                if iouThr is not None:
                    t = np.where(iouThr == self.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            return mean_s

        stats = np.zeros((12,))
        stats[0] = _summarize(1)
        stats[1] = _summarize(1, iouThr=.5, maxDets=self.maxDets[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=self.maxDets[2])
        stats[3] = _summarize(1, areaRng="small", maxDets=self.maxDets[2])
        stats[4] = _summarize(1, areaRng="medium", maxDets=self.maxDets[2])
        stats[5] = _summarize(1, areaRng="large", maxDets=self.maxDets[2])
        stats[6] = _summarize(0, maxDets=self.maxDets[0])
        stats[7] = _summarize(0, maxDets=self.maxDets[1])
        stats[8] = _summarize(0, maxDets=self.maxDets[2])
        stats[9] = _summarize(0, areaRng="small", maxDets=self.maxDets[2])
        stats[10] = _summarize(0, areaRng="medium", maxDets=self.maxDets[2])
        stats[11] = _summarize(0, areaRng="large", maxDets=self.maxDets[2])
        self.stats = stats
        return stats
