"""Box evaluation on the device: COCOeval(..., 'bbox'), the PASCAL VOC devkit's AP and CorLoc (csrc/box_eval.hip,
DESIGN.md 4.14).

Replaces what the reference's task_evaluation.evaluate_all runs on the boxes inference produced: pycocotools' COCOeval on
boxes (lib/datasets/json_dataset_evaluator.py:105-118), lib/datasets/voc_eval.py and lib/datasets/dis_eval.py.
`BoxEvaluator` is `SegmEvaluator` with boxes in place of masks (same constructor, accumulate, summarize, eval_imgs: the
matcher, the records and the accumulation are the same code); `VocBoxEvaluator` matches a whole dataset in one launch and
sorts, scans and integrates per class in a second call.  Device arguments must be CUDA/HIP tensors (no CPU fallback); host
arrays are uploaded.  The file-based drop-ins are cim_amd.datasets.voc_eval / dis_eval / json_dataset_evaluator.
"""
import numpy as np
import torch

from . import _lib
from .segm_eval import MAX_DT, MAX_GT, SegmEvaluator, _err, _upload, merge_rounds, to_host  # noqa: F401

MAX_RUN = _lib.CONSTANTS["CIM_VOC_MAX_RUN"]
THR11 = np.arange(0., 1.1, 0.1)  # voc_ap's 11 recall thresholds: the host's fp64 values, never recomputed on the device


def _host_f32(x, what, cols=None):
    """Device tensor or host array of float32 -> host float32 array (one copy for a device tensor)."""
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise _lib.CimHipError("cim_amd.box_eval: %s must be a CUDA/HIP tensor or a host array (no CPU fallback)" % what)
        if x.dtype != torch.float32:
            raise TypeError("cim_amd.box_eval: %s must be float32, got %s" % (what, x.dtype))
        a = x.detach().cpu().numpy()
    else:
        a = np.asarray(x)
        if a.size and a.dtype != np.float32:
            raise TypeError("cim_amd.box_eval: %s must be float32, got %s" % (what, a.dtype))
        a = a.astype(np.float32)
    return a.reshape(-1, cols) if cols else a.ravel()


def xyxy_to_xywh64(boxes):
    """utils/boxes.xyxy_to_xywh on fp32 boxes as json_dataset_evaluator.py:90-92 applies it: the fp32 values widened to
    fp64, then w = x2 - x1 + 1, h = y2 - y1 + 1."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4).astype(np.float64)
    return np.hstack((b[:, 0:2], b[:, 2:4] - b[:, 0:2] + 1))


class BoxEvaluator(SegmEvaluator):
    """COCOeval(cocoGt, cocoDt, 'bbox'), fed one image at a time; everything but add_image is SegmEvaluator's."""

    def add_image(self, img_id, gt_boxes, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, dt_boxes, dt_cat_ids, dt_scores):
        """One image: ground-truth boxes [G, 4] (x, y, w, h; host, any real dtype) with category ids, iscrowd flags, `area`
        fields and annotation ids; detections as fp32 (x1, y1, x2, y2) boxes [D, 4] (device tensor or host array; made xywh
        in fp64 as the reference's results file has them), category ids (host) and fp32 scores (device tensor or host
        array).  Launches the image's IoU and matching on the current stream; does not synchronise."""
        if torch.is_tensor(dt_boxes):
            if not dt_boxes.is_cuda:
                raise _lib.CimHipError("cim_amd.box_eval: dt_boxes must be a CUDA/HIP tensor (no CPU fallback)")
            if dt_boxes.dtype != torch.float32:
                raise TypeError("cim_amd.box_eval: dt_boxes must be float32, got %s" % dt_boxes.dtype)
            b = dt_boxes.to(self.device).reshape(-1, 4).double()
            xywh = torch.cat((b[:, 0:2], b[:, 2:4] - b[:, 0:2] + 1), 1).contiguous()       # (fp64 adds: exact as NumPy's)
        else:
            xywh = xyxy_to_xywh64(_host_f32(dt_boxes, "dt_boxes", 4))
        self._add_xywh(img_id, gt_boxes, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, xywh, dt_cat_ids, dt_scores)

    def _add_xywh(self, img_id, gt_boxes, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, dt_xywh, dt_cat_ids, dt_scores):
        """add_image on detections that are (x, y, w, h) fp64 already (a device tensor or a host array): a results file's."""
        img_id, gcat, crowd, garea, gids, dcat, scores_d = self._image_fields(img_id, gt_cat_ids, gt_iscrowd, gt_area, gt_ids,
                                                                              dt_cat_ids, dt_scores)
        G, D = gcat.size, dcat.size
        gb = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
        if gb.shape[0] != G:
            raise ValueError("cim_amd.box_eval: %d ground truths, %d boxes" % (G, gb.shape[0]))
        dev = self.device
        n = dt_xywh.shape[0] if dt_xywh.ndim == 2 else -1
        if n != D:
            raise ValueError("cim_amd.box_eval: %d detections, boxes of shape %s" % (D, tuple(dt_xywh.shape)))
        db_d = None
        if D:
            db_d = dt_xywh if torch.is_tensor(dt_xywh) else _upload(np.asarray(dt_xywh, np.float64), dev)
        info, meta, ndl, ngl, rec_off, pair_off = self._image_groups(img_id, dcat, gcat, crowd, gids)
        if meta is None:
            return
        T, A = len(self.iou_thrs), len(self.area_rng)
        ws_bytes = _lib.call("cim_box_image_ws_bytes", D, G, pair_off)
        if ws_bytes < 0:
            raise ValueError(_err())
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        records = torch.empty(max(rec_off, 8), dtype=torch.uint8, device=dev)
        meta_d = _upload(meta, dev)
        gb_d = _upload(gb, dev) if G else None
        garea_d = _upload(garea, dev) if G else None
        gids_d = _upload(gids, dev) if G else None
        thr_d, rng_d, _, _ = self._params()
        _lib.call("cim_box_eval_image", _lib.ptr(db_d), D, _lib.ptr(gb_d), G, _lib.ptr(scores_d), meta_d.data_ptr(),
                  len(info["groups"]), ndl, ngl, pair_off, _lib.ptr(garea_d), _lib.ptr(gids_d), thr_d.data_ptr(), T,
                  rng_d.data_ptr(), A, ws.data_ptr(), records.data_ptr(), _lib.stream_ptr())
        info["records"] = records


# ---- VOC -------------------------------------------------------------------------------------------------------------------------
def voc_text_round_trip(dets):
    """What _write_voc_results_files and voc_eval's reader do to the numbers of fp32 detections [n, 5] (x1, y1, x2, y2,
    score): the confidence through '{:.3f}', the coordinates through '{:.1f}' after + 1 - both on the fp64 value of the fp32
    entry (NumPy 1's float32 + int; NumPy 2 adds in fp32, which differs only where x + 1 is not an fp32 value) - and parsed
    back.  -> (boxes f64 [n, 4], conf f64 [n])."""
    d = np.asarray(dets, np.float32).reshape(-1, 5).astype(np.float64)
    conf = np.array(["{:.3f}".format(v) for v in d[:, 4]], np.float64)
    plus = d[:, :4] + 1.0
    boxes = np.array([[float("{:.1f}".format(v)) for v in row] for row in plus], np.float64).reshape(-1, 4)
    return boxes, conf


def voc_runs(starts, lengths, classes):
    """Runs of cim_voc_ap from the (class, image) groups (class-major): each group cut into pieces of <= MAX_RUN, empty
    ones dropped -> (start, length, class) int64 arrays."""
    s, n, c = [], [], []
    for a, l, k in zip(starts, lengths, classes):
        for o in range(0, int(l), MAX_RUN):
            s.append(int(a) + o)
            n.append(min(MAX_RUN, int(l) - o))
            c.append(int(k))
    return np.asarray(s, np.int64), np.asarray(n, np.int64), np.asarray(c, np.int64)


def voc_match(dt_box, dt_conf, gt_box, gt_difficult, groups, ovthresh=0.5, mode=0):
    """cim_voc_match on device tensors: dt_box [D, 4] f64, dt_conf [D] f64, gt_box [G, 4] f64, gt_difficult [G] uint8, groups
    [n, 4] int32 -> (tp uint8 [D], fp uint8 [D], ovmax f64 [D], jmax int32 [D]) device tensors."""
    for t, dt, what in ((dt_box, torch.float64, "dt_box"), (dt_conf, torch.float64, "dt_conf"), (gt_box, torch.float64, "gt_box"),
                        (gt_difficult, torch.uint8, "gt_difficult"), (groups, torch.int32, "groups")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.CimHipError("cim_amd.box_eval: %s must be a CUDA/HIP tensor (no CPU fallback)" % what)
        if t.dtype != dt:
            raise TypeError("cim_amd.box_eval: %s must be %s, got %s" % (what, dt, t.dtype))
    dt_box, dt_conf, gt_box, gt_difficult, groups = (t.contiguous() for t in (dt_box, dt_conf, gt_box, gt_difficult, groups))
    D, G = dt_conf.numel(), gt_difficult.numel()
    if dt_box.numel() != 4 * D or gt_box.numel() != 4 * G or groups.numel() % 4:
        raise ValueError("cim_amd.box_eval: %d confidences and %d box numbers, %d difficult flags and %d box numbers, %d group "
                         "numbers" % (D, dt_box.numel(), G, gt_box.numel(), groups.numel()))
    dev = dt_conf.device
    tp = torch.zeros(D, dtype=torch.uint8, device=dev)
    fp = torch.zeros(D, dtype=torch.uint8, device=dev)
    ovmax = torch.full((D,), -np.inf, dtype=torch.float64, device=dev)
    jmax = torch.full((D,), -1, dtype=torch.int32, device=dev)
    _lib.call("cim_voc_match", dt_box.data_ptr(), dt_conf.data_ptr(), D, gt_box.data_ptr(), gt_difficult.data_ptr(), G,
              groups.data_ptr(), groups.numel() // 4, float(ovthresh), int(mode), tp.data_ptr(), fp.data_ptr(), ovmax.data_ptr(),
              jmax.data_ptr(), _lib.stream_ptr())
    return tp, fp, ovmax, jmax


def voc_ap(dt_conf, tp, fp, class_off, npos, runs, use_07_metric=False):
    """cim_voc_ap: dt_conf f64 [D], tp / fp uint8 [D] device tensors, class-major; class_off [K + 1] and npos [K] host arrays;
    runs = (start, length, class) host arrays as voc_runs makes them -> (rec f64 [D], prec f64 [D], ap f64 [K]) device tensors,
    rec / prec in sorted order at each class's offsets."""
    for t, dt, what in ((dt_conf, torch.float64, "dt_conf"), (tp, torch.uint8, "tp"), (fp, torch.uint8, "fp")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.CimHipError("cim_amd.box_eval: %s must be a CUDA/HIP tensor (no CPU fallback)" % what)
        if t.dtype != dt:
            raise TypeError("cim_amd.box_eval: %s must be %s, got %s" % (what, dt, t.dtype))
    dt_conf, tp, fp = dt_conf.contiguous(), tp.contiguous(), fp.contiguous()
    D = dt_conf.numel()
    class_off = np.asarray(class_off, np.int64).ravel()
    npos = np.asarray(npos, np.float64).ravel()
    K = npos.size
    rs, rl, rc = (np.asarray(a, np.int64).ravel() for a in runs)
    if tp.numel() != D or fp.numel() != D or class_off.size != K + 1 or class_off[0] != 0 or class_off[-1] != D or \
            np.any(np.diff(class_off) < 0):
        raise ValueError("cim_amd.box_eval: %d detections, %d tp, %d fp, class offsets %s for %d classes"
                         % (D, tp.numel(), fp.numel(), class_off.tolist()[:4], K))
    if rl.size and (rl.min() < 1 or rl.max() > MAX_RUN or rs[0] != 0 or np.any(rs[1:] != (rs + rl)[:-1]) or rs[-1] + rl[-1] != D
                    or np.any(class_off[rc] > rs) or np.any(rs + rl > class_off[rc + 1])) or (D and not rl.size):
        raise ValueError("cim_amd.box_eval: the runs must tile the detections in pieces of 1..%d, each inside its class" % MAX_RUN)
    ws_bytes = _lib.call("cim_voc_ap_ws_bytes", D)
    if ws_bytes < 0:
        raise ValueError(_err())
    dev = dt_conf.device
    rounds = merge_rounds(rs, rl, rc)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rec = torch.empty(D, dtype=torch.float64, device=dev)
    prec = torch.empty(D, dtype=torch.float64, device=dev)
    ap = torch.empty(K, dtype=torch.float64, device=dev)
    off_d, npos_d = _upload(class_off, dev), _upload(npos, dev)
    runs_d = _upload(np.stack([rs, rl], 1), dev) if rl.size else None
    jobs_d = roff_d = None
    if rounds:
        roff = np.concatenate([[0], np.cumsum([len(j) for j in rounds])]).astype(np.int64)
        jobs_d, roff_d = _upload(np.concatenate(rounds).astype(np.int64), dev), _upload(roff, dev)
    thr_d = _upload(THR11, dev) if use_07_metric else None
    _lib.call("cim_voc_ap", dt_conf.data_ptr(), tp.data_ptr(), fp.data_ptr(), D, off_d.data_ptr(), npos_d.data_ptr(), K,
              _lib.ptr(runs_d), rl.size, _lib.ptr(jobs_d), _lib.ptr(roff_d), len(rounds), _lib.ptr(thr_d), ws.data_ptr(),
              rec.data_ptr(), prec.data_ptr(), ap.data_ptr(), _lib.stream_ptr())
    return rec, prec, ap


class VocBoxEvaluator(object):
    """voc_eval / dis_eval over a whole dataset: add_image per image, then evaluate() and / or corloc()."""

    def __init__(self, classes, ovthresh=0.5, use_07_metric=False, text_round_trip=True, device=None):
        self.classes = list(classes)
        if not self.classes:
            raise ValueError("cim_amd.box_eval: no classes")
        self.ovthresh = float(ovthresh)
        self.use_07_metric = bool(use_07_metric)
        self.text_round_trip = bool(text_round_trip)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise _lib.CimHipError("cim_amd.box_eval: VocBoxEvaluator needs a CUDA/HIP device (no CPU fallback)")
        self._index = {}
        self._gt = [[] for _ in self.classes]                            # per class: (image position, boxes f64, difficult u8)
        self._dt = [[] for _ in self.classes]                            # per class: (image position, boxes f64, conf f64)

    def add_image(self, index, gt_boxes, gt_classes, gt_difficult, dets_per_class):
        """index: the image's name; gt_boxes [G, 4] (xmin, ymin, xmax, ymax as the XML has them), gt_classes [G] positions in
        `classes`, gt_difficult [G]; dets_per_class: one entry per class - fp32 [n, 5] (x1, y1, x2, y2, score; 0-based, as
        all_boxes holds them; device tensor or host array), or an empty list / None."""
        if len(dets_per_class) != len(self.classes):
            raise ValueError("cim_amd.box_eval: %d classes, detections of %d" % (len(self.classes), len(dets_per_class)))
        staged = []
        for k, dets in enumerate(dets_per_class):
            if dets is None or (isinstance(dets, (list, tuple)) and len(dets) == 0):
                continue
            d = _host_f32(dets, "detections of class %d" % k, 5)
            if self.text_round_trip and np.isfinite(d).all():            # (add_parsed refuses the rest)
                boxes, conf = voc_text_round_trip(d)
            else:
                boxes, conf = d[:, :4].astype(np.float64) + 1.0, d[:, 4].astype(np.float64)
            staged.append((k, boxes, conf))
        self.add_parsed(index, gt_boxes, gt_classes, gt_difficult, staged)

    def add_parsed(self, index, gt_boxes, gt_classes, gt_difficult, dets):
        """add_image on numbers that already went through a results file: dets = [(class position, boxes f64 [n, 4] 1-based,
        confidences f64 [n])], each class at most once.  Every check of the values is here; a refused image leaves the
        evaluator as it was."""
        if index in self._index:
            raise ValueError("cim_amd.box_eval: image %r added twice" % (index,))
        K = len(self.classes)
        gb = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
        gc = np.asarray(gt_classes, dtype=np.int64).ravel()
        gd = np.asarray(gt_difficult).astype(bool).ravel().astype(np.uint8)
        if not gb.shape[0] == gc.size == gd.size:
            raise ValueError("cim_amd.box_eval: ground-truth fields of different lengths")
        if gc.size and (gc.min() < 0 or gc.max() >= K):
            raise ValueError("cim_amd.box_eval: a ground-truth class outside 0..%d" % (K - 1))
        if gc.size and np.bincount(gc).max() > MAX_GT:
            raise ValueError("cim_amd.box_eval: %d ground truths of one class in image %r, the kernels take <= %d"
                             % (np.bincount(gc).max(), index, MAX_GT))
        staged = [(int(k), np.asarray(b, np.float64).reshape(-1, 4), np.asarray(c, np.float64).ravel()) for k, b, c in dets]
        if len({k for k, _, _ in staged}) != len(staged) or any(not 0 <= k < K for k, _, _ in staged):
            raise ValueError("cim_amd.box_eval: image %r: detection classes must be distinct positions in 0..%d" % (index, K - 1))
        for k, b, c in staged:
            if b.shape[0] != c.size:
                raise ValueError("cim_amd.box_eval: class %d in image %r: %d boxes, %d confidences" % (k, index, b.shape[0], c.size))
            if np.isnan(c).any():
                raise ValueError("cim_amd.box_eval: NaN score")
            if not np.isfinite(b).all():
                raise ValueError("cim_amd.box_eval: a non-finite box coordinate")
            if c.size > MAX_DT:
                raise ValueError("cim_amd.box_eval: %d detections of class %d in image %r, the kernels take <= %d"
                                 % (c.size, k, index, MAX_DT))
        pos = self._index[index] = len(self._index)
        for k in np.unique(gc):
            self._gt[k].append((pos, gb[gc == k], gd[gc == k]))
        for k, boxes, conf in staged:
            if conf.size:
                self._dt[k].append((pos, boxes, conf))

    def _arrays(self):
        """Class-major, image-minor arrays and the (class, image) groups of cim_voc_match."""
        K = len(self.classes)
        dbox, dconf, gbox, gdiff, groups, gcls = [], [], [], [], [], []
        nd = ng = 0
        class_off = [0]
        npos, nimgs = np.zeros(K), np.zeros(K)
        for k in range(K):
            gts = {}
            for pos, b, df in self._gt[k]:
                gts[pos] = (ng, b.shape[0])
                gbox.append(b)
                gdiff.append(df)
                ng += b.shape[0]
                npos[k] += np.count_nonzero(df == 0)
                nimgs[k] += 1.0
            for pos, b, c in sorted(self._dt[k], key=lambda t: t[0]):
                gs, n = gts.get(pos, (0, 0))
                groups.append((nd, b.shape[0], gs, n))
                gcls.append(k)
                dbox.append(b)
                dconf.append(c)
                nd += b.shape[0]
            class_off.append(nd)
        cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)
        return (cat(dbox, (0, 4), np.float64), cat(dconf, (0,), np.float64), cat(gbox, (0, 4), np.float64),
                cat(gdiff, (0,), np.uint8), np.asarray(groups, np.int32).reshape(-1, 4), np.asarray(gcls, np.int64),
                np.asarray(class_off, np.int64), npos, nimgs)

    def _match(self, mode):
        dbox, dconf, gbox, gdiff, groups, gcls, class_off, npos, nimgs = self._arrays()
        dev = self.device
        one = lambda a, dt: _upload(a, dev) if a.size else torch.zeros(a.shape, dtype=dt, device=dev)
        conf_d = one(dconf, torch.float64)
        out = voc_match(one(dbox, torch.float64), conf_d, one(gbox, torch.float64), one(gdiff, torch.uint8),
                        one(groups, torch.int32), self.ovthresh, mode)
        return conf_d, out, groups, gcls, class_off, npos, nimgs

    def evaluate(self):
        """-> ({class: (rec, prec, ap)}, mean AP): voc_eval's return values per class (host fp64 arrays; a class without
        detections gives (0, 0, 0) as the reference's early return does)."""
        conf_d, (tp, fp, _, _), groups, gcls, class_off, npos, _ = self._match(0)
        rec, prec, ap = voc_ap(conf_d, tp, fp, class_off, npos, voc_runs(groups[:, 0], groups[:, 1], gcls), self.use_07_metric)
        rec, prec, ap = rec.cpu().numpy(), prec.cpu().numpy(), ap.cpu().numpy()
        out = {}
        for k, name in enumerate(self.classes):
            a, b = class_off[k], class_off[k + 1]
            out[name] = (rec[a:b], prec[a:b], ap[k]) if b > a else (0, 0, 0)
        return out, float(np.mean([v[2] for v in out.values()]))

    def corloc(self):
        """-> ({class: CorLoc}, mean): dis_eval's sum(tp) / nimgs per class, nimgs = the images with a ground truth of the class
        (IEEE division: NaN for a class without ground truth and detections, as NumPy gives)."""
        _, (tp, _, _, _), _, _, class_off, _, nimgs = self._match(1)
        csum = np.concatenate([[0], np.cumsum(tp.cpu().numpy().astype(np.float64))])
        out = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for k, name in enumerate(self.classes):
                out[name] = np.float64(csum[class_off[k + 1]] - csum[class_off[k]]) / np.float64(nimgs[k])
        return out, float(np.mean(list(out.values())))
