"""Instance-segmentation evaluation on the device: COCO RLE of masks and COCOeval(..., 'segm') (csrc/segm_eval.hip,
DESIGN.md 4.12).

Replaces pycocotools' mask.encode / decode and COCOeval.evaluate / accumulate / summarize as the reference runs them after
inference (tools/evaluation.py:72-145, 236-241; lib/datasets/json_inference.py:24-55).  Masks are DEVICE tensors; a CPU
tensor is an error (no CPU fallback).  `SegmEvaluator.add_image` only launches work on the current stream, so the masks of
an image may be freed or reused as soon as it returns; `accumulate` returns device tensors, `to_host` copies them.
`poly_masks` fills COCO polygon segmentations into the same packed masks (csrc/poly_fill.hip), so polygon ground truth
needs no pycocotools either.  The reference-shaped wrappers are cim_amd.utils.mask_eval_utils.coco_encode and cim_amd.datasets.json_inference.
"""
import numpy as np
import torch

from . import _lib
from .utils import rle as _rle

MAX_HW, MAX_GT, MAX_T, MAX_R, MAX_A, MAX_M = (_lib.CONSTANTS["CIM_SEGM_MAX_" + k] for k in ("HW", "GT", "T", "R", "A", "M"))
MAX_DT = _lib.CONSTANTS["CIM_DETECT_MAX_N"]                 # detections per (image, category), and maxDets[-1]: the detection stage's limit
MAX_POLY_POINTS = _lib.CONSTANTS["CIM_POLY_MAX_POINTS"]     # dense points of the polygons of one poly_masks call
MAX_POLY_COORD = float(1 << 20)

AREA_LABELS = ("all", "small", "medium", "large")


def _err():
    return _lib.load().cim_last_error().decode()


def _device_tensor(x, what):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.CimHipError("cim_amd.segm_eval: %s must be a CUDA/HIP tensor (no CPU fallback)" % what)
    return x


def _upload(a, dev):
    """Host array -> device tensor without waiting for the stream: pinned staging, asynchronous copy on the current stream."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory().to(dev, non_blocking=True)


def words_of(h, w):
    n = _lib.call("cim_segm_words", int(h), int(w))
    if n < 0:
        raise ValueError(_err())
    return n


def pack_masks(masks, index=None):
    """[n, H, W] bool / uint8 device masks (row-major, nonzero = 1) -> int64 [m, words] bit-packed in COCO's column-major
    pixel order; index (host or device int sequence, optional) picks the m masks to pack."""
    _device_tensor(masks, "masks")
    if masks.dim() != 3:
        raise ValueError("cim_amd.segm_eval: masks must be [n, H, W], got %s" % (tuple(masks.shape),))
    if masks.dtype == torch.bool:
        masks = masks.contiguous().view(torch.uint8)
    elif masks.dtype != torch.uint8:
        raise TypeError("cim_amd.segm_eval: masks must be bool or uint8, got %s" % masks.dtype)
    n_src, h, w = masks.shape
    words = words_of(h, w)
    masks = masks.contiguous()
    idx = None
    if index is None:
        n = n_src
    elif torch.is_tensor(index) and index.is_cuda:
        idx = index.to(masks.device, torch.int64).contiguous().view(-1)
        n = idx.numel()
    else:
        ih = np.asarray(index.cpu() if torch.is_tensor(index) else index, dtype=np.int64).ravel()
        if ih.size and (ih.min() < 0 or ih.max() >= n_src):
            raise IndexError("cim_amd.segm_eval: mask index out of range [0, %d)" % n_src)
        idx = _upload(ih, masks.device)
        n = ih.size
    packed = torch.empty((n, words), dtype=torch.int64, device=masks.device)
    if n:
        _lib.call("cim_segm_pack", masks.data_ptr(), None if idx is None else idx.data_ptr(), n_src, n, h, w, packed.data_ptr(),
                  _lib.stream_ptr())
    return packed


def mask_areas(packed):
    """Pixel count per packed mask (device int32 [n])."""
    n, words = packed.shape
    area = torch.empty(n, dtype=torch.int32, device=packed.device)
    if n:
        _lib.call("cim_segm_area", packed.data_ptr(), n, words, area.data_ptr(), _lib.stream_ptr())
    return area


def rle_counts(packed, h, w):
    """Packed masks -> (host uint32 counts of all masks, back to back, host int64 offsets [n + 1]).  Two phases: run counts
    per mask, one host read for the sizes, then the runs."""
    n = packed.shape[0]
    if packed.shape[1] != words_of(h, w):
        raise ValueError("cim_amd.segm_eval: packed masks have %d words, %d x %d needs %d" % (packed.shape[1], h, w, words_of(h, w)))
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64)
    dev = packed.device
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("cim_segm_rle_count", packed.data_ptr(), n, h, w, lens.data_ptr(), _lib.stream_ptr())
    lh = lens.cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lh)])
    counts = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
    off_d = _upload(off[:-1], dev)
    _lib.call("cim_segm_rle_write", packed.data_ptr(), n, h, w, off_d.data_ptr(), lens.data_ptr(), counts.data_ptr(),
              _lib.stream_ptr())
    return counts.cpu().numpy().view(np.uint32), off


def rle_encode(masks):
    """[n, H, W] device masks -> [{'size': [H, W], 'counts': str}], pycocotools' mask.encode with the counts string decoded."""
    packed = pack_masks(masks)
    h, w = int(masks.shape[1]), int(masks.shape[2])
    counts, off = rle_counts(packed, h, w)
    return [{"size": [h, w], "counts": _rle.counts_to_string(counts[off[i]:off[i + 1]])} for i in range(packed.shape[0])]


def _rle_size_counts(r):
    h, w = (int(v) for v in r["size"])
    c = r["counts"]
    if isinstance(c, (str, bytes)):
        return h, w, _rle.string_to_counts(c)
    return h, w, np.asarray(c, dtype=np.int64).astype(np.uint32)


def rle_decode(rles, device=None, size=None):
    """COCO RLEs (compressed 'counts' strings or uncompressed lists) -> (device int64 [n, words] packed masks, (H, W)).
    All masks must have the same size (`size` when the list is empty)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _lib.CimHipError("cim_amd.segm_eval: rle_decode needs a CUDA/HIP device (no CPU fallback)")
    parts = [_rle_size_counts(r) for r in rles]
    sizes = {(h, w) for h, w, _ in parts}
    if len(sizes) > 1:
        raise ValueError("cim_amd.segm_eval: RLEs of different sizes %s" % sorted(sizes))
    h, w = sizes.pop() if sizes else tuple(size)
    words = words_of(h, w)
    n = len(parts)
    packed = torch.empty((n, words), dtype=torch.int64, device=dev)
    if n == 0:
        return packed, (h, w)
    lens = np.array([p[2].size for p in parts], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    allc = np.concatenate([p[2] for p in parts]).astype(np.uint32) if off[-1] else np.zeros(1, np.uint32)
    ws_bytes = _lib.call("cim_segm_rle_decode_ws_bytes", int(off[-1]))
    if ws_bytes < 0:
        raise ValueError(_err())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    c_d, off_d, len_d = _upload(allc, dev), _upload(off[:-1], dev), _upload(lens.astype(np.int32), dev)
    _lib.call("cim_segm_rle_decode", c_d.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), n, h, w, ws.data_ptr(), packed.data_ptr(),
              _lib.stream_ptr())
    return packed, (h, w)


def _polygon_arrays(polygons_per_annotation, h, w):
    """The polygons of all annotations as the arrays of cim_poly_fill (include/cim_hip.h), after its refusals: (xy f64,
    poly_off, poly_ann, edge_off int32, dense points in all).  O(vertices) host work: the device needs the total before it
    can be launched, and a refusal needs no device round trip."""
    words_of(h, w)                                                       # (refuses h w > CIM_SEGM_MAX_HW)
    flat, sizes, ann = [], [], []
    for i, polys in enumerate(polygons_per_annotation):
        for xy in polys:
            a = np.asarray(xy, dtype=np.float64).ravel()
            if a.size % 2:
                raise ValueError("cim_amd.segm_eval: annotation %d: a polygon of odd length %d" % (i, a.size))
            if a.size < 6:
                raise ValueError("cim_amd.segm_eval: annotation %d: a polygon of %d numbers (need >= 6; pycocotools reads 4 "
                                 "numbers as a box, this does not)" % (i, a.size))
            if not np.isfinite(a).all():
                raise ValueError("cim_amd.segm_eval: annotation %d: a non-finite polygon coordinate" % i)
            if np.abs(a).max() > MAX_POLY_COORD:
                raise ValueError("cim_amd.segm_eval: annotation %d: a polygon coordinate outside [-2^20, 2^20]" % i)
            flat.append(a)
            sizes.append(a.size // 2)
            ann.append(i)
    xy = np.concatenate(flat) if flat else np.zeros(0, np.float64)
    poly_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    r = (5.0 * xy + .5).astype(np.int64)                                 # (int)(5 x + .5), as the device rounds them
    X, Y = r[0::2], r[1::2]
    nxt = np.arange(1, X.size + 1)
    nxt[poly_off[1:] - 1] = poly_off[:-1]                                # a polygon's last edge returns to its first vertex
    steps = np.maximum(np.abs(X[nxt] - X), np.abs(Y[nxt] - Y)) + 1
    edge_off = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
    total = int(edge_off[-1])
    if total > MAX_POLY_POINTS:
        raise ValueError("cim_amd.segm_eval: %d dense points in one call, the kernels take <= %d (CIM_POLY_MAX_POINTS)"
                         % (total, MAX_POLY_POINTS))
    return xy, poly_off.astype(np.int32), np.asarray(ann, np.int32), edge_off.astype(np.int32), total


def poly_masks(polygons_per_annotation, h, w, device=None):
    """COCO polygon segmentations -> device int64 [n, words] packed masks: pycocotools' frPyObjects + merge (annToRLE's
    polygon case) per annotation.  polygons_per_annotation[i] is annotation i's `segmentation` list: polygons [x0, y0, x1,
    y1, ...] in pixel coordinates, filled by COCO's rule and OR-ed (csrc/poly_fill.hip).  ValueError for a
    polygon of odd length or fewer than 6 numbers, a non-finite coordinate or one outside [-2^20, 2^20], h w > 2^22, or
    more than CIM_POLY_MAX_POINTS dense points in the call.  Launches on the current stream; does not synchronise."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _lib.CimHipError("cim_amd.segm_eval: poly_masks needs a CUDA/HIP device (no CPU fallback)")
    h, w = int(h), int(w)
    polys = list(polygons_per_annotation)
    xy, poly_off, poly_ann, edge_off, total = _polygon_arrays(polys, h, w)
    n, n_poly = len(polys), poly_ann.size
    packed = torch.empty((n, words_of(h, w)), dtype=torch.int64, device=dev)
    if n == 0:
        return packed
    ws_bytes = _lib.call("cim_poly_ws_bytes", n_poly, h, w)
    if ws_bytes < 0:
        raise ValueError(_err())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if n_poly:
        xy_d, po_d, pa_d, eo_d = (_upload(a, dev) for a in (xy, poly_off, poly_ann, edge_off))
    else:
        xy_d = po_d = pa_d = eo_d = None
    _lib.call("cim_poly_fill", _lib.ptr(xy_d), _lib.ptr(po_d), _lib.ptr(pa_d), _lib.ptr(eo_d), n_poly, xy.size // 2, total, n, h, w,
              ws.data_ptr(), packed.data_ptr(), _lib.stream_ptr())
    return packed


def record_layout(nd, ng, A, T):
    """Byte offsets of one (image, category) record (csrc/eval_match.h: rec_layout)."""
    L = {"dtm": 0}
    L["score"] = L["dtm"] + 8 * A * T * nd
    L["order"] = L["score"] + 4 * nd
    L["npig"] = L["order"] + 4 * nd
    L["gt_order"] = L["npig"] + 4 * A
    L["dt_ig"] = L["gt_order"] + 4 * A * ng
    L["gt_ig"] = L["dt_ig"] + A * T * nd
    L["bytes"] = (L["gt_ig"] + A * ng + 7) & ~7
    return L


def merge_rounds(start, length, cat):
    """Bottom-up merge schedule of sorted runs (start, length > 0, category; category-major): per round, jobs
    (startA, lenA, lenB) pairing runs 2j, 2j + 1 of each category, until every category is one run."""
    start, length, cat = (np.asarray(a, np.int64) for a in (start, length, cat))
    rounds = []
    while start.size:
        n = start.size
        first = np.r_[True, cat[1:] != cat[:-1]]
        pos = np.arange(n) - np.maximum.accumulate(np.where(first, np.arange(n), 0))
        if pos.max() == 0:
            break
        ia = np.flatnonzero(pos % 2 == 0)
        has_b = np.r_[cat[1:] == cat[:-1], False][ia]
        len_b = np.where(has_b, length[np.minimum(ia + 1, n - 1)], 0)
        rounds.append(np.stack([start[ia], length[ia], len_b], 1))
        start, length, cat = start[ia], length[ia] + len_b, cat[ia]
    return rounds


class SegmEvaluator(object):
    """COCOeval(cocoGt, cocoDt, 'segm') with params (imgIds, catIds, iouThrs, recThrs, areaRng, maxDets), fed one image at a
    time.  Image axis: ascending img_ids; category axis: ascending cat_ids (COCOeval's np.unique of both)."""

    def __init__(self, img_ids, cat_ids, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=(1, 10, 100), device=None):
        self.img_ids = [int(i) for i in np.unique(np.asarray(list(img_ids), dtype=np.int64))]
        self.cat_ids = [int(c) for c in np.unique(np.asarray(list(cat_ids), dtype=np.int64))]
        if not self.cat_ids:
            raise ValueError("cim_amd.segm_eval: no categories")
        self._img_rank = {i: r for r, i in enumerate(self.img_ids)}
        self._cat_index = {c: k for k, c in enumerate(self.cat_ids)}
        # COCOeval Params.setDetParams: the host's fp64 values, never recomputed on the device
        self.iou_thrs = (np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None
                         else np.asarray(iou_thrs, dtype=np.float64).ravel())
        self.rec_thrs = (np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True) if rec_thrs is None
                         else np.asarray(rec_thrs, dtype=np.float64).ravel())
        self.area_rng = np.asarray([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
                                   if area_rng is None else area_rng, dtype=np.float64).reshape(-1, 2)
        self.area_labels = list(AREA_LABELS[:len(self.area_rng)]) if area_rng is None else ["a%d" % i for i in range(len(self.area_rng))]
        self.max_dets = sorted(int(m) for m in max_dets)
        T, R, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.area_rng), len(self.max_dets)
        if not (1 <= T <= MAX_T and 1 <= R <= MAX_R and 1 <= A <= MAX_A and 1 <= M <= MAX_M):
            raise ValueError("cim_amd.segm_eval: need 1 <= T <= %d, R <= %d, A <= %d, M <= %d (T=%d, R=%d, A=%d, M=%d)"
                             % (MAX_T, MAX_R, MAX_A, MAX_M, T, R, A, M))
        if not (1 <= self.max_dets[0] and self.max_dets[-1] <= MAX_DT):
            raise ValueError("cim_amd.segm_eval: maxDets must lie in [1, %d], got %s" % (MAX_DT, self.max_dets))
        if np.any(np.diff(self.rec_thrs) < 0):
            raise ValueError("cim_amd.segm_eval: recall thresholds must be ascending")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._params_d = None
        self._images = {}

    def _params(self):
        if self._params_d is None:
            d = self.device
            self._params_d = (_upload(self.iou_thrs, d), _upload(self.area_rng.ravel(), d), _upload(self.rec_thrs, d),
                              _upload(np.asarray(self.max_dets, np.int32), d))
        return self._params_d

    def _masks(self, x, n, what, size=None, polygons=False):
        """-> (device packed [n, words] or None, (H, W) or None)"""
        if x is None:
            if n:
                raise ValueError("cim_amd.segm_eval: %d %s but no masks" % (n, what))
            return None, None
        if isinstance(x, tuple):                                         # (proposal masks, kept indices)
            props, index = x
            _device_tensor(props, what + " proposal masks")
            idx_len = index.numel() if torch.is_tensor(index) else len(np.asarray(index).ravel())
            if idx_len != n:
                raise ValueError("cim_amd.segm_eval: %d %s, %d indices" % (n, what, idx_len))
            return pack_masks(props, index), (int(props.shape[1]), int(props.shape[2]))
        if torch.is_tensor(x):
            _device_tensor(x, what + " masks")
            if x.dim() != 3 or x.shape[0] != n:
                raise ValueError("cim_amd.segm_eval: %s masks must be [%d, H, W], got %s" % (what, n, tuple(x.shape)))
            return pack_masks(x), (int(x.shape[1]), int(x.shape[2]))
        rles = list(x)
        if len(rles) != n:
            raise ValueError("cim_amd.segm_eval: %d %s, %d RLEs" % (n, what, len(rles)))
        if n == 0:
            return None, None
        is_poly = [isinstance(r, (list, tuple)) for r in rles]
        if not any(is_poly):
            packed, hw = rle_decode(rles, self.device)
            if size is not None and hw != tuple(size):
                raise ValueError("cim_amd.segm_eval: %s RLEs of size %s, asked for %s (H x W must match)" % (what, hw, tuple(size)))
            return packed, hw
        if not polygons:
            raise ValueError("cim_amd.segm_eval: %s must be masks or RLEs (polygons are taken for ground truths only)" % what)
        # polygon lists among the RLEs: the polygons' rows in one launch, the RLEs' rows decoded and copied over theirs
        rest = [j for j in range(n) if not is_poly[j]]
        sizes = {tuple(int(v) for v in rles[j]["size"]) for j in rest} | ({tuple(int(v) for v in size)} if size is not None else set())
        if len(sizes) > 1:
            raise ValueError("cim_amd.segm_eval: %s of different sizes %s (H x W must match)" % (what, sorted(sizes)))
        if not sizes:
            raise ValueError("cim_amd.segm_eval: polygon %s need the image's size=(H, W)" % what)
        h, w = sizes.pop()
        packed = poly_masks([r if p else [] for r, p in zip(rles, is_poly)], h, w, self.device)
        if rest:
            dec, _ = rle_decode([rles[j] for j in rest], self.device)
            packed.index_copy_(0, _upload(np.asarray(rest, np.int64), self.device), dec)
        return packed, (h, w)

    def add_image(self, img_id, gt, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, dt, dt_cat_ids, dt_scores, size=None):
        """One image: ground truths (device masks [G, H, W], or a list of COCO RLEs and / or polygon lists - an annotation's
        `segmentation` as the file stores it) with their category ids, iscrowd flags, annotation `area` fields and annotation
        ids (host sequences); detections (device masks [D, H, W], COCO RLEs, or (device proposal masks [N, H, W], kept
        proposal indices [D])) with category ids (host) and fp32 scores (device tensor or host array).  size = (H, W) of the
        image: what polygons are filled on (needed unless an RLE among the ground truths gives it).
        Ground truths and detections of categories outside cat_ids are left out, as COCOeval does.
        Launches the image's packing, IoU and matching on the current stream; does not synchronise."""
        img_id, gcat, crowd, garea, gids, dcat, scores_d = self._image_fields(img_id, gt_cat_ids, gt_iscrowd, gt_area, gt_ids,
                                                                              dt_cat_ids, dt_scores)
        G, D = gcat.size, dcat.size
        gp, ghw = self._masks(gt, G, "ground truths", size, True)
        dp, dhw = self._masks(dt, D, "detections")
        if ghw is not None and dhw is not None and ghw != dhw:
            raise ValueError("cim_amd.segm_eval: image %d: detection masks %s, ground-truth masks %s (H x W must match)"
                             % (img_id, dhw, ghw))
        hw = ghw or dhw
        info, meta, ndl, ngl, rec_off, pair_off = self._image_groups(img_id, dcat, gcat, crowd, gids)
        if meta is None:
            return
        dev = self.device
        T, A = len(self.iou_thrs), len(self.area_rng)
        ws_bytes = _lib.call("cim_segm_image_ws_bytes", D, G, pair_off)
        if ws_bytes < 0:
            raise ValueError(_err())
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        records = torch.empty(max(rec_off, 8), dtype=torch.uint8, device=dev)
        words = words_of(*hw)
        meta_d = _upload(meta, dev)
        garea_d = _upload(garea, dev) if G else None
        gids_d = _upload(gids, dev) if G else None
        thr_d, rng_d, _, _ = self._params()
        _lib.call("cim_segm_eval_image", _lib.ptr(dp), D, _lib.ptr(gp), G, words, _lib.ptr(scores_d), meta_d.data_ptr(),
                  len(info["groups"]), ndl, ngl, pair_off, _lib.ptr(garea_d), _lib.ptr(gids_d), thr_d.data_ptr(), T,
                  rng_d.data_ptr(), A, ws.data_ptr(), records.data_ptr(), _lib.stream_ptr())
        info["records"] = records

    def _image_fields(self, img_id, gt_cat_ids, gt_iscrowd, gt_area, gt_ids, dt_cat_ids, dt_scores):
        """add_image's checks of the per-annotation and per-detection fields -> (image id, ground-truth category ids, crowd
        flags int32, areas f64, ids int64, detection category ids, device fp32 scores or None)."""
        img_id = int(img_id)
        if img_id not in self._img_rank:
            raise ValueError("cim_amd.segm_eval: image %d is not among the evaluated image ids (COCO.loadRes asserts this)" % img_id)
        if img_id in self._images:
            raise ValueError("cim_amd.segm_eval: image %d added twice" % img_id)
        gcat = np.asarray(gt_cat_ids, dtype=np.int64).ravel()
        G = gcat.size
        crowd = np.asarray(gt_iscrowd).astype(bool).ravel().astype(np.int32)
        garea = np.asarray(gt_area, dtype=np.float64).ravel()
        gids = np.asarray(gt_ids, dtype=np.int64).ravel()
        if not crowd.size == garea.size == gids.size == G:
            raise ValueError("cim_amd.segm_eval: ground-truth fields of different lengths")
        if G > MAX_GT:
            raise ValueError("cim_amd.segm_eval: %d ground truths in image %d, the kernels take <= %d" % (G, img_id, MAX_GT))
        dcat = np.asarray(dt_cat_ids, dtype=np.int64).ravel()
        D = dcat.size
        if torch.is_tensor(dt_scores):
            _device_tensor(dt_scores, "dt_scores")
            if dt_scores.dtype != torch.float32:
                raise TypeError("cim_amd.segm_eval: dt_scores must be float32, got %s" % dt_scores.dtype)
            scores_d = dt_scores.to(self.device).contiguous().view(-1)
            if scores_d.numel() != D:
                raise ValueError("cim_amd.segm_eval: %d detections, %d scores" % (D, scores_d.numel()))
        else:
            sh = np.asarray(dt_scores)
            if sh.size and sh.dtype != np.float32:
                raise TypeError("cim_amd.segm_eval: dt_scores must be float32, got %s" % sh.dtype)
            sh = sh.astype(np.float32).ravel()
            if sh.size != D:
                raise ValueError("cim_amd.segm_eval: %d detections, %d scores" % (D, sh.size))
            if np.isnan(sh).any():
                raise ValueError("cim_amd.segm_eval: NaN score")
            scores_d = _upload(sh, self.device) if D else None
        return img_id, gcat, crowd, garea, gids, dcat, scores_d

    def _image_groups(self, img_id, dcat, gcat, crowd, gids):
        """The image's (image, category) groups: registers the image and returns (its info, the int32 meta array of
        cim_segm_eval_image or None when the image has no group, n_dl, n_gl, record bytes, IoU pairs)."""
        T, A = len(self.iou_thrs), len(self.area_rng)
        kd = np.array([self._cat_index.get(int(c), -1) for c in dcat], np.int64)
        kg = np.array([self._cat_index.get(int(c), -1) for c in gcat], np.int64)
        cats = np.unique(np.concatenate([kd[kd >= 0], kg[kg >= 0]]))
        groups, meta_g, dls, gls = [], [], [], []
        rec_off = pair_off = ndl = ngl = 0
        for k in cats:
            dl, gl = np.flatnonzero(kd == k), np.flatnonzero(kg == k)
            n_det, ng = dl.size, gl.size
            if n_det > MAX_DT:
                raise ValueError("cim_amd.segm_eval: %d detections of category %d in image %d, the kernels take <= %d"
                                 % (n_det, self.cat_ids[k], img_id, MAX_DT))
            nd = min(n_det, self.max_dets[-1])
            nbytes = _lib.call("cim_segm_record_bytes", nd, ng, A, T)
            if nbytes < 0:
                raise ValueError(_err())
            meta_g.append((ndl, n_det, ngl, ng, nd, rec_off, pair_off, 0))
            groups.append((int(k), nd, ng, rec_off))
            dls.append(dl)
            gls.append(gl)
            rec_off += nbytes
            pair_off += nd * ng
            ndl += n_det
            ngl += ng
        if rec_off >= 1 << 31:
            raise ValueError("cim_amd.segm_eval: image %d's records need %d bytes (< 2^31)" % (img_id, rec_off))
        info = {"groups": groups, "gt_ids": gids, "records": None}
        self._images[img_id] = info
        if not groups:
            return info, None, 0, 0, 0, 0
        meta = np.concatenate([np.asarray(meta_g, np.int32).ravel()] + [a.astype(np.int32) for a in dls + gls] + [crowd])
        return info, meta, ndl, ngl, rec_off, pair_off

    def accumulate(self):
        """COCOeval.accumulate: {'precision' [T,R,K,A,M], 'recall' [T,K,A,M], 'scores' [T,R,K,A,M]} fp64 device tensors."""
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng), len(self.max_dets)
        rows = []
        for img_id, info in self._images.items():
            if info["records"] is None:
                continue
            base = info["records"].data_ptr()
            r = self._img_rank[img_id]
            for k, nd, ng, off in info["groups"]:
                rows.append((k, r, base + off, nd, ng))
        rows.sort()
        ent = np.zeros((len(rows), 6), np.int64)
        if rows:
            a = np.asarray(rows, dtype=np.int64)
            ent[:, 0], ent[:, 1], ent[:, 2], ent[:, 4] = a[:, 2], a[:, 3], a[:, 4], a[:, 0]
        first = np.concatenate([[0], np.cumsum(ent[:, 1])])
        ent[:, 3] = first[:-1]
        E = int(first[-1])
        cat_off = first[np.searchsorted(ent[:, 4], np.arange(K + 1), side="left")]
        run = ent[:, 1] > 0
        rounds = merge_rounds(ent[run, 3], ent[run, 1], ent[run, 4])
        ws_bytes = _lib.call("cim_segm_accumulate_ws_bytes", E, K, A, T)
        if ws_bytes < 0:
            raise ValueError(_err())
        dev = self.device
        _, _, rec_d, md_d = self._params()
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ent_d = _upload(ent, dev) if len(rows) else None
        cat_d = _upload(cat_off.astype(np.int64), dev)
        jobs_d = roff_d = None
        if rounds:
            roff = np.concatenate([[0], np.cumsum([len(j) for j in rounds])]).astype(np.int64)
            jobs_d, roff_d = _upload(np.concatenate(rounds).astype(np.int64), dev), _upload(roff, dev)
        out = {"precision": torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev),
               "recall": torch.empty((T, K, A, M), dtype=torch.float64, device=dev),
               "scores": torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)}
        _lib.call("cim_segm_accumulate", _lib.ptr(ent_d), len(rows), E, K, cat_d.data_ptr(), _lib.ptr(jobs_d), _lib.ptr(roff_d),
                  len(rounds), rec_d.data_ptr(), R, md_d.data_ptr(), M, A, T, ws.data_ptr(), out["precision"].data_ptr(),
                  out["recall"].data_ptr(), out["scores"].data_ptr(), _lib.stream_ptr())
        self.eval = out
        return out

    def summarize(self, ev=None):
        """COCOeval.summarize()'s 12 stats (_summarizeDets) from accumulate's results, on the host (12 means)."""
        ev = to_host(ev if ev is not None else self.eval)
        return summarize_stats(ev["precision"], ev["recall"], self.iou_thrs, self.area_labels, self.max_dets)

    def eval_imgs(self):
        """Host copy of COCOeval.evalImgs: a list over (category, area range, image) in that nesting order, None where the
        (image, category) has neither ground truth nor detection.  dtIds are the detections' positions in add_image's
        list, gtIds the annotation ids, dtMatches the matched annotation id (0 = none)."""
        T, A = len(self.iou_thrs), len(self.area_rng)
        K, I = len(self.cat_ids), len(self.img_ids)
        out = [None] * (K * A * I)
        for img_id, info in self._images.items():
            if info["records"] is None:
                continue
            h = info["records"].cpu().numpy()
            i = self._img_rank[img_id]
            for k, nd, ng, off in info["groups"]:
                L = record_layout(nd, ng, A, T)
                sl = lambda key, dt, cnt: np.frombuffer(h[off + L[key]:off + L[key] + cnt * np.dtype(dt).itemsize].tobytes(), dt)
                dtm = sl("dtm", np.int64, A * T * nd).reshape(A, T, nd)
                dtig = sl("dt_ig", np.uint8, A * T * nd).reshape(A, T, nd)
                gord = sl("gt_order", np.int32, A * ng).reshape(A, ng)
                gig = sl("gt_ig", np.uint8, A * ng).reshape(A, ng)
                order = sl("order", np.int32, nd)
                score = sl("score", np.float32, nd)
                for a in range(A):
                    out[(k * A + a) * I + i] = {
                        "image_id": img_id, "category_id": self.cat_ids[k], "aRng": list(self.area_rng[a]),
                        "maxDet": self.max_dets[-1], "dtIds": order.astype(np.int64), "gtIds": info["gt_ids"][gord[a]],
                        "dtMatches": dtm[a].copy(), "dtScores": score.astype(np.float64), "gtIgnore": gig[a].astype(bool),
                        "dtIgnore": dtig[a].astype(bool)}
        return out


def to_host(ev):
    """accumulate()'s device tensors -> NumPy fp64 arrays (one copy each)."""
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in ev.items()}


def summarize_stats(precision, recall, iou_thrs, area_labels, max_dets):
    """COCOeval._summarizeDets: stats[12] from host precision [T,R,K,A,M] and recall [T,K,A,M] (-1 where empty)."""
    def one(ap, iou_thr=None, area="all", md=100):
        aind = [i for i, a in enumerate(area_labels) if a == area]
        mind = [i for i, m in enumerate(max_dets) if m == md]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == np.asarray(iou_thrs))[0]]
        s = s[:, :, :, aind, mind] if ap else s[:, :, aind, mind]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    md = list(max_dets) + [None] * 3
    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5, md=md[2])
    stats[2] = one(1, iou_thr=.75, md=md[2])
    stats[3] = one(1, area="small", md=md[2])
    stats[4] = one(1, area="medium", md=md[2])
    stats[5] = one(1, area="large", md=md[2])
    stats[6] = one(0, md=md[0])
    stats[7] = one(0, md=md[1])
    stats[8] = one(0, md=md[2])
    stats[9] = one(0, area="small", md=md[2])
    stats[10] = one(0, area="medium", md=md[2])
    stats[11] = one(0, area="large", md=md[2])
    return stats
