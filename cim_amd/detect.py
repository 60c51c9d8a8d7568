"""Detection post-processing on the device: per-class score threshold, greedy box NMS and the per-image detection limit,
and the per-class argmax of CorLoc (csrc/detect.hip).

Replaces the host loops of lib/core/test.py:320-420 and lib/utils/mask_eval_utils.py:6-108 over the
compiled lib/utils/cython_nms.pyx.  Takes and returns DEVICE tensors and launches on the current stream; a CPU tensor is an
error (no CPU fallback).  `to_host` / `corloc_host` make the one device-to-host copy a caller of host results needs.
`postprocess` / `softvote_to_host` / `box_voting` are the same stage under TEST.SOFT_NMS / TEST.BBOX_VOTE.
The reference-shaped wrappers are cim_amd.core.test, cim_amd.utils.mask_eval_utils and cim_amd.utils.boxes.
"""
import collections

import numpy as np
import torch

from . import _lib

MAX_N = _lib.CONSTANTS["CIM_DETECT_MAX_N"]
MAX_IMAGES = _lib.CONSTANTS["CIM_BATCH_DETECT_MAX_IMAGES"]         # images of one batched call

# device results: views of ONE int32 buffer [total | count_per_class[C] | det[C * N][3]] so that the host copy is one slice
Detections = collections.namedtuple("Detections", "buf num_classes max_det")


def _scores(scores, num_classes=None):
    if not torch.is_tensor(scores) or not scores.is_cuda:
        raise _lib.CimHipError("cim_amd.detect: scores must be a CUDA/HIP tensor (no CPU fallback)")
    if scores.dtype != torch.float32:
        raise TypeError("cim_amd.detect: scores must be float32 (the reference compares fp32 scores), got %s" % scores.dtype)
    if scores.dim() != 2:
        raise ValueError("cim_amd.detect: scores must be [N, C], got %s" % (tuple(scores.shape),))
    n, c = scores.shape
    C = c if num_classes is None else int(num_classes)
    if not 1 <= n <= MAX_N:
        raise ValueError("cim_amd.detect: N = %d proposals, the kernels take 1 <= N <= %d" % (n, MAX_N))
    if not 1 <= C <= c:
        raise ValueError("cim_amd.detect: %d classes asked of a [%d, %d] score array" % (C, n, c))
    if scores.stride(1) != 1 or scores.stride(0) < C:
        scores = scores.contiguous()
    return scores, n, C


def _boxes(boxes, n, device):
    if not torch.is_tensor(boxes) or not boxes.is_cuda:
        raise _lib.CimHipError("cim_amd.detect: boxes must be a CUDA/HIP tensor (no CPU fallback)")
    if tuple(boxes.shape) != (n, 4):
        raise ValueError("cim_amd.detect: boxes must be [%d, 4], got %s" % (n, tuple(boxes.shape)))
    if boxes.device != device:
        raise ValueError("cim_amd.detect: boxes on %s, scores on %s" % (boxes.device, device))
    return boxes.to(torch.float32).contiguous()


def nms_limit(scores, boxes, score_thr=1e-5, nms_thr=0.3, max_det=100, num_classes=None):
    """scores [N, C] f32, boxes [N, 4] f32 (x1, y1, x2, y2), both on the device.  Per class c < num_classes (default C):
    proposals with scores[:, c] > score_thr, greedy NMS at nms_thr; then, if max_det > 0 and more than max_det boxes are
    kept over all classes, only those scoring >= the max_det-th largest kept score.  Returns Detections (device buffer; see
    `to_host`).  Launches on the current stream, does not synchronise."""
    scores, n, C = _scores(scores, num_classes)
    boxes = _boxes(boxes, n, scores.device)
    ws_bytes = _lib.call("cim_detect_ws_bytes", n, C)
    if ws_bytes < 0:
        raise ValueError(_lib.load().cim_last_error().decode())
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=scores.device)
    buf = torch.empty(1 + C + 3 * C * n, dtype=torch.int32, device=scores.device)
    base = buf.data_ptr()
    _lib.call("cim_detect_nms_limit", scores.data_ptr(), scores.stride(0), boxes.data_ptr(), n, C, float(score_thr),
              float(nms_thr), int(max_det), ws.data_ptr(), base + 4 * (1 + C), base + 4, base, _lib.stream_ptr())
    return Detections(buf, C, int(max_det))


def to_host(det):
    """Detections -> NumPy (idx int64 [T], cls int32 [T], score f32 [T], count_per_class int32 [C]), records in (class,
    proposal) order.  One device-to-host copy of the header and the first max(max_det, 0) records (all of them when there
    is no limit); a second only when ties at the limit's threshold keep more than max_det."""
    C = det.num_classes
    head = 1 + C
    cap = (det.buf.numel() - head) // 3
    first = cap if det.max_det <= 0 else min(cap, det.max_det)
    h = det.buf[:head + 3 * first].cpu().numpy()
    total = int(h[0])
    if total > first:
        h = np.concatenate([h, det.buf[head + 3 * first:head + 3 * total].cpu().numpy()])
    rec = h[head:head + 3 * total].reshape(total, 3)
    return (rec[:, 0].astype(np.int64), rec[:, 1].copy(), rec[:, 2].view(np.float32).copy(), h[1:head].copy())


def _batch_parts(x, what):
    """A per-image list or one concatenated array - device tensors or NumPy arrays - as (parts, rows per part); float32 is
    demanded of scores here, before anything is uploaded."""
    parts = list(x) if isinstance(x, (list, tuple)) else [x]
    if not parts:
        raise ValueError("cim_amd.detect: no images")
    for a in parts:
        if torch.is_tensor(a) and not a.is_cuda:
            raise _lib.CimHipError("cim_amd.detect: %s must be CUDA/HIP tensors or NumPy arrays (no CPU fallback)" % what)
    parts = [a if torch.is_tensor(a) else np.asarray(a) for a in parts]
    if what == "scores":
        for a in parts:
            if a.dtype not in (torch.float32, np.float32):
                raise TypeError("cim_amd.detect: scores must be float32 (the reference compares fp32 scores), got %s" % a.dtype)
    return parts, [int(a.shape[0]) for a in parts]


def _batch_cat(parts):
    """The parts back to back as ONE device tensor."""
    if all(torch.is_tensor(a) for a in parts):
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    host = [a.cpu().numpy() if torch.is_tensor(a) else a for a in parts]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(host, 0))).to(_device())


def _per_image(x, B, cols, dtype, what, dev):
    """Optional [B, cols] per-image argument (NumPy or device tensor) -> contiguous device tensor, or None."""
    if x is None:
        return None
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise _lib.CimHipError("cim_amd.detect: %s must be a CUDA/HIP tensor or a NumPy array (no CPU fallback)" % what)
        t = x.to(dev, dtype).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype={torch.float32: np.float32, torch.uint8: np.uint8}[dtype])).to(dev)
    if tuple(t.shape) != (B, cols):
        raise ValueError("cim_amd.detect: %s must be [%d, %d], got %s" % (what, B, cols, tuple(t.shape)))
    return t


def _image_bytes(n, C):
    """Workspace + output bytes one image of n proposals adds to a batched call (include/cim_hip.h; alignment aside)."""
    W = (n + 63) // 64
    return n * W * 8 + C * W * 8 + 9 * C * n * 4 + 28 + 4 * (1 + C)


def _chunks(row_off, C, ws_budget_bytes):
    """Consecutive images [i0, i1) per library call: workspace + output within the budget, the library's limits on B and
    3 * C * sum N."""
    B = len(row_off) - 1
    cost = np.array([_image_bytes(int(n), C) for n in np.diff(row_off)], dtype=np.int64)
    if cost.max() + 4096 > ws_budget_bytes:
        raise ValueError("cim_amd.detect: ws_budget_bytes = %d does not hold one image (%d bytes)" % (ws_budget_bytes, cost.max() + 4096))
    chunks, i0 = [], 0
    while i0 < B:
        i1, used = i0, 4096
        while (i1 < B and i1 - i0 < MAX_IMAGES and used + cost[i1] <= ws_budget_bytes
               and 3 * C * (row_off[i1 + 1] - row_off[i0]) < 2 ** 31):
            used += cost[i1]
            i1 += 1
        if i1 == i0:
            raise ValueError("cim_amd.detect: image %d: 3 * C * N reaches 2^31" % i0)
        chunks.append((i0, i1))
        i0 = i1
    return chunks


def nms_limit_batch(scores, boxes, score_thr=1e-5, nms_thr=0.3, max_det=100, num_classes=None, area_bounds=None,
                    class_mask=None, ws_budget_bytes=1 << 30):
    """`nms_limit` for many images in a few launches (csrc/detect.hip's ragged batch form).

    scores / boxes: a list of per-image [N_b, C] / [N_b, 4] arrays (device tensors or NumPy), or scores = (concatenated
    [sum N, C], row_off [B + 1]) with boxes the concatenated [sum N, 4].  One score_thr, nms_thr, max_det for all images.
    area_bounds [B, 2] f32 = (lo_b, hi_b): TEST.PROPOSAL_FILTER - a proposal whose (x2 - x1) * (y2 - y1) is > hi_b or < lo_b
    scores 0 in every class (tools/evaluation.py:108-115; the caller passes float32(0.00002 * area), float32(0.85 * area)).
    class_mask [B, C] u8: classes whose records are returned, applied AFTER the limit over all classes.

    The images are split into chunks whose workspace plus output fits ws_budget_bytes (at most MAX_IMAGES images each); each
    chunk is one library call and one device-to-host copy of its header and records (a second only when ties at the limit
    keep more than max_det in an image, or without a limit).  Launches on the current stream.  Returns host arrays
    (image int64 [T], idx int64 [T], cls int32 [T], score f32 [T], count int32 [B, C]), records in (image, class, proposal)
    order."""
    if isinstance(scores, tuple) and len(scores) == 2 and np.ndim(scores[1]) == 1 and np.ndim(scores[0]) == 2:
        sp, _ = _batch_parts(scores[0], "scores")
        bp, _ = _batch_parts(boxes, "boxes")
        row_off = np.asarray(scores[1].cpu() if torch.is_tensor(scores[1]) else scores[1], dtype=np.int64)
    else:
        sp, rows = _batch_parts(scores, "scores")
        bp, brows = _batch_parts(boxes, "boxes")
        if rows != brows:
            raise ValueError("cim_amd.detect: scores and boxes disagree on the proposals per image")
        row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    sc, bx = _batch_cat(sp), _batch_cat(bp)
    if sc.dim() != 2:
        raise ValueError("cim_amd.detect: scores must be [sum N, C], got %s" % (tuple(sc.shape),))
    total_n, cols = sc.shape
    C = cols if num_classes is None else int(num_classes)
    if not 1 <= C <= cols:
        raise ValueError("cim_amd.detect: %d classes asked of a [%d, %d] score array" % (C, total_n, cols))
    B = row_off.size - 1
    n_b = np.diff(row_off)
    if B < 1 or row_off[0] != 0 or row_off[-1] != total_n or n_b.min() < 1 or n_b.max() > MAX_N:
        raise ValueError("cim_amd.detect: row_off must run from 0 to %d with 1 <= N_b <= %d proposals per image" % (total_n, MAX_N))
    if tuple(bx.shape) != (total_n, 4) or bx.device != sc.device:
        raise ValueError("cim_amd.detect: boxes must be [%d, 4] on %s, got %s on %s" % (total_n, sc.device, tuple(bx.shape), bx.device))
    if sc.stride(1) != 1 or sc.stride(0) < C:
        sc = sc.contiguous()
    bx = bx.to(torch.float32).contiguous()
    dev = sc.device
    bounds = _per_image(area_bounds, B, 2, torch.float32, "area_bounds", dev)
    cmask = _per_image(class_mask, B, C, torch.uint8, "class_mask", dev)
    max_det = int(max_det)

    chunks = _chunks(row_off, C, ws_budget_bytes)

    out_img, out_idx, out_cls, out_sc = [], [], [], []
    count = np.zeros((B, C), np.int32)
    for i0, i1 in chunks:
        nb, r0, r1 = i1 - i0, int(row_off[i0]), int(row_off[i1])
        ro_h = np.ascontiguousarray(row_off[i0:i1 + 1] - r0, dtype=np.int32)
        ws_bytes = _lib.call("cim_batch_detect_ws_bytes", ro_h.ctypes.data, nb, C)
        if ws_bytes < 0:
            raise ValueError(_lib.load().cim_last_error().decode())
        ro_d = torch.from_numpy(ro_h).pin_memory().to(dev, non_blocking=True)
        ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
        head = nb * (1 + C)
        cap = C * (r1 - r0)
        buf = torch.empty(head + 3 * cap, dtype=torch.int32, device=dev)          # [total[nb] | count[nb, C] | det[cap][3]]
        s_c, b_c = sc[r0:r1], bx[r0:r1]
        base = buf.data_ptr()
        _lib.call("cim_batch_detect_nms_limit", s_c.data_ptr(), sc.stride(0), b_c.data_ptr(), ro_d.data_ptr(), ro_h.ctypes.data,
                  nb, C, float(score_thr), float(nms_thr), max_det, None if bounds is None else bounds[i0:i1].data_ptr(),
                  None if cmask is None else cmask[i0:i1].data_ptr(), ws.data_ptr(), base + 4 * head, base + 4 * nb, base,
                  _lib.stream_ptr())
        first = min(cap, nb * max_det) if max_det > 0 else 0
        h = buf[:head + 3 * first].cpu().numpy()
        tot = h[:nb].astype(np.int64)
        if tot.min() < 0:
            raise _lib.CimHipError("cim_amd.detect: the device's row_off disagrees with the host's")
        T = int(tot.sum())
        if T > first:
            h = np.concatenate([h, buf[head + 3 * first:head + 3 * T].cpu().numpy()])
        rec = h[head:head + 3 * T].reshape(T, 3)
        count[i0:i1] = h[nb:head].reshape(nb, C)
        out_img.append(np.repeat(np.arange(i0, i1, dtype=np.int64), tot))
        out_idx.append(rec[:, 0].astype(np.int64))
        out_cls.append(rec[:, 1].copy())
        out_sc.append(rec[:, 2].view(np.float32).copy())
    return (np.concatenate(out_img), np.concatenate(out_idx), np.concatenate(out_cls), np.concatenate(out_sc), count)


def corloc(scores, num_classes=None):
    """Per class np.argmax(scores[:, c]) (the first maximum, the first NaN if any): device int32 [C, 2] = (proposal,
    score bit pattern)."""
    scores, n, C = _scores(scores, num_classes)
    out = torch.empty((C, 2), dtype=torch.int32, device=scores.device)
    _lib.call("cim_detect_corloc", scores.data_ptr(), scores.stride(0), n, C, out.data_ptr(), _lib.stream_ptr())
    return out


def corloc_host(scores, num_classes=None):
    """corloc + its one device-to-host copy: (idx int64 [C], score f32 [C])."""
    h = corloc(scores, num_classes).cpu().numpy()
    return h[:, 0].astype(np.int64), h[:, 1].view(np.float32).copy()


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def device_inputs(scores, boxes, boxes_on_device=True):
    """scores / boxes of the reference-shaped wrappers - device tensors (as im_detect_all returns them) or NumPy arrays -
    as (device scores f32, device boxes f32 (None unless boxes_on_device), host boxes f32).  Boxes are taken in fp32, as the reference's
    dets_j.astype(np.float32) does; scores must already be fp32 (the reference thresholds them before that cast)."""
    if torch.is_tensor(scores):
        if not scores.is_cuda:
            raise _lib.CimHipError("cim_amd.detect: scores must be a CUDA/HIP tensor or a NumPy array (no CPU fallback)")
        dev = scores.device
    else:
        scores = np.asarray(scores)
        if scores.dtype != np.float32:
            raise TypeError("cim_amd.detect: scores must be float32, got %s" % scores.dtype)
        dev = _device()
        scores = torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    if torch.is_tensor(boxes):
        if not boxes.is_cuda:
            raise _lib.CimHipError("cim_amd.detect: boxes must be a CUDA/HIP tensor or a NumPy array (no CPU fallback)")
        boxes_d = boxes.to(dev, torch.float32).contiguous()
        boxes_h = boxes_d.cpu().numpy()
        boxes_d = boxes_d if boxes_on_device else None
    else:
        boxes_h = np.ascontiguousarray(np.asarray(boxes), dtype=np.float32)
        boxes_d = torch.from_numpy(boxes_h).to(dev) if boxes_on_device else None
    return scores, boxes_d, boxes_h


# ---------------------------------------------------------------- soft-NMS and box voting
SOFT_NMS_METHODS = {"hard": _lib.CONSTANTS["CIM_SOFTVOTE_NMS_SOFT_HARD"], "linear": _lib.CONSTANTS["CIM_SOFTVOTE_NMS_SOFT_LINEAR"],
                    "gaussian": _lib.CONSTANTS["CIM_SOFTVOTE_NMS_SOFT_GAUSSIAN"]}
SCORING_METHODS = {m: _lib.CONSTANTS["CIM_SOFTVOTE_SCORE_" + m]
                   for m in ("ID", "AVG", "IOU_AVG", "QUASI_SUM", "GENERALIZED_AVG", "TEMP_AVG")}

# device results: `buf` int32 [total | empty votes | count_per_class[C] | det[C * N][3]], `boxes` f32 [C * N, 4]
SoftDetections = collections.namedtuple("SoftDetections", "buf boxes num_classes max_det")


def _scoring(method):
    if method not in SCORING_METHODS:
        raise NotImplementedError("Unknown scoring method {}".format(method))          # boxes.py:313-315
    return SCORING_METHODS[method]


def postprocess(scores, boxes, score_thr=1e-5, nms_thr=0.3, max_det=100, soft_nms=None, box_vote=None, num_classes=None):
    """`nms_limit` with TEST.SOFT_NMS and / or TEST.BBOX_VOTE (lib/core/test.py:378-396), on the device.

    soft_nms: None (the greedy pass of `nms_limit`) or dict(method='hard' | 'linear' | 'gaussian', sigma=0.5,
    min_score=0.0001): per class the reference's swap-based loop on the candidates in ascending proposal order; records come
    in SELECTION order with the DECAYED scores, bit for bit the reference's.  box_vote: None or dict(thresh=0.8,
    scoring_method='ID', beta=1.0): every kept box becomes the score-weighted mean of the class's candidates overlapping it
    by >= thresh, its score follows scoring_method; needs score_thr >= 0.  The limit over all classes comes last, on the
    decayed / re-scored values.  Returns SoftDetections (device buffers; see `softvote_to_host`).  Launches on the current
    stream, does not synchronise."""
    kind, sigma, min_score = _lib.CONSTANTS["CIM_SOFTVOTE_NMS_GREEDY"], 0.5, 0.0001
    if soft_nms is not None:
        method = soft_nms.get("method", "linear")
        assert method in SOFT_NMS_METHODS, "Unknown soft_nms method: {}".format(method)  # boxes.py:335
        kind, sigma, min_score = SOFT_NMS_METHODS[method], soft_nms.get("sigma", 0.5), soft_nms.get("min_score", 0.0001)
    vote, vote_thr, scoring, beta = 0, 0.8, 0, 1.0
    if box_vote is not None:
        vote, vote_thr = 1, box_vote.get("thresh", 0.8)
        scoring, beta = _scoring(box_vote.get("scoring_method", "ID")), box_vote.get("beta", 1.0)
        if not np.float32(score_thr) >= 0:
            raise ValueError("cim_amd.detect: box voting needs score_thr >= 0 (the voters' scores are the weights of a mean), "
                             "got %r" % (score_thr,))
    scores, n, C = _scores(scores, num_classes)
    boxes = _boxes(boxes, n, scores.device)
    ws_bytes = _lib.call("cim_softvote_ws_bytes", n, C)
    if ws_bytes < 0:
        raise ValueError(_lib.load().cim_last_error().decode())
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=scores.device)
    buf = torch.empty(2 + C + 3 * C * n, dtype=torch.int32, device=scores.device)
    out_boxes = torch.empty((C * n, 4), dtype=torch.float32, device=scores.device)
    base = buf.data_ptr()
    _lib.call("cim_softvote_postprocess", scores.data_ptr(), scores.stride(0), boxes.data_ptr(), n, C, float(score_thr),
              float(nms_thr), kind, float(sigma), float(min_score), vote, float(vote_thr), scoring, float(beta), int(max_det),
              ws.data_ptr(), base + 4 * (2 + C), out_boxes.data_ptr(), base + 8, base, base + 4, _lib.stream_ptr())
    return SoftDetections(buf, out_boxes, C, int(max_det))


def softvote_to_host(det):
    """SoftDetections -> NumPy (idx int64 [T], cls int32 [T], score f32 [T], count_per_class int32 [C], boxes f32 [T, 4]),
    records in class order, within a class in the reference's.  One device-to-host copy of the header, the first
    max(max_det, 0) records and their boxes (all of them without a limit); a second only when ties at the limit's threshold
    keep more than max_det.  Raises ZeroDivisionError, as the reference's np.average does, if a voted box had no voter."""
    C = det.num_classes
    head = 2 + C
    cap = (det.buf.numel() - head) // 3
    first = cap if det.max_det <= 0 else min(cap, det.max_det)
    h = torch.cat([det.buf[:head + 3 * first], det.boxes[:first].reshape(-1).view(torch.int32)]).cpu().numpy()
    total = int(h[0])
    if int(h[1]):
        raise ZeroDivisionError("Weights sum to zero, can't be normalized (%d voted boxes had no voter)" % int(h[1]))
    rec, bx = h[head:head + 3 * first], h[head + 3 * first:]
    if total > first:
        more = torch.cat([det.buf[head + 3 * first:head + 3 * total],
                          det.boxes[first:total].reshape(-1).view(torch.int32)]).cpu().numpy()
        rec, bx = np.concatenate([rec, more[:3 * (total - first)]]), np.concatenate([bx, more[3 * (total - first):]])
    rec = rec[:3 * total].reshape(total, 3)
    return (rec[:, 0].astype(np.int64), rec[:, 1].copy(), rec[:, 2].view(np.float32).copy(), h[2:head].copy(),
            bx[:4 * total].view(np.float32).reshape(total, 4).copy())


def box_voting(top_boxes, all_boxes, all_scores, thresh, scoring_method="ID", beta=1.0):
    """lib/utils/boxes.py:268-317 for arbitrary top boxes: top_boxes [T, 4], all_boxes [K, 4], all_scores [K], device f32
    tensors.  Returns device (boxes [T, 4], scores [T] - written unless scoring_method is 'ID' -, empty int32 [1]: top boxes
    without a voter, which the reference answers with ZeroDivisionError)."""
    scoring = _scoring(scoring_method)
    for t in (top_boxes, all_boxes, all_scores):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.CimHipError("cim_amd.detect: box_voting takes CUDA/HIP tensors (no CPU fallback)")
    T, K = int(top_boxes.shape[0]), int(all_boxes.shape[0])
    if tuple(top_boxes.shape) != (T, 4) or tuple(all_boxes.shape) != (K, 4) or tuple(all_scores.shape) != (K,) or T < 1 or K < 1:
        raise ValueError("cim_amd.detect: box_voting takes top_boxes [T, 4], all_boxes [K, 4], all_scores [K] with T, K >= 1")
    top = top_boxes.to(torch.float32).contiguous()
    allb = all_boxes.to(torch.float32).contiguous()
    alls = all_scores.to(torch.float32).contiguous()
    out_b = torch.empty((T, 4), dtype=torch.float32, device=top.device)
    out_s = torch.zeros(T, dtype=torch.float32, device=top.device)
    empty = torch.empty(1, dtype=torch.int32, device=top.device)
    _lib.call("cim_softvote_vote", allb.data_ptr(), alls.data_ptr(), K, top.data_ptr(), T, float(thresh), scoring, float(beta),
              out_b.data_ptr(), out_s.data_ptr(), empty.data_ptr(), _lib.stream_ptr())
    return out_b, out_s, empty
