"""NumPy restatement of the detection post-processing stage (cim_amd/csrc/detect.hip), fp32 throughout.

It pins what the device computes: tests/test_detect_cpu.py checks it bit for bit against every detect_*.npz golden captured
from the reference, and tests/test_gpu_detect.py checks the device against it where no golden exists (ties, large N).
Every step cites the reference line it restates (paths under the reference checkout).  The one deliberate difference from
the reference: candidates of equal score are visited higher proposal index first (np.argsort(kind="stable")[::-1]); the
reference's default-kind argsort leaves that order to the NumPy build.
"""
import numpy as np

F32 = np.float32


def _pmax(a, b):
    return np.where(a >= b, a, b)          # cython_nms.pyx:28-29: `a if a >= b else b` (not np.maximum: NaN)


def _pmin(a, b):
    return np.where(a <= b, a, b)          # cython_nms.pyx:31-32


def nms(dets, thresh):
    """lib/utils/boxes.py:320-324 + cython_nms.pyx:36-87: keep positions into `dets`, ascending."""
    dets = np.asarray(dets, dtype=F32)
    if dets.shape[0] == 0:
        return []
    thr = F32(thresh)
    x1, y1, x2, y2, scores = (np.ascontiguousarray(dets[:, k]) for k in range(5))
    areas = (x2 - x1 + F32(1)) * (y2 - y1 + F32(1))                                  # :45
    order = np.argsort(scores, kind="stable")[::-1]                                    # :46 (tie rule)
    suppressed = np.zeros(len(order), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _i in range(len(order)):                                                   # :62
            i = order[_i]
            if suppressed[i]:
                continue
            rest = order[_i + 1:]
            rest = rest[~suppressed[rest]]
            if rest.size == 0:
                break
            xx1 = _pmax(x1[i], x1[rest])                                               # :74-77
            yy1 = _pmax(y1[i], y1[rest])
            xx2 = _pmin(x2[i], x2[rest])
            yy2 = _pmin(y2[i], y2[rest])
            w = _pmax(F32(0), xx2 - xx1 + F32(1))                                      # :78-79
            h = _pmax(F32(0), yy2 - yy1 + F32(1))
            inter = w * h                                                              # :80
            ovr = inter / (areas[i] + areas[rest] - inter)                             # :81
            suppressed[rest[ovr >= thr]] = True                                        # :82-83
    return np.where(~suppressed)[0]


def nms_limit(scores, boxes, score_thr, nms_thr, max_det):
    """lib/core/test.py:355-403 in the device's output form: (idx, cls, score, count) with the records in (class, proposal)
    order, score the fp32 input score, count [C] int32."""
    scores = np.asarray(scores, dtype=F32)
    boxes = np.asarray(boxes, dtype=F32)
    C = scores.shape[1]
    per = []
    for j in range(C):
        inds = np.where(scores[:, j] > F32(score_thr))[0]                              # :370
        dets = np.hstack((boxes[inds, :], scores[inds, j][:, None])).astype(F32)       # :371-373
        keep = nms(dets, nms_thr)                                                      # :383
        per.append(inds[np.asarray(keep, dtype=np.int64)])
    if max_det > 0:                                                                    # :396
        image_scores = np.hstack([scores[per[j], j] for j in range(C)])
        if len(image_scores) > max_det:
            image_thresh = np.sort(image_scores)[-max_det]                             # :401
            per = [per[j][scores[per[j], j] >= image_thresh] for j in range(C)]        # :402-404
    idx = np.concatenate(per).astype(np.int32) if per else np.zeros(0, np.int32)
    cls = np.concatenate([np.full(len(p), j, np.int32) for j, p in enumerate(per)])
    sc = scores[idx, cls]
    count = np.array([len(p) for p in per], dtype=np.int32)
    return idx, cls, sc, count


def corloc(scores):
    """lib/core/test.py:336-338: np.argmax per class."""
    scores = np.asarray(scores, dtype=F32)
    return np.array([np.argmax(scores[:, j]) for j in range(scores.shape[1])], dtype=np.int32)
