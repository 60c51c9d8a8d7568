"""NumPy restatement of soft-NMS, box voting and their limit (cim_amd/csrc/detect.hip).

It pins what the device computes: tests/test_softvote_cpu.py checks it against every softvote_*.npz golden captured from
the reference - soft-NMS bit for bit, voting within the derived bound -, and tests/test_gpu_softvote.py checks the device
against it where no golden exists.  Every step cites the reference line it restates (paths under the reference checkout).

Soft-NMS comes in two forms that must agree: `soft_nms_loop`, the pyx's loop row by row, and `soft_nms`, vectorised per
selection step with the swap-with-last removal restated as a partition (the form of the kernel).  Box voting is evaluated
in float64: the reference's fp32 sums and the device's double sums are both compared against it.
"""
import numpy as np

from detect_np import _pmax, _pmin, nms

F32 = np.float32
METHODS = {"hard": 0, "linear": 1, "gaussian": 2}                       # boxes.py:334
SCORING = ("ID", "AVG", "IOU_AVG", "QUASI_SUM", "GENERALIZED_AVG", "TEMP_AVG")
GAUSS_ARGS = None                   # a list: every fp32 argument the gaussian weight is evaluated at is appended (capture)


def _weight(ov, nt, sigma, method):
    """cython_nms.pyx:174-185 on fp32 arrays: the weight as the C float the pyx assigns it to."""
    if method == 1:
        return np.where(ov > nt, F32(1) - ov, F32(1)).astype(F32)
    if method == 2:
        arg = (-(ov * ov) / sigma).astype(F32)                          # an fp32 expression ...
        if GAUSS_ARGS is not None:
            GAUSS_ARGS.append(arg)
        return np.exp(arg.astype(np.float64)).astype(F32)               # ... np.exp in double, rounded to the C float
    return np.where(ov > nt, F32(0), F32(1)).astype(F32)


def _overlap(t, b):
    """cython_nms.pyx:166-172 / cython_bbox.pyx:52-72: (guard iw > 0 and ih > 0, ov where the guard holds), fp32.
    t [4] the selected / top box, b [n, 4]."""
    one = F32(1)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    iw = _pmin(t[2], b[:, 2]) - _pmax(t[0], b[:, 0]) + one
    ih = _pmin(t[3], b[:, 3]) - _pmax(t[1], b[:, 1]) + one
    ua = (t[2] - t[0] + one) * (t[3] - t[1] + one) + area - iw * ih
    guard = (iw > 0) & (ih > 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ov = (iw * ih / ua).astype(F32)
    return guard, ov


def soft_nms_loop(dets, sigma=0.5, nt=0.3, threshold=0.001, method=1):
    """cython_nms.pyx:98-203 row by row.  Returns (boxes[:N], inds[:N])."""
    boxes = np.array(dets, dtype=F32)
    sigma, nt, threshold = F32(sigma), F32(nt), F32(threshold)
    N = boxes.shape[0]
    inds = np.arange(N)
    for i in range(N):                                                  # (the bound is the initial N: rows past the
        if i >= N:                                                      # shrunken N only swap with themselves)
            break
        maxpos = i + int(np.argmax(boxes[i:N, 4]))                      # :128-132: first position of the maximum
        boxes[[i, maxpos]] = boxes[[maxpos, i]]                         # :135-148
        inds[[i, maxpos]] = inds[[maxpos, i]]
        t = boxes[i, :4].copy()
        pos = i + 1
        while pos < N:                                                  # :159-201
            guard, ov = _overlap(t, boxes[pos:pos + 1, :4])
            if guard[0]:
                w = _weight(ov, nt, sigma, method)[0]
                boxes[pos, 4] = w * boxes[pos, 4]
                if boxes[pos, 4] < threshold:                           # :191, inside the overlap branch
                    boxes[pos] = boxes[N - 1]
                    inds[pos] = inds[N - 1]
                    N -= 1
                    pos -= 1
            pos += 1
    return boxes[:N], inds[:N]


def soft_nms(dets, sigma=0.5, nt=0.3, threshold=0.001, method=1):
    """The same result, one vectorised pass per selection step.  Every row behind i is examined exactly once against the
    selected box, so scores and survival come first; the removal is then a partition: with M survivors, the holes (removed
    rows among the first M, ascending) take the survivors behind the first M in descending order."""
    boxes = np.array(dets, dtype=F32)
    sigma, nt, threshold = F32(sigma), F32(nt), F32(threshold)
    N = boxes.shape[0]
    inds = np.arange(N)
    i = 0
    while i < N:
        maxpos = i + int(np.argmax(boxes[i:N, 4]))
        boxes[[i, maxpos]] = boxes[[maxpos, i]]
        inds[[i, maxpos]] = inds[[maxpos, i]]
        lo = i + 1
        if lo < N:
            guard, ov = _overlap(boxes[i, :4].copy(), boxes[lo:N, :4])
            s = boxes[lo:N, 4]
            with np.errstate(invalid="ignore", over="ignore"):
                s = s.copy()
                s[guard] = _weight(ov[guard], nt, sigma, method) * s[guard]          # (only examined rows reach the weight)
            boxes[lo:N, 4] = s
            surv = ~(guard & (s < threshold))
            M = int(surv.sum())
            holes = np.where(~surv[:M])[0]
            fill = np.where(surv[M:])[0][::-1] + M
            boxes[lo + holes] = boxes[lo + fill]
            inds[lo + holes] = inds[lo + fill]
            N = lo + M
        i += 1
    return boxes[:N], inds[:N]


def bbox_overlaps(top, allb):
    """cython_bbox.pyx:32-73 in fp32: [T, K], 0 where the guards fail."""
    out = np.zeros((top.shape[0], allb.shape[0]), F32)
    for k in range(top.shape[0]):
        guard, ov = _overlap(top[k], allb)
        out[k] = np.where(guard, ov, F32(0))
    return out


def box_voting(top_dets, all_dets, thresh, scoring_method="ID", beta=1.0):
    """boxes.py:268-317 with every sum in float64.  Returns (out [T, 5] float64, votes [T] int64 - the vote set sizes,
    sets - the vote sets).  The overlaps and the `>= thresh` test are the reference's fp32 ones."""
    top = np.asarray(top_dets, dtype=F32)
    alld = np.asarray(all_dets, dtype=F32)
    out = top.astype(np.float64)
    ovs = bbox_overlaps(top[:, :4], alld[:, :4])
    votes, sets = np.zeros(top.shape[0], np.int64), []
    for k in range(top.shape[0]):
        sel = np.where(ovs[k] >= thresh)[0]                              # :281 (fp32 overlap against the Python float)
        sets.append(sel)
        votes[k] = len(sel)
        ws = alld[sel, 4].astype(np.float64)
        if len(sel) == 0 or ws.sum() == 0:
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        out[k, :4] = (alld[sel, :4].astype(np.float64) * ws[:, None]).sum(0) / ws.sum()
        if scoring_method == "ID":
            pass
        elif scoring_method == "TEMP_AVG":
            P = np.vstack((ws, 1.0 - ws))
            X = np.log(P / P.max(axis=0))
            X_exp = np.exp(X / beta)
            out[k, 4] = (X_exp / X_exp.sum(axis=0))[0].mean()
        elif scoring_method == "AVG":
            out[k, 4] = ws.mean()
        elif scoring_method == "IOU_AVG":
            o = ovs[k, sel].astype(np.float64)
            out[k, 4] = (ws * o).sum() / o.sum()
        elif scoring_method == "GENERALIZED_AVG":
            out[k, 4] = np.mean(ws ** beta) ** (1.0 / beta)
        elif scoring_method == "QUASI_SUM":
            out[k, 4] = ws.sum() / float(len(ws)) ** beta
        else:
            raise NotImplementedError("Unknown scoring method {}".format(scoring_method))
    return out, votes, sets


def vote_bound(n, magnitude):
    """fp32 accumulation of a convex combination of n terms of size <= magnitude, in any order, against float64."""
    return (2 * n + 4) * 2.0 ** -24 * magnitude


def postprocess(scores, boxes, score_thr, nms_thr, max_det, soft=None, vote=None, min_score=0.0001):
    """lib/core/test.py:369-408.  soft = (method name, sigma) or None (greedy NMS); vote = (thresh, scoring method, beta) or
    None.  Returns (idx int64 [T], cls int32 [T], dets [T, 5] - fp32 rows, or float64 rows rounded to fp32 after voting -,
    count int32 [C], votes int64 [T] (zeros without voting), rows64 [T, 5] the rows before that rounding), records in class
    order, within a class the reference's."""
    scores = np.asarray(scores, dtype=F32)
    boxes = np.asarray(boxes, dtype=F32)
    C = scores.shape[1]
    per_idx, per_det, per_votes, per_64 = [], [], [], []
    for j in range(C):
        inds = np.where(scores[:, j] > F32(score_thr))[0]
        dets_j = np.hstack((boxes[inds, :], scores[inds, j][:, None])).astype(F32)
        if soft is not None:
            if len(inds):
                nms_dets, keep = soft_nms(dets_j, soft[1], nms_thr, min_score, METHODS[soft[0]])
            else:
                nms_dets, keep = dets_j, np.zeros(0, np.int64)
        else:
            keep = np.asarray(nms(dets_j, nms_thr), dtype=np.int64)
            nms_dets = dets_j[keep, :]
        v, out = np.zeros(len(keep), np.int64), nms_dets.astype(np.float64)
        if vote is not None and len(keep):
            out, v, _ = box_voting(nms_dets, dets_j, vote[0], vote[1], vote[2])
            nms_dets = out.astype(F32)
        per_64.append(out)
        per_idx.append(inds[np.asarray(keep, dtype=np.int64)])
        per_det.append(nms_dets)
        per_votes.append(v)
    if max_det > 0:
        image_scores = np.hstack([d[:, -1] for d in per_det])
        if len(image_scores) > max_det:
            image_thresh = np.sort(image_scores)[-max_det]
            for j in range(C):
                on = per_det[j][:, -1] >= image_thresh
                per_idx[j], per_det[j], per_votes[j], per_64[j] = per_idx[j][on], per_det[j][on], per_votes[j][on], per_64[j][on]
    count = np.array([len(p) for p in per_idx], dtype=np.int32)
    return (np.concatenate(per_idx).astype(np.int64), np.repeat(np.arange(C, dtype=np.int32), count),
            np.vstack(per_det).astype(F32), count, np.concatenate(per_votes), np.vstack(per_64))
