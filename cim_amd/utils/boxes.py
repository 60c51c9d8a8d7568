"""lib/utils/boxes.py of the reference, the part on the inference path: `nms`, `soft_nms` and `box_voting`, on the device
(cim_amd.detect)."""
import numpy as np
import torch

from .. import detect


def nms(dets, thresh):
    """lib/utils/boxes.py:320-324 (+ cython_nms.pyx:36-87): dets [K, 5] = (x1, y1, x2, y2, score); greedy NMS keeping a
    box unless a higher-ranked kept box overlaps it by >= thresh.  Returns the kept row indices in ASCENDING order ([] for
    no rows).  Equal scores rank the higher row first.  Scores must not be NaN or -inf (every row is a candidate)."""
    if dets.shape[0] == 0:
        return []
    if torch.is_tensor(dets):
        d = dets.to(torch.float32)
        bad = bool((torch.isnan(d[:, 4]) | (d[:, 4] == float("-inf"))).any())
    else:
        d = np.asarray(dets, dtype=np.float32)
        bad = bool((np.isnan(d[:, 4]) | (d[:, 4] == -np.inf)).any())
    if bad:
        raise ValueError("cim_amd.utils.boxes.nms: NaN or -inf scores are not supported")
    s, b, _ = detect.device_inputs(d[:, 4:5].contiguous() if torch.is_tensor(d) else np.ascontiguousarray(d[:, 4:5]),
                                   d[:, :4])
    idx, _, _, _ = detect.to_host(detect.nms_limit(s, b, float("-inf"), thresh, 0))
    return idx


def _host_dets(dets, what):
    d = dets.detach().cpu().numpy() if torch.is_tensor(dets) else np.asarray(dets)
    d = np.ascontiguousarray(d, dtype=np.float32)
    if d.ndim != 2 or d.shape[1] != 5:
        raise ValueError("cim_amd.utils.boxes.%s: dets must be [K, 5], got %s" % (what, d.shape))
    return d


def soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=0.001, method='linear'):
    """lib/utils/boxes.py:327-344 (+ cython_nms.pyx:98-203): dets [K, 5] = (x1, y1, x2, y2, score) -> (dets [M, 5] f32 in
    selection order with the decayed scores, keep [M] the rows they came from), bit for bit the reference's.  Empty input
    comes back as (dets, []).  Scores must not be NaN or -inf (every row is a candidate); K <= cim_amd.detect.MAX_N."""
    if dets.shape[0] == 0:
        return dets, []
    assert method in detect.SOFT_NMS_METHODS, 'Unknown soft_nms method: {}'.format(method)
    if torch.is_tensor(dets) and not dets.is_cuda:
        raise detect._lib.CimHipError("cim_amd.utils.boxes.soft_nms: dets must be a CUDA/HIP tensor or a NumPy array")
    d = _host_dets(dets, "soft_nms")
    if bool((np.isnan(d[:, 4]) | (d[:, 4] == -np.inf)).any()):
        raise ValueError("cim_amd.utils.boxes.soft_nms: NaN or -inf scores are not supported")
    s, b, _ = detect.device_inputs(np.ascontiguousarray(d[:, 4:5]), np.ascontiguousarray(d[:, :4]))
    det = detect.postprocess(s, b, float("-inf"), overlap_thresh, 0,
                             soft_nms=dict(method=method, sigma=sigma, min_score=score_thresh))
    idx, _, sc, _, bx = detect.softvote_to_host(det)
    return np.hstack((bx, sc[:, None])).astype(np.float32, copy=False), idx


def box_voting(top_dets, all_dets, thresh, scoring_method='ID', beta=1.0):
    """lib/utils/boxes.py:268-317: top_dets [T, 5] refined by the score-weighted mean of the all_dets [K, 5] rows that
    overlap them by >= thresh; the score by scoring_method.  Returns top_dets_out [T, 5] f32.  An empty vote set raises
    ZeroDivisionError, as np.average does."""
    if scoring_method not in detect.SCORING_METHODS:
        raise NotImplementedError('Unknown scoring method {}'.format(scoring_method))
    for t in (top_dets, all_dets):
        if torch.is_tensor(t) and not t.is_cuda:
            raise detect._lib.CimHipError("cim_amd.utils.boxes.box_voting: dets must be CUDA/HIP tensors or NumPy arrays")
    top, alld = _host_dets(top_dets, "box_voting"), _host_dets(all_dets, "box_voting")
    out = top.copy()
    if top.shape[0] == 0:
        return out
    if alld.shape[0] == 0:
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    dev = detect._device()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                    # noqa: E731
    bx, sc, empty = detect.box_voting(up(top[:, :4]), up(alld[:, :4]), up(alld[:, 4]), thresh, scoring_method, beta)
    h = torch.cat([bx.reshape(-1), sc, empty.view(torch.float32)]).cpu().numpy()
    T = top.shape[0]
    if int(h[-1:].view(np.int32)[0]):
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    out[:, :4] = h[:4 * T].reshape(T, 4)
    if scoring_method != 'ID':
        out[:, 4] = h[4 * T:5 * T]
    return out
