"""lib/utils/boxes.py of the reference, the part on the inference path: `nms`, on the device (cim_amd.detect)."""
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
