"""Detection post-processing on the device: per-class score threshold, greedy box NMS and the per-image detection limit,
and the per-class argmax of CorLoc (csrc/detect.hip).

Replaces the host loops of lib/core/test.py:320-420 and lib/utils/mask_eval_utils.py:6-108 over the
compiled lib/utils/cython_nms.pyx.  Takes and returns DEVICE tensors and launches on the current stream; a CPU tensor is an
error (no CPU fallback).  `to_host` / `corloc_host` make the one device-to-host copy a caller of host results needs.
The reference-shaped wrappers are cim_amd.core.test, cim_amd.utils.mask_eval_utils and cim_amd.utils.boxes.
"""
import collections

import numpy as np
import torch

from . import _lib

MAX_N = 8192                    # CIM_DETECT_MAX_N of include/cim_hip.h

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
