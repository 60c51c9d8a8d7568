"""-m gpu: detection post-processing on the device (csrc/detect.hip) - bit for bit against the reference's goldens through
the reference-shaped wrappers, and against the NumPy restatement (tests/golden/detect_np.py) where no golden exists."""
import os
import threading

import numpy as np
import pytest
import torch

import detect_np
from test_detect_cpu import GOLDEN_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set_cfg(cfg, C, thr, nms, D):
    cfg.MODEL.NUM_CLASSES = C
    cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = float(thr), float(nms), int(D)


def _check_structure(cls_boxes, C):
    assert len(cls_boxes) == C + 1 and cls_boxes[0] == []
    for a in cls_boxes[1:]:
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
@pytest.mark.parametrize("on_device", [False, True])
def test_goldens_through_reference_interfaces(name, on_device):
    from cim_amd.core import test as core_test
    from cim_amd.core.config import cfg
    from cim_amd.utils import boxes as box_utils
    from cim_amd.utils import mask_eval_utils
    g = GOLDEN_CASES[name]
    scores, boxes = g["scores"], g["boxes"]
    thr, nms, D = g["params"]
    C = scores.shape[1]
    _set_cfg(cfg, C, thr, nms, D)
    s_in, b_in = (torch.from_numpy(scores).to(DEV), torch.from_numpy(boxes).to(DEV)) if on_device else (scores, boxes)

    s, b, cb = core_test.box_results_with_nms_and_limit(s_in, b_in)
    _check_structure(cb, C)
    assert np.array_equal([len(a) for a in cb[1:]], g["nms_counts"])
    assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(g["nms_cls_boxes"]))
    assert np.array_equal(_bits(s), _bits(g["nms_scores"])) and np.array_equal(_bits(b), _bits(g["nms_boxes"]))
    assert len(s) == int(g["nms_counts"][:-1].sum())                   # the last class is not in the flat arrays

    s, b, cb = core_test.box_results_for_corloc(s_in, b_in)
    _check_structure(cb, C)
    assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(g["corloc_cls_boxes"]))
    assert np.array_equal(_bits(s), _bits(g["corloc_scores"])) and np.array_equal(_bits(b), _bits(g["corloc_boxes"]))

    _set_cfg(cfg, C, thr, nms, 12345)                                  # _get_index takes its limit from the argument
    s, b, cb, ci = mask_eval_utils.mask_results_with_nms_and_limit_get_index(cfg, s_in, b_in, DETECTIONS_PER_IM=int(D))
    _check_structure(cb, C)
    assert len(ci) == C + 1 and ci[0] == [] and all(a.dtype == np.int64 for a in ci[1:])
    assert np.array_equal(np.concatenate(ci[1:]), g["index_inds"])
    assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(g["index_cls_boxes"]))
    assert np.array_equal(_bits(s), _bits(g["index_scores"])) and np.array_equal(_bits(b), _bits(g["index_boxes"]))

    _set_cfg(cfg, C, thr, nms, D)
    masks = np.arange(len(boxes) * 6, dtype=np.float32).reshape(len(boxes), 2, 3)
    m_in = torch.from_numpy(masks).to(DEV) if on_device else masks
    s, b, cb, cm = mask_eval_utils.mask_results_with_nms_and_limit(cfg, s_in, b_in, m_in)
    assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(g["nms_cls_boxes"]))
    got = np.concatenate([a.cpu().numpy() if on_device else a for a in cm[1:]])
    assert np.array_equal(got, masks[g["index_inds"]])

    # utils.boxes.nms on one class's candidates of the golden
    j = int(np.argmax(g["nms_counts"]))
    inds = np.where(scores[:, j] > np.float32(thr))[0]
    dets = np.hstack((boxes[inds], scores[inds, j][:, None])).astype(np.float32)
    keep = box_utils.nms(torch.from_numpy(dets).to(DEV) if on_device else dets, nms)
    assert np.array_equal(keep, detect_np.nms(dets, nms))
    assert list(keep) == sorted(keep)


def _sweep_inputs(n, c, seed, kind):
    rng = np.random.RandomState(seed)
    size = 40.0 * np.sqrt(n)                                           # ~constant box density
    x1, y1 = rng.uniform(0, size, n), rng.uniform(0, size, n)
    w, h = rng.uniform(2, 80, n), rng.uniform(2, 80, n)
    boxes = np.stack([x1, y1, x1 + w, y1 + h], 1)
    boxes[: n // 2] = np.floor(boxes[: n // 2])
    boxes = boxes.astype(np.float32)
    scores = rng.rand(n, c).astype(np.float32)
    scores[rng.rand(n, c) < (0.5 if c <= 20 else 0.875)] = 0          # most proposals below the threshold, as for real classes
    if kind == "ties":                                                 # duplicate boxes with bit-identical scores
        dup = rng.choice(n, n // 3)
        src = rng.choice(n, n // 3)
        boxes[dup], scores[dup] = boxes[src], scores[src]
        scores = np.round(scores * 8) / 8                              # and many equal scores across boxes
    elif kind == "one_box":                                            # one box contains every other, highest score
        boxes[0] = [0, 0, size + 100, size + 100]
        boxes[1:] = boxes[0]
        scores[0] = 2.0
    elif kind == "none":
        scores[:] = np.float32(1e-5)
    return scores.astype(np.float32), boxes


def _device_vs_restatement(scores, boxes, thr, nms, D, stream=None):
    from cim_amd import detect
    s, b = torch.from_numpy(scores).to(DEV), torch.from_numpy(boxes).to(DEV)
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        got = detect.to_host(detect.nms_limit(s, b, thr, nms, D))
    return got


def _assert_same(got, ref):
    idx, cls, sc, count = got
    ridx, rcls, rsc, rcount = ref
    assert np.array_equal(count, rcount)
    assert np.array_equal(idx, ridx) and np.array_equal(cls, rcls)
    assert np.array_equal(_bits(sc), _bits(rsc))


SWEEP = [(n, c) for n in (1, 63, 64, 65, 1000, 2000, 4097, 8192) for c in (1, 20, 80)]


@pytest.mark.parametrize("n,c", SWEEP)
def test_sweep_matches_restatement(n, c):
    from cim_amd import detect
    scores, boxes = _sweep_inputs(n, c, n * 131 + c, "plain")
    for thr, nms, D in ((1e-5, 0.3, 100), (0.2, 0.5, 0)):
        ref = detect_np.nms_limit(scores, boxes, thr, nms, D)
        _assert_same(_device_vs_restatement(scores, boxes, thr, nms, D), ref)
    idx, sc = detect.corloc_host(torch.from_numpy(scores).to(DEV))
    assert np.array_equal(idx, detect_np.corloc(scores)) and np.array_equal(_bits(sc), _bits(scores[idx, np.arange(c)]))


@pytest.mark.parametrize("kind", ["ties", "one_box", "none"])
@pytest.mark.parametrize("n,c", [(65, 3), (2000, 20)])
@pytest.mark.parametrize("D", [100, 0, -1])
def test_special_inputs_match_restatement(kind, n, c, D):
    scores, boxes = _sweep_inputs(n, c, 7 + n + c, kind)
    ref = detect_np.nms_limit(scores, boxes, 1e-5, 0.3, D)
    _assert_same(_device_vs_restatement(scores, boxes, 1e-5, 0.3, D), ref)
    if kind == "one_box":
        assert np.all(ref[3] == (scores > np.float32(1e-5)).any(0))   # one box (proposal 0) per class survives
    if kind == "none":
        assert ref[3].sum() == 0


def test_corloc_nan_and_ties():
    from cim_amd import detect
    s = np.array([[0.5, 0.1, np.nan], [0.7, 0.1, 0.2], [0.7, np.nan, np.nan], [-0.0, 0.1, 0.9]], np.float32)
    idx, _ = detect.corloc_host(torch.from_numpy(s).to(DEV))
    assert list(idx) == list(detect_np.corloc(s)) == [1, 2, 0]


def test_im_detect_all_scores_match_restatement():
    """The stage on the device scores im_detect_all returns (cfg1 model, test-time augmentation on)."""
    from cases import TTA, procedural_init, tta_inputs
    from cim_amd.core import test as core_test
    from cim_amd.core.config import cfg
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling.model_builder import Generalized_RCNN
    apply_preset(TTA["config"])
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = TTA["SCALE"], TTA["MAX_SIZE"]
    cfg.TEST.BBOX_AUG.SCALES, cfg.TEST.BBOX_AUG.MAX_SIZE = TTA["SCALES"], TTA["MAX_SIZE"]
    m = Generalized_RCNN()
    procedural_init(m)
    m = m.to(DEV).eval()
    im, boxes, masks = tta_inputs()
    with torch.no_grad():
        res = core_test.im_detect_all(m, im, boxes, masks)
    assert res["scores"].is_cuda
    scores = res["scores"].cpu().numpy()
    C = cfg.MODEL.NUM_CLASSES
    for D in (100, 5):
        cfg.TEST.DETECTIONS_PER_IM = D
        s, b, cb = core_test.box_results_with_nms_and_limit(res["scores"], res["boxes"])
        idx, cls, sc, count = detect_np.nms_limit(scores[:, :C], boxes, core_test._post_cfg(cfg, "SCORE_THRESH"),
                                                 core_test._post_cfg(cfg, "NMS"), D)
        assert np.array_equal([len(a) for a in cb[1:]], count)
        assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(np.hstack((boxes[idx], sc[:, None]))))
    s, b, cb = core_test.box_results_for_corloc(res["scores"], res["boxes"])
    assert np.array_equal(_bits(np.vstack(cb[1:])[:, 4]), _bits(scores[detect_np.corloc(scores[:, :C]), np.arange(C)]))


def test_two_streams_match_one():
    from cim_amd import detect
    inputs = [_sweep_inputs(2000, 20, 11, "plain"), _sweep_inputs(1000, 80, 12, "ties")]
    one = [_device_vs_restatement(s, b, 1e-5, 0.3, 100) for s, b in inputs]
    dev = [(torch.from_numpy(s).to(DEV), torch.from_numpy(b).to(DEV)) for s, b in inputs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    results = [None, None]

    def run(k):
        with torch.cuda.stream(streams[k]):
            dets = [detect.nms_limit(*dev[k], 1e-5, 0.3, 100) for _ in range(8)]
            results[k] = [detect.to_host(d) for d in dets]

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k in range(2):
        for got in results[k]:
            _assert_same(got, one[k])


def test_n_above_limit_raises_before_launch():
    from cim_amd import detect
    s, b = torch.rand(8193, 3, device=DEV), torch.rand(8193, 4, device=DEV)
    with pytest.raises(ValueError, match="8192"):
        detect.nms_limit(s, b)
    with pytest.raises(ValueError, match="8192"):
        detect.corloc(s)
    torch.cuda.synchronize()
