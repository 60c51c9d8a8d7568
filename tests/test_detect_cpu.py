"""Detection post-processing (cim_amd.detect, csrc/detect.hip): the C ABI, the Python API's refusals, and the NumPy
restatement (tests/golden/detect_np.py) against every golden captured from the reference (make_golden_detect.py).
No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import detect_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FILES = ("detect_n1000_c20", "detect_n2000_c80", "detect_eval_vgg16_voc")
CASES = ("limit_exact", "limit_plus1", "limit_tie", "empty", "degenerate", "nolimit")


def golden_cases():
    for f in FILES:
        d = np.load(os.path.join(GOLDEN, f + ".npz"))
        yield f, {k: d[k] for k in d.files}
    d = np.load(os.path.join(GOLDEN, "detect_cases.npz"))
    for c in CASES:
        yield c, {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(c + "/")}


GOLDEN_CASES = dict(golden_cases())


def test_header_declares_and_lib_binds_detect_entries():
    from cim_amd import _lib, build
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_detect_[a-z0-9_]+)\s*\(", header))
    assert declared == {"cim_detect_ws_bytes", "cim_detect_nms_limit", "cim_detect_corloc"}
    assert declared <= set(_lib.SIGNATURES)
    assert "#define CIM_DETECT_MAX_N 8192" in header
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]


def test_workspace_size_refuses_out_of_range_shapes():
    from cim_amd import _lib, build, detect
    build.build()
    assert _lib.call("cim_detect_ws_bytes", 1, 1) > 0
    assert _lib.call("cim_detect_ws_bytes", 8192, 80) >= 8192 * 128 * 8
    for n, c in ((0, 20), (8193, 20), (100, 0), (8192, 1 << 20)):
        assert _lib.call("cim_detect_ws_bytes", n, c) == -1
        assert b"N <= 8192" in _lib.load().cim_last_error()
    assert detect.MAX_N == 8192


def test_detect_rejects_cpu_tensors():
    from cim_amd import _lib, detect
    from cim_amd.core import test as core_test
    from cim_amd.utils import boxes as box_utils
    s, b = torch.rand(10, 3), torch.rand(10, 4)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        detect.nms_limit(s, b)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        detect.corloc(s)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        core_test.box_results_with_nms_and_limit(s, b)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        box_utils.nms(torch.rand(5, 5), 0.3)
    assert box_utils.nms(np.zeros((0, 5), np.float32), 0.3) == []


def test_soft_nms_and_box_voting_are_refused():
    from cim_amd.core import test as core_test
    from cim_amd.core.config import cfg
    saved = cfg.TEST if "TEST" in cfg else None
    try:
        for key in ("SOFT_NMS", "BBOX_VOTE"):
            cfg.TEST = {key: {"ENABLED": True}}
            with pytest.raises(NotImplementedError, match=key):
                core_test._post_check(cfg)
    finally:
        if saved is None:
            del cfg["TEST"]
        else:
            cfg.TEST = saved


def _dets(boxes, idx, score):
    return np.hstack((boxes[idx], score[:, None])).astype(np.float32)


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_restatement_matches_reference_goldens(name):
    g = GOLDEN_CASES[name]
    scores, boxes = g["scores"], g["boxes"]
    thr, nms_thr, D = g["params"]
    C = scores.shape[1]
    idx, cls, sc, count = detect_np.nms_limit(scores, boxes, thr, nms_thr, int(D))
    assert np.array_equal(count, g["nms_counts"]) and np.array_equal(count, g["index_counts"])
    assert np.array_equal(_dets(boxes, idx, sc).view(np.uint32), g["nms_cls_boxes"].view(np.uint32))
    assert np.array_equal(idx, g["index_inds"])
    flat = _dets(boxes, idx, sc)[cls < C - 1]                      # the reference's flat arrays omit the last class
    assert np.array_equal(flat[:, -1].view(np.uint32), g["nms_scores"].view(np.uint32))
    assert np.array_equal(flat[:, :-1].view(np.uint32), g["nms_boxes"].view(np.uint32))
    am = detect_np.corloc(scores)
    assert np.array_equal(_dets(boxes, am, scores[am, np.arange(C)]).view(np.uint32),
                          g["corloc_cls_boxes"].view(np.uint32))


def test_restatement_tie_rule_and_nan_overlaps():
    """Equal scores: the higher proposal index is visited first; zero-area duplicates (0 / 0 overlaps) never suppress."""
    boxes = np.array([[0, 0, 10, 10]] * 3 + [[50, 50, 49, 60]] * 2, np.float32)
    dets = np.hstack((boxes, np.full((5, 1), 0.5, np.float32)))
    assert list(detect_np.nms(dets, 0.3)) == [2, 3, 4]
    dets[1, 4] = 0.6
    assert list(detect_np.nms(dets, 0.3)) == [1, 3, 4]
