"""Soft-NMS and box voting (cim_amd.detect.postprocess, csrc/detect.hip): the C ABI, the wrappers'
refusals and empty-input answers, and the NumPy restatement (tests/golden/softvote_np.py) against every golden captured
from the reference (make_golden_softvote.py).  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import softvote_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW = {"cim_softvote_ws_bytes", "cim_softvote_postprocess", "cim_softvote_vote"}
SUM_ONLY = ("AVG", "IOU_AVG", "QUASI_SUM")                              # scores that are sums and one division
TRANSCENDENTAL = ("GENERALIZED_AVG", "TEMP_AVG")


def parse_variant(v):
    """'greedy' | 'soft-<method>[@sigma]' [+ '+vote-<thresh>-<scoring>'] -> (soft (method, sigma) | None, vote (thresh,
    scoring, beta) | None)"""
    nms_part, _, vote_part = v.partition("+vote-")
    soft = None
    if nms_part != "greedy":
        name, _, sg = nms_part[len("soft-"):].partition("@")
        soft = (name, float(sg) if sg else 0.5)
    vote = None
    if vote_part:
        th, _, m = vote_part.partition("-")
        vote = (float(th), m, 1.0)
    return soft, vote


def _load():
    out = {}
    d = np.load(os.path.join(GOLDEN, "softvote_cases.npz"))
    for name in sorted({k.split("/", 1)[0] for k in d.files}):
        out[name] = {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(name + "/")}
    d = np.load(os.path.join(GOLDEN, "softvote_n1000_c20.npz"))
    out["n1000_c20"] = {k: d[k] for k in d.files}
    return out


GOLDENS = _load()
ZERO_WIDTH = GOLDENS.pop("zero_width")
VARIANTS = [(name, str(v)) for name in sorted(GOLDENS) for v in GOLDENS[name]["variants"]]
DIRECT = dict(np.load(os.path.join(GOLDEN, "softvote_direct.npz")))
DIRECT_CALLS = [(m, float(b), float(t)) for m, b, t in (str(c).split() for c in DIRECT["vote/calls"])]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_RESTATED = {}


def restated(name, variant):
    """softvote_np.postprocess of one golden variant, computed once and shared (never modified)."""
    if (name, variant) not in _RESTATED:
        g = GOLDENS[name]
        thr, nms, D = g["params"]
        soft, vote = parse_variant(variant)
        _RESTATED[(name, variant)] = softvote_np.postprocess(g["scores"], g["boxes"], thr, nms, int(D), soft=soft, vote=vote)
    return _RESTATED[(name, variant)]


def check_voted(got, want64, votes, all_boxes_max, scoring, yardstick=None, beta=1.0):
    """Voted rows `got` [T, 5] against the float64 evaluation `want64`: coordinates and the sum-only scores inside
    (2 n + 4) 2^-24 max|term| for a vote set of n (max|coordinate| of the voters for the boxes, 1 >= every score for the
    scores - QUASI_SUM is the mean times n^(1 - beta), so its bound scales by that -); the log / exp / pow scores inside
    `yardstick`."""
    got = np.asarray(got, np.float64)
    for k in range(len(got)):
        n = int(votes[k])
        assert np.all(np.abs(got[k, :4] - want64[k, :4]) <= softvote_np.vote_bound(n, all_boxes_max)), (k, got[k], want64[k])
        if scoring == "ID":
            assert got[k, 4] == want64[k, 4]
        elif scoring in SUM_ONLY:
            scale = float(n) ** (1.0 - beta) if scoring == "QUASI_SUM" else 1.0
            assert abs(got[k, 4] - want64[k, 4]) <= softvote_np.vote_bound(n, scale), (k, got[k, 4], want64[k, 4])
        elif yardstick is not None:
            assert abs(got[k, 4] - want64[k, 4]) <= yardstick, (k, got[k, 4], want64[k, 4], yardstick)


def reference_yardstick():
    """The largest deviation of the reference's own fp32 goldens from the float64 evaluation over the log / exp / pow
    scoring methods (goldens without an active limit, so rows pair up one to one)."""
    worst = 0.0
    for name, variant in VARIANTS:
        soft, vote = parse_variant(variant)
        if vote is None or vote[1] not in TRANSCENDENTAL:
            continue
        want = restated(name, variant)[5]
        worst = max(worst, float(np.abs(GOLDENS[name][variant + "/cls_boxes"][:, 4].astype(np.float64) - want[:, 4]).max()))
    for m, beta, th in DIRECT_CALLS:
        if m in TRANSCENDENTAL:
            want, _, _ = softvote_np.box_voting(DIRECT["vote/top"], DIRECT["vote/all"], th, m, beta)
            worst = max(worst, float(np.abs(DIRECT["vote/%s/out" % m][:, 4].astype(np.float64) - want[:, 4]).max()))
    assert worst > 0
    return worst


def test_header_declares_and_lib_binds_softvote_entries():
    from cim_amd import _lib, build
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_softvote_[a-z0-9_]+)\s*\(", header))
    assert declared == NEW
    assert declared <= set(_lib.SIGNATURES)
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert [_lib.CONSTANTS["CIM_SOFTVOTE_SCORE_" + m] for m in softvote_np.SCORING] == list(range(6))
    assert [_lib.CONSTANTS["CIM_SOFTVOTE_NMS_SOFT_" + m.upper()] for m in ("hard", "linear", "gaussian")] == [1, 2, 3]


def test_workspace_size_refuses_out_of_range_shapes():
    from cim_amd import _lib, build
    build.build()
    assert _lib.call("cim_softvote_ws_bytes", 1, 1) > 0
    assert _lib.call("cim_softvote_ws_bytes", 8192, 80) > _lib.call("cim_detect_ws_bytes", 8192, 80)
    for n, c in ((0, 20), (8193, 20), (100, 0)):
        assert _lib.call("cim_softvote_ws_bytes", n, c) == -1
        assert b"N <= 8192" in _lib.load().cim_last_error()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from cim_amd import _lib, build
    build.build()

    def post(n, c, kind=2, scoring=0, vote=0, score_thr=1e-5):
        return _lib.call("cim_softvote_postprocess", None, c, None, n, c, score_thr, 0.3, kind, 0.5, 1e-4, vote, 0.8, scoring, 1.0,
                         100, None, None, None, None, None, None, None)

    for args in ((0, 3), (8193, 3), (10, 0)):
        with pytest.raises(_lib.CimHipError, match="N <= 8192"):
            post(*args)
    with pytest.raises(_lib.CimHipError, match="unknown nms_kind"):
        post(10, 3, kind=4)
    with pytest.raises(_lib.CimHipError, match="unknown nms_kind"):
        post(10, 3, scoring=6)
    with pytest.raises(_lib.CimHipError, match="score_thr >= 0"):
        post(10, 3, vote=1, score_thr=-1.0)
    with pytest.raises(_lib.CimHipError, match="K >= 1"):
        _lib.call("cim_softvote_vote", None, None, 0, None, 1, 0.5, 0, 1.0, None, None, None, None)


def test_wrappers_reject_cpu_tensors_and_answer_empty_inputs():
    from cim_amd import _lib, detect
    from cim_amd.core import test as core_test
    from cim_amd.core.config import cfg
    from cim_amd.utils import boxes as box_utils
    s, b = torch.rand(10, 3), torch.rand(10, 4)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        detect.postprocess(s, b, soft_nms=dict(method="linear"))
    with pytest.raises(_lib.CimHipError, match="CUDA/HIP"):
        detect.box_voting(b, b, s[:, 0], 0.5)
    with pytest.raises(_lib.CimHipError):
        box_utils.soft_nms(torch.rand(5, 5))
    with pytest.raises(_lib.CimHipError):
        box_utils.box_voting(torch.rand(5, 5), torch.rand(5, 5), 0.5)
    with pytest.raises(ValueError, match="score_thr >= 0"):
        detect.postprocess(s, b, score_thr=-1.0, box_vote=dict(thresh=0.8))
    with pytest.raises(AssertionError, match="Unknown soft_nms method"):
        box_utils.soft_nms(np.zeros((3, 5), np.float32), method="cubic")
    with pytest.raises(NotImplementedError, match="Unknown scoring method"):
        box_utils.box_voting(np.zeros((3, 5), np.float32), np.zeros((3, 5), np.float32), 0.5, scoring_method="MAX")
    empty = np.zeros((0, 5), np.float32)
    d, keep = box_utils.soft_nms(empty)
    assert d is empty and keep == []
    out = box_utils.box_voting(empty, np.ones((4, 5), np.float32), 0.5)
    assert out.shape == (0, 5) and out is not empty
    saved, saved_classes = cfg.TEST, cfg.MODEL.NUM_CLASSES
    try:
        for key in ("SOFT_NMS", "BBOX_VOTE"):                          # no longer refused: the call reaches the device path
            cfg.TEST = dict(saved, **{key: {"ENABLED": True}})
            cfg.MODEL.NUM_CLASSES = 3
            with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
                core_test.box_results_with_nms_and_limit(s, b)
    finally:
        cfg.TEST = saved
        cfg.MODEL.NUM_CLASSES = saved_classes


def test_config_keys_and_defaults():
    from cim_amd.core import test as core_test
    from cim_amd.core.config import AttrDict
    c = AttrDict(TEST=AttrDict())
    assert core_test._soft_vote_cfg(c) == (None, None)
    c.TEST.SOFT_NMS = AttrDict(ENABLED=True)
    c.TEST.BBOX_VOTE = AttrDict(ENABLED=True)
    assert core_test._soft_vote_cfg(c) == (dict(method="linear", sigma=0.5, min_score=0.0001),
                                           dict(thresh=0.8, scoring_method="ID", beta=1.0))
    c.TEST.SOFT_NMS = AttrDict(ENABLED=True, METHOD="gaussian", SIGMA=0.3)
    c.TEST.BBOX_VOTE = AttrDict(ENABLED=False, VOTE_TH=0.5, SCORING_METHOD="AVG")
    assert core_test._soft_vote_cfg(c) == (dict(method="gaussian", sigma=0.3, min_score=0.0001), None)


def test_goldens_cover_what_they_must():
    assert {"k1", "n63", "n64", "n65", "n255", "n257", "n1000_c20", "ties", "identical", "disjoint_low", "clustered",
            "degenerate", "limit_exact", "limit_plus1", "limit_tie", "vote", "vote_limit", "empty"} <= set(GOLDENS)
    g = GOLDENS["identical"]
    assert list(g["soft-hard/counts"]) == [1, 1]                       # all boxes identical: one survives per class
    lin = g["soft-linear/cls_boxes"]
    assert list(g["soft-linear/counts"]) == [1, 1] and len(lin) == 2   # linear: weight 1 - 1 = 0
    g = GOLDENS["disjoint_low"]
    thr = np.float32(g["params"][0])
    for v in ("soft-hard", "soft-linear", "soft-gaussian"):            # below the soft-NMS minimum, yet never removed
        assert np.array_equal(g[v + "/counts"], (g["scores"] > thr).sum(0))
        assert g[v + "/cls_boxes"][:, 4].max() < 1e-4
    g = GOLDENS["ties"]
    assert all(len(np.unique(g["scores"][:, j])) < 10 for j in range(g["scores"].shape[1]))
    assert int(GOLDENS["limit_exact"]["soft-linear/counts"].sum()) == 120
    assert int(GOLDENS["limit_plus1"]["soft-linear/counts"].sum()) == 119
    assert int(GOLDENS["limit_tie"]["soft-gaussian/counts"].sum()) == 61
    g = GOLDENS["vote_limit"]                                          # vote -> limit: re-scoring changes who stays
    assert not np.array_equal(g["greedy+vote-0.5-AVG/cls_boxes"][:, :4], g["greedy+vote-0.5-ID/cls_boxes"][:, :4])
    scorings = {parse_variant(v)[1][1] for _, v in VARIANTS if parse_variant(v)[1]}
    assert scorings == set(softvote_np.SCORING)
    assert {parse_variant(v)[1][0] for _, v in VARIANTS if parse_variant(v)[1]} == {0.5, 0.8}


@pytest.mark.parametrize("name,variant", [nv for nv in VARIANTS if parse_variant(nv[1])[1] is None])
def test_soft_nms_restatement_is_bit_identical_to_the_goldens(name, variant):
    g = GOLDENS[name]
    idx, cls, dets, count, _, _ = restated(name, variant)
    assert np.array_equal(count, g[variant + "/counts"])
    assert np.array_equal(_bits(dets), _bits(g[variant + "/cls_boxes"]))       # selection order, decayed score bits
    assert np.array_equal(_bits(g["boxes"][idx]), _bits(dets[:, :4]))          # ... and the proposals they came from
    last = cls < g["scores"].shape[1] - 1                                      # the flat arrays omit the last class
    assert np.array_equal(_bits(dets[last, 4]), _bits(g[variant + "/out_scores"]))
    assert np.array_equal(_bits(dets[last, :4]), _bits(g[variant + "/out_boxes"]))


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_soft_nms_restatement_direct_call(method):
    want_d, want_k = DIRECT["soft/%s/dets" % method], DIRECT["soft/%s/keep" % method]
    for form in (softvote_np.soft_nms, softvote_np.soft_nms_loop):
        d, k = form(DIRECT["soft/dets_in"], 0.5, 0.3, 0.001, softvote_np.METHODS[method])
        assert np.array_equal(k, want_k) and np.array_equal(_bits(d), _bits(want_d))


@pytest.mark.parametrize("name,variant", [nv for nv in VARIANTS if parse_variant(nv[1])[1] is not None])
def test_voting_restatement_against_the_goldens(name, variant):
    """The reference's fp32 rows lie inside the derived bound around the float64 evaluation, on identical vote sets (the
    record counts, and through them the sets' effect on the limit, are identical)."""
    g = GOLDENS[name]
    soft, vote = parse_variant(variant)
    idx, cls, dets, count, votes, rows64 = restated(name, variant)
    assert np.array_equal(count, g[variant + "/counts"])
    want = g[variant + "/cls_boxes"]
    assert len(want) == len(rows64)
    mx = float(np.abs(g["boxes"]).max())
    yard = reference_yardstick() if vote[1] in TRANSCENDENTAL else None
    check_voted(want, rows64, votes, mx, vote[1], yard)


def test_voting_restatement_direct_calls():
    mx = float(np.abs(DIRECT["vote/all"][:, :4]).max())
    for m, beta, th in DIRECT_CALLS:
        want, votes, _ = softvote_np.box_voting(DIRECT["vote/top"], DIRECT["vote/all"], th, m, beta)
        assert votes.min() >= 1
        check_voted(DIRECT["vote/%s/out" % m], want, votes, mx, m, reference_yardstick(), beta)


def test_partition_form_equals_the_literal_loop():
    rng = np.random.RandomState(5)
    for it in range(2000):
        k = rng.randint(1, 41)
        centres = rng.uniform(0, 60, (rng.randint(1, 4), 2))
        at = centres[rng.randint(0, len(centres), k)] + np.round(rng.uniform(-4, 4, (k, 2)))
        wh = np.round(rng.uniform(8, 30, (k, 2)))
        score = (rng.randint(1, rng.randint(3, 8), k) / 8.0) * rng.choice([1.0, 0.01, 0.0005])
        dets = np.hstack((at, at + wh, score[:, None])).astype(np.float32)
        method, thresh = it % 3, float(rng.choice([0.001, 0.0001, 0.05]))
        d0, k0 = softvote_np.soft_nms_loop(dets, 0.5, 0.3, thresh, method)
        d1, k1 = softvote_np.soft_nms(dets, 0.5, 0.3, thresh, method)
        assert np.array_equal(k0, k1) and np.array_equal(_bits(d0), _bits(d1)), (it, method)
