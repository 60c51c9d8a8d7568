"""-m gpu: soft-NMS and box voting on the device (csrc/detect.hip) - soft-NMS bit for bit against the
reference's goldens through the reference-shaped wrappers, voting inside the derived bound around the float64 evaluation,
and both against the NumPy restatement (tests/golden/softvote_np.py) where no golden exists."""
import numpy as np
import pytest
import torch

import softvote_np
from test_detect_cpu import GOLDEN_CASES as DETECT_GOLDENS
from test_softvote_cpu import (DIRECT, DIRECT_CALLS, GOLDENS, SUM_ONLY, TRANSCENDENTAL, VARIANTS, ZERO_WIDTH, check_voted,
                               parse_variant, reference_yardstick, restated)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METHODS = ("hard", "linear", "gaussian")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Cfg:
    """cfg.TEST / NUM_CLASSES set for one call of the wrapper and put back."""

    def __init__(self, C, thr, nms, D, soft, vote):
        from cim_amd.core.config import cfg
        self.cfg, self.C = cfg, C
        self.test = dict(SCORE_THRESH=float(thr), NMS=float(nms), DETECTIONS_PER_IM=int(D))
        if soft is not None:
            self.test["SOFT_NMS"] = dict(ENABLED=True, METHOD=soft[0], SIGMA=soft[1])
        if vote is not None:
            self.test["BBOX_VOTE"] = dict(ENABLED=True, VOTE_TH=vote[0], SCORING_METHOD=vote[1])

    def __enter__(self):
        self.saved = (self.cfg.TEST, self.cfg.MODEL.NUM_CLASSES)
        self.cfg.TEST = type(self.saved[0])(self.saved[0], **self.test)
        self.cfg.MODEL.NUM_CLASSES = self.C

    def __exit__(self, *exc):
        self.cfg.TEST, self.cfg.MODEL.NUM_CLASSES = self.saved


def vote_counts(top, dets_j, thresh):
    """The vote set sizes, read back from the device: QUASI_SUM with unit weights and beta = 0 is sum(1) / n^0 = n."""
    from cim_amd import detect
    _, n, empty = detect.box_voting(_dev(top[:, :4]), _dev(dets_j[:, :4]), torch.ones(len(dets_j), device=DEV), thresh,
                                    "QUASI_SUM", beta=0.0)
    assert int(empty.cpu()[0]) == 0
    return n.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("name,variant", VARIANTS)
def test_goldens_through_box_results_with_nms_and_limit(name, variant, on_device):
    from cim_amd.core import test as core_test
    g = GOLDENS[name]
    scores, boxes = g["scores"], g["boxes"]
    thr, nms, D = g["params"]
    C = scores.shape[1]
    soft, vote = parse_variant(variant)
    s_in, b_in = (_dev(scores), _dev(boxes)) if on_device else (scores, boxes)
    with _Cfg(C, thr, nms, D, soft, vote):
        s, b, cb = core_test.box_results_with_nms_and_limit(s_in, b_in)
    assert len(cb) == C + 1 and cb[0] == []
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5 for a in cb[1:])
    assert np.array_equal([len(a) for a in cb[1:]], g[variant + "/counts"])
    got, want = np.vstack(cb[1:]), g[variant + "/cls_boxes"]
    last = int(g[variant + "/counts"][:-1].sum())                      # the flat arrays omit the last class
    assert np.array_equal(_bits(s), _bits(got[:last, 4])) and np.array_equal(_bits(b), _bits(got[:last, :4]))
    if vote is None:                                                   # selection order, decayed score bits
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(s), _bits(g[variant + "/out_scores"]))
        assert np.array_equal(_bits(b), _bits(g[variant + "/out_boxes"]))
        return
    idx, cls, dets, count, votes, rows64 = restated(name, variant)
    yard = 4 * reference_yardstick() if vote[1] in TRANSCENDENTAL else None
    check_voted(got, rows64, votes, float(np.abs(boxes).max()), vote[1], yard)
    if vote[1] == "ID":                                                # scores pass through: the NMS stage's bits
        assert np.array_equal(_bits(got[:, 4]), _bits(want[:, 4]))


@pytest.mark.parametrize("name,variant", [nv for nv in VARIANTS if parse_variant(nv[1])[1] is not None and nv[1].endswith("-ID")])
def test_vote_sets_are_identical(name, variant):
    g = GOLDENS[name]
    thr = np.float32(g["params"][0])
    soft, vote = parse_variant(variant)
    idx, cls, dets, count, votes, _ = restated(name, variant)
    for j in range(g["scores"].shape[1]):
        if not count[j]:
            continue
        inds = np.where(g["scores"][:, j] > thr)[0]
        dets_j = np.hstack((g["boxes"][inds], g["scores"][inds, j][:, None])).astype(np.float32)
        top = np.hstack((g["boxes"][idx[cls == j]], dets[cls == j, 4:5])).astype(np.float32)
        assert np.array_equal(vote_counts(top, dets_j, vote[0]), votes[cls == j])


@pytest.mark.parametrize("on_device", [False, True])
def test_goldens_through_utils_boxes(on_device):
    from cim_amd.utils import boxes as box_utils
    dets = DIRECT["soft/dets_in"]
    for m in METHODS:
        d, keep = box_utils.soft_nms(_dev(dets) if on_device else dets, method=m)
        assert np.array_equal(keep, DIRECT["soft/%s/keep" % m]) and keep.dtype == np.int64
        assert d.dtype == np.float32 and np.array_equal(_bits(d), _bits(DIRECT["soft/%s/dets" % m]))
    top, alld = DIRECT["vote/top"], DIRECT["vote/all"]
    mx = float(np.abs(alld[:, :4]).max())
    yard = 4 * reference_yardstick()
    for m, beta, th in DIRECT_CALLS:
        out = box_utils.box_voting(_dev(top) if on_device else top, _dev(alld) if on_device else alld, th, scoring_method=m,
                                   beta=beta)
        want, votes, _ = softvote_np.box_voting(top, alld, th, m, beta)
        assert out.dtype == np.float32 and out.shape == top.shape
        assert np.array_equal(vote_counts(top, alld, th), votes)
        check_voted(out, want, votes, mx, m, yard, beta)
        if m == "ID":
            assert np.array_equal(_bits(out[:, 4]), _bits(top[:, 4]))


_NMS_STAGE = {}


def nms_stage(name, variant):
    """The restatement of a golden variant's NMS stage alone - no voting, no limit -, computed once per (golden, NMS kind)."""
    g = GOLDENS[name]
    thr, nms, _ = g["params"]
    soft, _ = parse_variant(variant)
    if (name, soft) not in _NMS_STAGE:
        _NMS_STAGE[(name, soft)] = softvote_np.postprocess(g["scores"], g["boxes"], thr, nms, 0, soft=soft)
    return _NMS_STAGE[(name, soft)]


def class_dets(g, j):
    inds = np.where(g["scores"][:, j] > np.float32(g["params"][0]))[0]
    return inds, np.hstack((g["boxes"][inds], g["scores"][inds, j][:, None])).astype(np.float32)


@pytest.mark.parametrize("name,variant", [nv for nv in VARIANTS if nv[1].startswith("soft-") and "+vote" not in nv[1]])
def test_every_soft_nms_golden_through_utils_boxes(name, variant):
    """Class by class (the first four of the 20-class golden); without a limit the golden's rows are the classes' rows."""
    from cim_amd.utils import boxes as box_utils
    g = GOLDENS[name]
    (method, sigma), _ = parse_variant(variant)
    idx, cls, dets, count, _, _ = nms_stage(name, variant)
    for j in range(min(g["scores"].shape[1], 4)):
        inds, dets_j = class_dets(g, j)
        d, keep = box_utils.soft_nms(dets_j, sigma=sigma, overlap_thresh=g["params"][1], score_thresh=0.0001, method=method)
        if not len(dets_j):
            assert keep == [] and d is dets_j
            continue
        assert np.array_equal(inds[keep], idx[cls == j]) and np.array_equal(_bits(d), _bits(dets[cls == j]))
        if g["params"][2] == 0:
            lo = int(g[variant + "/counts"][:j].sum())
            assert np.array_equal(_bits(d), _bits(g[variant + "/cls_boxes"][lo:lo + len(d)]))


@pytest.mark.parametrize("name,variant", [nv for nv in VARIANTS if "+vote" in nv[1]])
def test_every_voting_golden_through_utils_boxes(name, variant):
    from cim_amd.utils import boxes as box_utils
    g = GOLDENS[name]
    _, vote = parse_variant(variant)
    idx, cls, dets, count, _, _ = nms_stage(name, variant)
    mx = float(np.abs(g["boxes"]).max())
    yard = 4 * reference_yardstick() if vote[1] in TRANSCENDENTAL else None
    for j in range(min(g["scores"].shape[1], 4)):
        _, dets_j = class_dets(g, j)
        top = dets[cls == j]
        out = box_utils.box_voting(top, dets_j, vote[0], scoring_method=vote[1])
        assert out.dtype == np.float32 and out.shape == top.shape
        if not len(top):
            continue
        want, votes, _ = softvote_np.box_voting(top, dets_j, vote[0], vote[1], 1.0)
        assert np.array_equal(vote_counts(top, dets_j, vote[0]), votes)
        check_voted(out, want, votes, mx, vote[1], yard)
        if g["params"][2] == 0:                                        # no limit: the golden's rows of this class
            lo = int(g[variant + "/counts"][:j].sum())
            check_voted(g[variant + "/cls_boxes"][lo:lo + len(top)], want, votes, mx, vote[1],
                        reference_yardstick() if yard else None)


def _sweep_inputs(n, c, seed, kind):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
    boxes = np.stack([x1, y1, x1 + rng.uniform(4, 150, n), y1 + rng.uniform(4, 150, n)], 1)
    boxes = (np.round(boxes * 4) / 4).astype(np.float32)
    scores = rng.uniform(0, 1, (n, c)).astype(np.float32) ** 4
    if kind == "ties":
        scores = (rng.randint(1, 6, (n, c)) / np.float32(8)).astype(np.float32)
    elif kind == "identical":
        boxes[:] = boxes[0]
    elif kind == "none":
        scores[:] = np.float32(1e-5)                                  # the compare is strict
    return scores, boxes


def _device_vs_restatement(scores, boxes, D, soft, vote=None, thr=1e-5, nms=0.3):
    from cim_amd import detect
    det = detect.postprocess(_dev(scores), _dev(boxes), thr, nms, D, soft_nms=None if soft is None else
                             dict(method=soft[0], sigma=soft[1]), box_vote=None if vote is None else
                             dict(thresh=vote[0], scoring_method=vote[1], beta=vote[2]))
    idx, cls, sc, count, bx = detect.softvote_to_host(det)
    w_idx, w_cls, w_dets, w_count, w_votes, w64 = softvote_np.postprocess(scores, boxes, thr, nms, D, soft=soft, vote=vote)
    assert np.array_equal(count, w_count) and np.array_equal(idx, w_idx) and np.array_equal(cls, w_cls)
    if vote is None:
        assert np.array_equal(_bits(sc), _bits(w_dets[:, 4])) and np.array_equal(_bits(bx), _bits(w_dets[:, :4]))
    else:
        check_voted(np.hstack((bx, sc[:, None])), w64, w_votes, float(np.abs(boxes).max()), vote[1])
    return int(count.sum())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("c", [1, 20])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2000])
def test_sweep_against_the_restatement(n, c, method):
    scores, boxes = _sweep_inputs(n, c, 1000 * n + c, "plain")
    for D in (100, 0) if n * c <= 2000 else (100,):                    # (the host restatement takes seconds at 2000 x 20)
        _device_vs_restatement(scores, boxes, D, (method, 0.5))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["ties", "identical", "none"])
def test_sweep_ties_identical_boxes_and_nothing_above_threshold(kind, method):
    for n, c in ((65, 1), (257, 20), (1100, 3)):
        scores, boxes = _sweep_inputs(n, c, 77 + n, kind)
        for D in (100, 0):
            kept = _device_vs_restatement(scores, boxes, D, (method, 0.5))
            if kind == "none":
                assert kept == 0
            if kind == "identical" and method == "hard" and D == 0:
                assert kept == c


def test_sweep_voting_against_the_restatement():
    scores, boxes = _sweep_inputs(257, 3, 9, "plain")
    for soft in (None, ("linear", 0.5)):
        if soft is None:                                               # the greedy pass: tie-free by construction here
            assert all(len(np.unique(scores[:, j])) == len(scores) for j in range(3))
        for m in ("ID",) + SUM_ONLY:
            _device_vs_restatement(scores, boxes, 40, soft, (0.5, m, 1.0))


def test_capacity_hard_on_heavily_clustered_boxes():
    rng = np.random.RandomState(3)
    n = 8192
    centre = rng.randint(0, 4, n)
    base = np.array([[10, 10, 110, 90], [300, 20, 380, 140], [40, 300, 200, 420], [320, 320, 400, 380]], np.float32)
    boxes = base[centre] + rng.randint(-3, 4, (n, 4)).astype(np.float32)
    scores = rng.uniform(0.01, 1, (n, 2)).astype(np.float32)
    kept = _device_vs_restatement(scores, boxes, 0, ("hard", 0.5))
    assert 8 <= kept <= 64


def test_capacity_linear_on_a_disjoint_grid():
    """The worst case: nothing decays, nothing is removed - 8192 selection steps in one workgroup."""
    n = 8192
    k = np.arange(n)
    boxes = np.stack([(k % 128) * 20.0, (k // 128) * 20.0, (k % 128) * 20.0 + 9, (k // 128) * 20.0 + 9], 1).astype(np.float32)
    scores = np.random.RandomState(4).uniform(0.01, 1, (n, 2)).astype(np.float32)
    scores[::5, 1] = np.float32(0.25)                                  # ties: the first position wins
    assert _device_vs_restatement(scores, boxes, 0, ("linear", 0.5)) == 2 * n


def test_zero_width_top_box_raises_zero_division():
    from cim_amd.core import test as core_test
    with _Cfg(2, 1e-5, 0.3, 100, None, (0.8, "ID", 1.0)):
        with pytest.raises(ZeroDivisionError):
            core_test.box_results_with_nms_and_limit(ZERO_WIDTH["scores"], ZERO_WIDTH["boxes"])
    with _Cfg(2, 1e-5, 0.3, 100, ("linear", 0.5), None):               # without voting the box is an ordinary detection
        _, _, cb = core_test.box_results_with_nms_and_limit(ZERO_WIDTH["scores"], ZERO_WIDTH["boxes"])
    assert [len(a) for a in cb[1:]] == [2, 2]


def test_negative_score_threshold_with_voting_raises_value_error():
    from cim_amd.core import test as core_test
    g = GOLDENS["n65"]
    with _Cfg(3, -1.0, 0.3, 100, None, (0.8, "ID", 1.0)):
        with pytest.raises(ValueError, match="score_thr >= 0"):
            core_test.box_results_with_nms_and_limit(g["scores"], g["boxes"])


def test_two_streams_give_the_bits_of_one():
    from cim_amd import detect
    g = GOLDENS["vote"]
    s, b = _dev(g["scores"]), _dev(g["boxes"])
    kw = dict(soft_nms=dict(method="gaussian"), box_vote=dict(thresh=0.5, scoring_method="TEMP_AVG"))
    one = detect.softvote_to_host(detect.postprocess(s, b, 1e-5, 0.3, 50, **kw))
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    dets = []
    for st in streams:
        with torch.cuda.stream(st):
            dets.append(detect.postprocess(s, b, 1e-5, 0.3, 50, **kw))
    torch.cuda.synchronize()
    for d in dets:
        got = detect.softvote_to_host(d)
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32
                                  else y) for x, y in zip(got, one))


def test_keys_off_is_the_existing_path_bit_for_bit():
    from cim_amd import detect
    from cim_amd.core import test as core_test
    g = DETECT_GOLDENS["degenerate"]
    thr, nms, D = g["params"]
    C = g["scores"].shape[1]
    with _Cfg(C, thr, nms, D, None, None):
        s, b, cb = core_test.box_results_with_nms_and_limit(g["scores"], g["boxes"])
    idx, cls, sc, count = detect.to_host(detect.nms_limit(_dev(g["scores"]), _dev(g["boxes"]), thr, nms, int(D)))
    assert np.array_equal([len(a) for a in cb[1:]], count)
    assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(np.hstack((g["boxes"][idx], sc[:, None]))))
    assert np.array_equal(_bits(np.vstack(cb[1:])), _bits(g["nms_cls_boxes"]))
    # and the greedy kind of the new entry point gives the same records
    i2, c2, s2, n2, b2 = detect.softvote_to_host(detect.postprocess(_dev(g["scores"]), _dev(g["boxes"]), thr, nms, int(D)))
    assert np.array_equal(i2, idx) and np.array_equal(c2, cls) and np.array_equal(_bits(s2), _bits(sc)) and np.array_equal(n2, count)
    assert np.array_equal(_bits(b2), _bits(g["boxes"][idx]))
