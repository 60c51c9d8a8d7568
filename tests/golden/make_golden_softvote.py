#!/usr/bin/env python3
"""Capture the soft-NMS / box-voting goldens by RUNNING THE REFERENCE (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_softvote.py      # rewrites tests/golden/softvote_*.npz

Runs the reference's own lib/core/test.py `box_results_with_nms_and_limit` with TEST.SOFT_NMS / TEST.BBOX_VOTE set, and
lib/utils/boxes.py `soft_nms` / `box_voting`, on top of the reference's REAL compiled lib/utils/cython_nms.pyx and
lib/utils/cython_bbox.pyx: both are compiled at capture time in a temporary directory (cythonize -3, gcc), cython_nms.pyx
after the two-token NumPy-2 edit of make_golden_detect.py, cython_bbox.pyx as it is.  Nothing of the reference is written
into this repository.

Before anything is written the script asserts, against the compiled reference:
  - the partition form and the loop form of the restatement (softvote_np.py) equal the reference's soft_nms bit for bit on
    3000 random small cases (K <= 40, low-entropy scores, heavy clustering, all three methods);
  - every gaussian golden is robust: no weight's double-precision exp lies within 2^-40 relative of an fp32 rounding
    boundary, so an exp that is 1 ulp off in double still rounds to the same fp32 (a case that violates it is re-drawn).

Soft-NMS resolves equal scores by array position, so ties ARE in these goldens; the cases that go through the greedy pass
(voting after plain NMS) are tie-free, as in make_golden_detect.py.  Files are written with fixed zip timestamps.
"""
import importlib
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402
import make_golden_detect as mgd  # noqa: E402
import softvote_np  # noqa: E402

F32 = np.float32


def build_cython_bbox(tmp):
    src = open(os.path.join(_ref_shims.REF_ROOT, "lib", "utils", "cython_bbox.pyx")).read()
    assert src.count("np.int") == 0 and src.count("np.float)") == 0, "cython_bbox.pyx changed: review the edit"
    pyx = os.path.join(tmp, "cython_bbox.pyx")
    with open(pyx, "w") as f:
        f.write(src)
    subprocess.check_call(["cythonize", "-3", "-q", pyx], cwd=tmp)
    so = os.path.join(tmp, "cython_bbox" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O2", "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(),
                           os.path.join(tmp, "cython_bbox.c"), "-o", so])
    spec = importlib.util.spec_from_file_location("cython_bbox", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def install(tmp):
    cfg, ref_test, _ = mgd.install(tmp)
    bbox = build_cython_bbox(tmp)
    sys.modules["utils.cython_bbox"] = bbox
    ref_boxes = importlib.import_module("utils.boxes")
    ref_boxes.cython_bbox = bbox
    ref_boxes.bbox_overlaps = bbox.bbox_overlaps
    return cfg, ref_test, ref_boxes


# ---------------------------------------------------------------- inputs
def cluster_boxes(rng, n, clusters, jitter=6.0, size=600.0):
    """n boxes around `clusters` centres: many removals per selection step."""
    cx = rng.uniform(50, size - 150, clusters)
    cy = rng.uniform(50, size - 150, clusters)
    w = rng.uniform(30, 120, clusters)
    h = rng.uniform(30, 120, clusters)
    k = rng.randint(0, clusters, n)
    d = rng.uniform(-jitter, jitter, (n, 4))
    b = np.stack([cx[k] + d[:, 0], cy[k] + d[:, 1], cx[k] + w[k] + d[:, 2], cy[k] + h[k] + d[:, 3]], 1)
    b[: n // 2] = np.floor(b[: n // 2])
    b[n // 2:] = np.round(b[n // 2:] * 4) / 4
    return b.astype(F32)


def low_entropy_scores(rng, n, c, levels=6):
    """Scores from a few values: exact ties inside every class."""
    vals = (np.arange(1, levels + 1) / F32(levels + 1)).astype(F32)
    return vals[rng.randint(0, levels, (n, c))]


CASE_NAMES = ("k1", "n63", "n64", "n65", "n255", "n257", "ties", "identical", "disjoint_low", "clustered", "degenerate",
              "limit_exact", "limit_plus1", "limit_tie", "vote", "vote_limit", "empty")


def make_case(name, attempt):
    """dict(scores, boxes, thr, nms, D, variants) of one case, drawn from its own stream (attempt > 0: a re-draw after the
    gaussian robustness condition failed); a variant is 'greedy' or 'soft-<method>[@sigma]', optionally followed by
    '+vote-<thresh>-<scoring>'."""
    rng = np.random.RandomState(20261019 + 1000 * CASE_NAMES.index(name) + attempt)
    lim = np.random.RandomState(20261019)                              # the three limit cases share their scores
    soft3 = ["soft-hard", "soft-linear", "soft-gaussian"]
    out = {}
    # (two classes: the reference's flat arrays need NUM_CLASSES >= 2; the second class has its one candidate, K = 1)
    out["k1"] = dict(scores=np.array([[1e-6, 0.5]], F32), boxes=np.array([[10, 10, 50, 60]], F32), thr=1e-5, nms=0.3, D=100,
                     variants=soft3 + ["soft-linear+vote-0.8-AVG", "greedy+vote-0.8-ID"])
    for n in (63, 64, 65, 255, 257):
        v = soft3 if n in (65, 257) else [soft3[n % 3]]
        out["n%d" % n] = dict(scores=mgd.make_scores(rng, n, 3), boxes=cluster_boxes(rng, n, 6), thr=1e-5, nms=0.3, D=100,
                              variants=v)
    out["ties"] = dict(scores=low_entropy_scores(rng, 200, 4), boxes=cluster_boxes(rng, 200, 5), thr=1e-5, nms=0.3, D=0,
                       variants=soft3 + ["soft-gaussian@0.3", "soft-linear+vote-0.5-IOU_AVG"])
    same = np.tile(np.array([[20, 30, 120, 90]], F32), (70, 1))
    out["identical"] = dict(scores=low_entropy_scores(rng, 70, 2, 3), boxes=same, thr=1e-5, nms=0.3, D=0, variants=soft3)
    # disjoint boxes with scores between SCORE_THRESH and the soft-NMS minimum 1e-4: nothing overlaps, nothing is removed
    low = (rng.uniform(1.5e-5, 9e-5, (80, 2))).astype(F32)
    low[::7] = F32(5e-6)
    out["disjoint_low"] = dict(scores=low, boxes=mgd.grid_boxes(80), thr=1e-5, nms=0.3, D=0, variants=soft3)
    # heavy clustering: two centres, many removals in one step (the hole-filling order)
    out["clustered"] = dict(scores=mgd.make_scores(rng, 400, 2), boxes=cluster_boxes(rng, 400, 2, jitter=3.0), thr=1e-5,
                            nms=0.3, D=0, variants=soft3 + ["soft-hard+vote-0.8-QUASI_SUM"])
    b = mgd.make_boxes(rng, 64)
    b[0:8, 2] = b[0:8, 0] - 1                      # zero width
    b[8:16, 2] = b[8:16, 0] - 5                    # negative width
    b[16:24] = b[16]
    b[16:24, 2] = b[16, 0] - 1                     # identical, zero area
    b[24:28, 3] = b[24:28, 1] - 3                  # negative height
    out["degenerate"] = dict(scores=mgd.make_scores(rng, 64, 6), boxes=b, thr=1e-5, nms=0.3, D=100, variants=soft3)
    # the limit on decayed scores: 3 classes x 40 disjoint boxes, globally distinct scores -> 120 kept
    vals = ((lim.permutation(120) + 1) / F32(128)).astype(F32).reshape(40, 3)
    out["limit_exact"] = dict(scores=vals, boxes=mgd.grid_boxes(40), thr=1e-5, nms=0.3, D=120, variants=["soft-linear"])
    out["limit_plus1"] = dict(scores=vals, boxes=mgd.grid_boxes(40), thr=1e-5, nms=0.3, D=119, variants=["soft-linear"])
    tie = vals.copy()
    flat = np.sort(tie.ravel())[::-1]
    v = flat[59]
    (_, cv), = np.argwhere(tie == v)
    for u in flat[60:]:
        (pu, cu), = np.argwhere(tie == u)
        if cu != cv:
            tie[pu, cu] = v
            break
    out["limit_tie"] = dict(scores=tie, boxes=mgd.grid_boxes(40), thr=1e-5, nms=0.3, D=60, variants=["soft-gaussian"])
    # voting: every scoring method at both thresholds, after the greedy pass (tie-free) and after soft-NMS
    vs = mgd.untie(mgd.make_scores(rng, 300, 4), 1e-5, rng)
    allv = ["%s+vote-%s-%s" % (k, t, m) for m in softvote_np.SCORING for k, t in (("greedy", "0.8"), ("soft-linear", "0.5"))]
    out["vote"] = dict(scores=vs, boxes=cluster_boxes(rng, 300, 8), thr=1e-5, nms=0.3, D=0,
                       variants=allv + ["greedy+vote-0.5-TEMP_AVG", "soft-gaussian+vote-0.8-GENERALIZED_AVG"])
    # a non-ID scoring method under an active limit: the limit sees the re-scored detections
    out["vote_limit"] = dict(scores=mgd.untie(mgd.make_scores(rng, 150, 3), 1e-5, rng), boxes=cluster_boxes(rng, 150, 10),
                             thr=1e-5, nms=0.3, D=12, variants=["greedy+vote-0.5-AVG", "soft-linear+vote-0.5-AVG",
                                                                "greedy+vote-0.5-ID"])
    out["empty"] = dict(scores=np.full((50, 4), F32(2e-6), F32), boxes=mgd.make_boxes(rng, 50), thr=1e-5, nms=0.3, D=100,
                        variants=["soft-linear", "soft-hard+vote-0.8-AVG"])
    return out[name]


def big_case(attempt):
    rng = np.random.RandomState(20261020 + attempt)
    return dict(scores=mgd.make_scores(rng, 1000, 20), boxes=mgd.make_boxes(rng, 1000), thr=1e-5, nms=0.3, D=100,
                variants=["soft-hard", "soft-linear", "soft-gaussian", "soft-linear+vote-0.8-AVG", "greedy+vote-0.8-ID"])


def parse_variant(v):
    """-> (soft method or None, sigma, vote (thresh, scoring) or None)"""
    nms_part, _, vote_part = v.partition("+vote-")
    soft, sigma = None, 0.5
    if nms_part != "greedy":
        name, _, sg = nms_part[len("soft-"):].partition("@")
        soft, sigma = name, float(sg) if sg else 0.5
    vote = None
    if vote_part:
        th, _, m = vote_part.partition("-")
        vote = (float(th), m)
    return soft, sigma, vote


def set_cfg(cfg, case, variant):
    soft, sigma, vote = parse_variant(variant)
    cfg.MODEL.NUM_CLASSES = case["scores"].shape[1]
    cfg.TEST.SCORE_THRESH = case["thr"]
    cfg.TEST.NMS = case["nms"]
    cfg.TEST.DETECTIONS_PER_IM = case["D"]
    cfg.TEST.SOFT_NMS.ENABLED = soft is not None
    cfg.TEST.SOFT_NMS.METHOD = soft or "linear"
    cfg.TEST.SOFT_NMS.SIGMA = sigma
    cfg.TEST.BBOX_VOTE.ENABLED = vote is not None
    cfg.TEST.BBOX_VOTE.VOTE_TH = vote[0] if vote else 0.8
    cfg.TEST.BBOX_VOTE.SCORING_METHOD = vote[1] if vote else "ID"
    return soft, sigma, vote


def gaussian_robust(args):
    """No exp(arg) (double) within 2^-40 relative of the midpoint between two neighbouring fp32 values."""
    a = np.concatenate([np.ravel(x) for x in args]).astype(np.float64) if args else np.zeros(0)
    a = a[np.isfinite(a)]
    y = np.exp(a)
    f = y.astype(F32)
    up = (f.astype(np.float64) + np.nextafter(f, F32(np.inf)).astype(np.float64)) / 2
    dn = (f.astype(np.float64) + np.nextafter(f, F32(-np.inf)).astype(np.float64)) / 2
    gap = np.minimum(np.abs(y - up), np.abs(y - dn))
    return bool(np.all(gap > 2.0 ** -40 * y))


def capture(cfg, ref_test, case):
    sc, bx = case["scores"], case["boxes"]
    rec = dict(scores=sc, boxes=bx, params=np.array([case["thr"], case["nms"], case["D"]], np.float64),
               variants=np.array(case["variants"]))
    for v in case["variants"]:
        soft, sigma, vote = set_cfg(cfg, case, v)
        if soft is None:
            mgd.assert_tie_free(sc, case["thr"])
        if soft == "gaussian":                                         # the robustness condition, on the restatement's weights
            softvote_np.GAUSS_ARGS = []
            softvote_np.postprocess(sc, bx, case["thr"], case["nms"], case["D"], soft=(soft, sigma))
            ok = gaussian_robust(softvote_np.GAUSS_ARGS)
            softvote_np.GAUSS_ARGS = None
            if not ok:
                return None                                             # re-draw
        s, b, cb = ref_test.box_results_with_nms_and_limit(sc, bx)
        assert len(cb) == sc.shape[1] + 1 and isinstance(cb[0], list) and cb[0] == []
        arrs = [np.asarray(a, F32).reshape(-1, 5) for a in cb[1:]]
        rec[v + "/cls_boxes"] = np.vstack(arrs).astype(F32)
        rec[v + "/counts"] = np.array([len(a) for a in arrs], np.int32)
        rec[v + "/out_scores"], rec[v + "/out_boxes"] = np.asarray(s, F32), np.asarray(b, F32)
    return rec


def drawn(cfg, ref_test, make):
    """The first draw of a case whose gaussian variants are robust."""
    for attempt in range(20):
        case = make(attempt)
        rec = capture(cfg, ref_test, case)
        if rec is not None:
            if attempt:
                print("  (re-drawn %d times for the gaussian robustness condition)" % attempt)
            return case, rec
    raise AssertionError("no robust draw in 20 attempts")


def check_partition(ref_boxes):
    """The claim the kernel rests on, against the compiled reference."""
    rng = np.random.RandomState(7)
    for it in range(3000):
        k = rng.randint(1, 41)
        dets = np.hstack((cluster_boxes(rng, k, rng.randint(1, 4), jitter=rng.choice([1.0, 4.0, 15.0])),
                          low_entropy_scores(rng, k, 1, rng.randint(2, 6)) * F32(rng.choice([1.0, 0.01, 0.0005]))))
        method = ("hard", "linear", "gaussian")[it % 3]
        thresh = float(rng.choice([0.001, 0.0001, 0.05]))
        want_d, want_i = ref_boxes.soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=thresh, method=method)
        for form in (softvote_np.soft_nms, softvote_np.soft_nms_loop):
            got_d, got_i = form(dets, 0.5, 0.3, thresh, softvote_np.METHODS[method])
            assert np.array_equal(np.asarray(want_i), got_i), (it, method, form.__name__)
            assert np.array_equal(np.asarray(want_d, F32).view(np.uint32), got_d.view(np.uint32)), (it, method, form.__name__)


def standalone(ref_boxes):
    """soft_nms / box_voting called directly: defaults, beta != 1, top boxes that are not among the voters."""
    rng = np.random.RandomState(11)
    rec = {}
    dets = np.hstack((cluster_boxes(rng, 120, 4), low_entropy_scores(rng, 120, 1, 9)))
    for m in ("hard", "linear", "gaussian"):
        if m == "gaussian":
            softvote_np.GAUSS_ARGS = []
            softvote_np.soft_nms(dets, 0.5, 0.3, 0.001, 2)
            assert gaussian_robust(softvote_np.GAUSS_ARGS)
            softvote_np.GAUSS_ARGS = None
        d, k = ref_boxes.soft_nms(dets, method=m)
        rec["soft/%s/dets" % m], rec["soft/%s/keep" % m] = np.asarray(d, F32), np.asarray(k, np.int64)
    rec["soft/dets_in"] = dets
    alld = np.hstack((cluster_boxes(rng, 200, 5), rng.uniform(0.01, 0.99, (200, 1)).astype(F32)))
    top = alld[rng.choice(200, 12, replace=False)].copy()
    top[:, :4] += rng.uniform(-2, 2, (12, 4)).astype(F32)              # not among the voters
    rec["vote/all"], rec["vote/top"] = alld, top
    calls = [("ID", 1.0, 0.5), ("AVG", 1.0, 0.5), ("IOU_AVG", 1.0, 0.6), ("QUASI_SUM", 0.5, 0.5),
             ("GENERALIZED_AVG", 2.0, 0.5), ("TEMP_AVG", 0.5, 0.5)]
    rec["vote/calls"] = np.array(["%s %r %r" % c for c in calls])
    for m, beta, th in calls:
        rec["vote/%s/out" % m] = np.asarray(ref_boxes.box_voting(top, alld, th, scoring_method=m, beta=beta), F32)
    return rec


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cfg, ref_test, ref_boxes = install(tmp)
        check_partition(ref_boxes)
        print("partition form == loop form == compiled reference on 3000 cases")
        # a zero-width top box has no voter: the reference raises
        z = dict(scores=np.array([[0.5, 0.2], [0.4, 0.3]], F32), boxes=np.array([[10, 10, 9, 40], [50, 50, 80, 90]], F32), thr=1e-5,
                 nms=0.3, D=100)
        set_cfg(cfg, z, "greedy+vote-0.8-ID")
        try:
            ref_test.box_results_with_nms_and_limit(z["scores"], z["boxes"])
            raise AssertionError("the reference did not raise for an empty vote set")
        except ZeroDivisionError:
            pass
        small = {}
        for name in CASE_NAMES:
            case, rec = drawn(cfg, ref_test, lambda a: make_case(name, a))
            print(name, {v: int(rec[v + "/counts"].sum()) for v in case["variants"]})
            small.update({name + "/" + k: v for k, v in rec.items()})
        small.update({"zero_width/" + k: z[k] for k in ("scores", "boxes")})
        mgd.save_npz(os.path.join(HERE, "softvote_cases.npz"), small)
        mgd.save_npz(os.path.join(HERE, "softvote_n1000_c20.npz"), drawn(cfg, ref_test, big_case)[1])
        mgd.save_npz(os.path.join(HERE, "softvote_direct.npz"), standalone(ref_boxes))


if __name__ == "__main__":
    main()
