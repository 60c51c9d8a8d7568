#!/usr/bin/env python3
"""Capture the detection post-processing goldens by RUNNING THE REFERENCE (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_detect.py      # rewrites tests/golden/detect_*.npz

Runs the reference's own lib/core/test.py `box_results_with_nms_and_limit` / `box_results_for_corloc` and
lib/utils/mask_eval_utils.py `mask_results_with_nms_and_limit_get_index`, on top of the reference's REAL compiled greedy
NMS: lib/utils/cython_nms.pyx is compiled at capture time in a temporary directory (cythonize -3, gcc), after a two-token
edit in memory - np.int_t -> np.intp_t and dtype=np.int -> dtype=np.intp, the same 64-bit integer on this platform, for
NumPy 2 (the arithmetic is untouched).  Nothing of the reference is written into this repository.

Inputs are stored next to the outputs.  Every input is tie-free within a class's candidates (asserted): the reference's
argsort leaves the order of equal scores to the NumPy build, so ties are tested against the restatement
(tests/golden/detect_np.py) on the device instead.  The .npz files are written with fixed zip timestamps so a rerun is
byte-identical.
"""
import importlib
import importlib.util
import io
import os
import subprocess
import sys
import sysconfig
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402

F32 = np.float32


def build_cython_nms(tmp):
    src = open(os.path.join(_ref_shims.REF_ROOT, "lib", "utils", "cython_nms.pyx")).read()
    assert src.count("np.int_t") == 2 and src.count("dtype=np.int)") == 1, "cython_nms.pyx changed: review the edit"
    src = src.replace("np.int_t", "np.intp_t").replace("dtype=np.int)", "dtype=np.intp)")
    pyx = os.path.join(tmp, "cython_nms.pyx")
    with open(pyx, "w") as f:
        f.write(src)
    subprocess.check_call(["cythonize", "-3", "-q", pyx], cwd=tmp)
    so = os.path.join(tmp, "cython_nms" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O2", "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(),
                           os.path.join(tmp, "cython_nms.c"), "-o", so])
    spec = importlib.util.spec_from_file_location("cython_nms", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def install(tmp):
    _ref_shims.install()
    _ref_shims._module("cv2")
    _ref_shims._module("six.moves", cPickle=__import__("pickle"))
    _ref_shims._module("pycocotools")
    sys.modules["pycocotools"].mask = _ref_shims._module("pycocotools.mask")      # only coco_encode uses it

    def _bbox_unavailable(*a, **k):
        raise RuntimeError("cython_bbox: not on the post-processing path")

    _ref_shims._module("utils.cython_bbox", bbox_overlaps=_bbox_unavailable)
    sys.modules["utils.cython_nms"] = build_cython_nms(tmp)
    np.float, np.int = float, int                      # removed NumPy aliases the reference still uses
    cfg = importlib.import_module("core.config").cfg
    if cfg.is_immutable():
        cfg.immutable(False)
    return (cfg, importlib.import_module("core.test"), importlib.import_module("utils.mask_eval_utils"))


# ---------------------------------------------------------------- inputs
def make_boxes(rng, n, size=600.0):
    """Half integer, half fractional (quarter-pixel) boxes, sizes from a few pixels to half the image."""
    x1 = rng.uniform(0, size * 0.8, n)
    y1 = rng.uniform(0, size * 0.8, n)
    w = rng.uniform(4, size * 0.5, n)
    h = rng.uniform(4, size * 0.5, n)
    b = np.stack([x1, y1, x1 + w, y1 + h], 1)
    half = n // 2
    b[:half] = np.floor(b[:half])
    b[half:] = np.round(b[half:] * 4) / 4
    return b.astype(F32)


def make_scores(rng, n, c):
    """cls_score (softmax over classes) * iou_score (sigmoid), the form of the refinement heads' product."""
    logits = rng.randn(n, c) * 3
    e = np.exp(logits - logits.max(1, keepdims=True))
    cls = e / e.sum(1, keepdims=True)
    iou = 1 / (1 + np.exp(-rng.randn(n, c) * 2))
    return (cls * iou).astype(F32)


def untie(scores, thr, rng):
    """Nudge equal scores of one class apart by one ulp until every class's candidates are distinct."""
    s = scores.copy()
    for j in range(s.shape[1]):
        while True:
            col = s[:, j]
            cand = col[col > F32(thr)]
            vals, cnt = np.unique(cand, return_counts=True)
            dup = vals[cnt > 1]
            if not len(dup):
                break
            for v in dup:
                at = np.where(col == v)[0][1:]
                s[at, j] = np.nextafter(v, F32(np.inf)) if rng.rand() < 0.5 else np.nextafter(v, F32(0))
    return s


def assert_tie_free(scores, thr):
    for j in range(scores.shape[1]):
        cand = scores[scores[:, j] > F32(thr), j]
        assert len(np.unique(cand)) == len(cand), "ties within class %d" % j


def grid_boxes(n):
    """Disjoint boxes (gap > 1 px): NMS keeps every candidate, so the limit alone decides."""
    k = np.arange(n)
    return np.stack([(k % 8) * 20.0, (k // 8) * 20.0, (k % 8) * 20.0 + 9, (k // 8) * 20.0 + 9], 1).astype(F32)


def cases():
    rng = np.random.RandomState(20261016)
    out = {}
    for n, c, name in ((1000, 20, "detect_n1000_c20"), (2000, 80, "detect_n2000_c80")):
        out[name] = dict(scores=untie(make_scores(rng, n, c), 1e-5, rng), boxes=make_boxes(rng, n), thr=1e-5, nms=0.3, D=100)
    ev = np.load(os.path.join(HERE, "e2e_vgg16_voc_eval.npz"))
    s = (ev["refine_score_0"] + ev["refine_score_1"] + ev["refine_score_2"]) / F32(3)   # test.py:131-135
    out["detect_eval_vgg16_voc"] = dict(scores=s.astype(F32), boxes=make_boxes(rng, s.shape[0]), thr=1e-5, nms=0.3, D=100)

    # the limit: 3 classes x 40 disjoint boxes, globally distinct scores -> 120 kept
    vals = ((rng.permutation(120) + 1) / F32(128)).astype(F32).reshape(40, 3)
    out["detect_limit_exact"] = dict(scores=vals, boxes=grid_boxes(40), thr=1e-5, nms=0.3, D=120)     # exactly D kept
    out["detect_limit_plus1"] = dict(scores=vals, boxes=grid_boxes(40), thr=1e-5, nms=0.3, D=119)     # D + 1 kept
    tie = vals.copy()
    flat = np.sort(tie.ravel())[::-1]
    v = flat[59]                                   # the 60th largest ...
    (_, cv), = np.argwhere(tie == v)
    for u in flat[60:]:                            # ... copied onto the next lower score of ANOTHER class
        (pu, cu), = np.argwhere(tie == u)
        if cu != cv:
            tie[pu, cu] = v
            break
    out["detect_limit_tie"] = dict(scores=tie, boxes=grid_boxes(40), thr=1e-5, nms=0.3, D=60)
    # nothing above the threshold (some scores exactly float32(1e-5): the compare is strict)
    none = np.full((50, 4), F32(1e-5), F32)
    none[::3] = F32(2e-6)
    out["detect_empty"] = dict(scores=none, boxes=make_boxes(rng, 50), thr=1e-5, nms=0.3, D=100)
    # degenerate boxes: zero width (area 0), negative widths, identical zero-area boxes (0 / 0 = NaN overlaps)
    b = make_boxes(rng, 64)
    b[0:8, 2] = b[0:8, 0] - 1                      # zero width
    b[8:16, 2] = b[8:16, 0] - 5                    # negative width
    b[16:24] = b[16]                               # identical boxes ...
    b[16:24, 2] = b[16, 0] - 1                     # ... of area 0: ovr = 0 / 0
    b[24:28, 3] = b[24:28, 1] - 3                  # negative height
    out["detect_degenerate"] = dict(scores=untie(make_scores(rng, 64, 6), 1e-5, rng), boxes=b, thr=1e-5, nms=0.3, D=100)
    # a low overlap threshold and no limit
    out["detect_nolimit"] = dict(scores=untie(make_scores(rng, 300, 5), 1e-5, rng), boxes=make_boxes(rng, 300),
                                 thr=0.05, nms=0.1, D=0)
    return out


def flat_cls(cls_boxes):
    """cls_boxes (length C + 1, [0] == []) -> concatenated [sum k, 5] + counts [C]."""
    assert isinstance(cls_boxes[0], list) and cls_boxes[0] == []
    arrs = cls_boxes[1:]
    return np.vstack(arrs).astype(F32), np.array([len(a) for a in arrs], np.int32)


def capture(cfg, ref_test, ref_mask, case):
    sc, bx = case["scores"], case["boxes"]
    assert_tie_free(sc, case["thr"])
    cfg.MODEL.NUM_CLASSES = sc.shape[1]
    cfg.TEST.SCORE_THRESH = case["thr"]
    cfg.TEST.NMS = case["nms"]
    cfg.TEST.DETECTIONS_PER_IM = case["D"]
    assert not cfg.TEST.SOFT_NMS.ENABLED and not cfg.TEST.BBOX_VOTE.ENABLED
    rec = dict(scores=sc, boxes=bx, params=np.array([case["thr"], case["nms"], case["D"]], np.float64))
    s, b, cb = ref_test.box_results_with_nms_and_limit(sc, bx)
    assert len(cb) == sc.shape[1] + 1 and all(a.dtype == F32 and a.shape[1:] == (5,) for a in cb[1:])
    rec["nms_scores"], rec["nms_boxes"] = s, b
    rec["nms_cls_boxes"], rec["nms_counts"] = flat_cls(cb)
    s, b, cb = ref_test.box_results_for_corloc(sc, bx)
    rec["corloc_scores"], rec["corloc_boxes"] = s, b
    rec["corloc_cls_boxes"], _ = flat_cls(cb)
    s, b, cb, ci = ref_mask.mask_results_with_nms_and_limit_get_index(cfg, sc, bx, DETECTIONS_PER_IM=case["D"])
    rec["index_scores"], rec["index_boxes"] = s, b
    rec["index_cls_boxes"], rec["index_counts"] = flat_cls(cb)
    rec["index_inds"] = np.concatenate([np.asarray(a, np.int64) for a in ci[1:]])
    return rec


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps (a rerun gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cfg, ref_test, ref_mask = install(tmp)
        allc = cases()
        small = {}
        for name, case in allc.items():
            rec = capture(cfg, ref_test, ref_mask, case)
            print(name, "kept", int(rec["nms_counts"].sum()), "per class max", int(rec["nms_counts"].max()))
            if name in ("detect_n1000_c20", "detect_n2000_c80", "detect_eval_vgg16_voc"):
                save_npz(os.path.join(HERE, name + ".npz"), rec)
            else:
                small.update({name[len("detect_"):] + "/" + k: v for k, v in rec.items()})
        save_npz(os.path.join(HERE, "detect_cases.npz"), small)


if __name__ == "__main__":
    main()
