#!/usr/bin/env python3
"""Capture the VOC box-evaluation golden by RUNNING THE REFERENCE (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_box_eval.py      # rewrites tests/golden/box_eval_voc.npz

Runs the reference's own lib/datasets/voc_eval.py `voc_eval` (both AP forms) and lib/datasets/dis_eval.py `dis_eval` on a
small synthetic dataset written to a temporary directory (box_eval_np.write_voc_files: XML annotations, image set,
per-class results files), on the CPU.  The two modules are loaded from their files with two stand-ins for what this
container lacks: six.moves.cPickle (the standard pickle) and np.bool (removed from NumPy; voc_eval.py:152).  Nothing of
the reference is written into this repository.

Inputs are stored next to the outputs.  Confidences stay distinct within a class after '{:.3f}' (asserted), so the
reference's unstable argsort has one answer; ties are tested against the restatement (box_eval_np.py) on the device
instead.  Coordinates are multiples of 0.25 below 1024, so x + 1 is exact in fp32 and in fp64.  The .npz is written with
fixed zip timestamps: a rerun is byte-identical.
"""
import importlib.util
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402
import box_eval_np  # noqa: E402
from make_golden_detect import save_npz  # noqa: E402

CLASSES = ["alpha", "beta", "gamma", "nogt", "nodet"]


def case():
    """8 images, 5 classes: three ordinary ones (difficult ground truths, several detections on one ground truth, images
    without ground truth, ground truths without detection), one with detections and no ground truth at all (npos = 0), one
    with ground truth and no detection."""
    rng = np.random.RandomState(20261017)
    names = ["img_%03d" % i for i in range(8)]
    gt_img, gt_cls, gt_box, gt_diff, dt_img, dt_cls, dets = [], [], [], [], [], [], []
    for k in range(5):
        cls_dets = []
        for i in range(8):
            n_gt = 0 if k == 3 else int(rng.randint(0, 4))
            boxes = []
            for _ in range(n_gt):
                x, y = rng.randint(1, 300, 2)
                w, h = rng.randint(20, 200, 2)
                boxes.append((x, y, x + w, y + h))
                gt_img.append(i), gt_cls.append(k), gt_box.append(boxes[-1]), gt_diff.append(int(rng.rand() < 0.25))
            if k == 4:
                continue
            for b in boxes:                                              # 0-3 jittered copies of every ground truth
                for _ in range(int(rng.randint(0, 4))):
                    j = np.round(rng.uniform(-0.2, 0.2, 4) * (b[2] - b[0]) * 4) / 4
                    cls_dets.append((i, np.asarray(b, np.float64) - 1 + j))
            for _ in range(int(rng.randint(0, 3))):                      # and stray boxes
                x, y = np.round(rng.uniform(0, 300, 2) * 4) / 4
                w, h = np.round(rng.uniform(10, 200, 2) * 4) / 4
                cls_dets.append((i, np.array([x, y, x + w, y + h])))
        conf = (rng.permutation(997)[:len(cls_dets)] + 1) / 1000.0 + rng.uniform(-4e-4, 4e-4, len(cls_dets))
        for (i, b), c in zip(cls_dets, conf):
            b = np.clip(b, 0, 1000)
            dt_img.append(i), dt_cls.append(k), dets.append(np.r_[b, c])
    out = dict(classes=np.asarray(CLASSES), imagenames=np.asarray(names), gt_img=np.asarray(gt_img, np.int32),
               gt_cls=np.asarray(gt_cls, np.int32), gt_box=np.asarray(gt_box, np.int32).reshape(-1, 4),
               gt_diff=np.asarray(gt_diff, np.uint8), dt_img=np.asarray(dt_img, np.int32), dt_cls=np.asarray(dt_cls, np.int32),
               dets=np.asarray(dets, np.float32).reshape(-1, 5))
    for k in range(5):
        c = ["%.3f" % float(v) for v in out["dets"][out["dt_cls"] == k, 4]]
        assert len(set(c)) == len(c), "confidences of class %d tie after the text round trip" % k
    b = out["dets"][:, :4].astype(np.float64)
    assert np.array_equal(b * 4, np.round(b * 4)) and b.max() < 1024
    return out


def load_reference(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(_ref_shims.REF_ROOT, "lib", "datasets", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def capture(data):
    _ref_shims._module("six")
    _ref_shims._module("six.moves", cPickle=__import__("pickle"))
    if not hasattr(np, "bool"):
        np.bool = bool                                                   # voc_eval.py:152
    ref_voc, ref_dis = load_reference("voc_eval"), load_reference("dis_eval")
    K = len(data["classes"])
    rec, prec, off = [], [], [0]
    ap07, ap, corloc = np.zeros(K), np.zeros(K), np.zeros(K)
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # 0 / 0 of the class without ground truth
        detpath, annopath, imageset = box_eval_np.write_voc_files(tmp, data)
        for k, cls in enumerate(data["classes"]):
            r7, p7, ap07[k] = ref_voc.voc_eval(detpath, annopath, imageset, str(cls), os.path.join(tmp, "cache"), 0.5, True)
            r, p, ap[k] = ref_voc.voc_eval(detpath, annopath, imageset, str(cls), os.path.join(tmp, "cache"), 0.5, False)
            corloc[k] = ref_dis.dis_eval(detpath, annopath, imageset, str(cls), os.path.join(tmp, "cache_dis"), 0.5)
            if isinstance(r, np.ndarray):
                assert np.array_equal(r, r7, equal_nan=True) and np.array_equal(p, p7)
                rec.append(r), prec.append(p)
            else:
                assert (r, p, ap[k], r7, p7, ap07[k]) == (0, 0, 0, 0, 0, 0)
            off.append(off[-1] + (len(r) if isinstance(r, np.ndarray) else 0))
    return dict(rec=np.concatenate(rec), prec=np.concatenate(prec), cls_off=np.asarray(off, np.int64), ap07=ap07, ap=ap,
                corloc=corloc)


def main():
    data = case()
    out = capture(data)
    print("detections per class", np.bincount(data["dt_cls"], minlength=5), "ap07", out["ap07"], "ap", out["ap"], "corloc",
          out["corloc"])
    save_npz(os.path.join(HERE, "box_eval_voc.npz"), dict(data, **out))


if __name__ == "__main__":
    main()
