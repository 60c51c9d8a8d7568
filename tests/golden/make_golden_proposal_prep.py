#!/usr/bin/env python3
"""Capture the proposal-preprocessing goldens by RUNNING THE REFERENCE (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_proposal_prep.py      # rewrites tests/golden/proposal_prep_*.npz

Drives the reference's own tools/pre/generate_7_7_voc.py `generate_pkl_voc2012`, generate_7_7_coco.py
`generate_pkl_coco2017` and point_level_label_assign.py `assign_voc2012` over seeded masks written as .mat files (and
Center_points .txt files) in a temporary ./data tree, and reads back the pickles they write.  Stubs stand in for what this
host lacks: pycocotools.coco.COCO (an annotation table of ours), chainer.backends.cuda (get_array_module -> numpy), the PRM
network modules that point_level_label_assign imports and never calls, and np.bool where NumPy dropped it.  Nothing of the
reference is written into this repository.

`assign_voc2012` allocates 21 columns whatever the dataset (point_level_label_assign.py:58) and the reference has no COCO
form of it, so every `mat` golden has 21 columns; the COCO-shaped image takes part with classes below 20, and 80-class
matrices are tested against the restatement (proposal_prep_np.py).  AGPL_label_assign.py:154-180 is the same statements
with [:, x, y] indexing behind the PRM network: it is covered by peaks_to_pixels + these goldens rather than run.

Three images:
  voc     97 x 131 (H W a multiple of neither 64 nor 4), 20 classes: boxes of widths / heights at which the closed form
          floor((c + .5) w / 7) differs from Pillow's walk (2, 4, 8, 16, 32, 64, 128) and others, 1-pixel masks, ellipses,
          and a crafted cluster: a point covered by exactly 10 masks with a strip in exactly 7 of them (coverage 7/10: out)
          and one in 8 (in), a proposal at IoU exactly 0.5 (background for that point, assigned by a later one), two
          points assigning the same proposals (the last wins), a point no mask covers (it still uses up a cluster number).
  coco    40 x 1400, the larger widths of the mismatch set, a full-image mask, 80-class layout of the .mat file.
  nopoints  the voc masks with an empty point file (P = 0).
The generator asserts that each of these situations really occurs.  The .npz files are written with fixed zip timestamps
so a rerun is byte-identical.
"""
import importlib
import io
import os
import pickle
import sys
import tempfile
import types
import zipfile

import numpy as np
import scipy.io

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_shims  # noqa: E402
import proposal_prep_np as ppn  # noqa: E402
from cim_amd import synthetic  # noqa: E402

S = 7
VOC_ID, COCO_ID, NOPOINTS_ID = 2008000001, 2009000002, 2010000003


def mismatch_extents(limit, size=S):
    """Extents at which floor((i + .5) e / size) differs from Pillow's accumulated walk."""
    out = []
    for e in range(1, limit + 1):
        closed = np.minimum(((np.arange(size) + 0.5) * e / size).astype(np.int64), e - 1)
        if not np.array_equal(closed, ppn.nearest_index(e, size)):
            out.append(e)
    return out


def rect(h, w, y0, x0, bh, bw, rng, drop=0.3):
    m = np.zeros((h, w), dtype=np.uint8)
    m[y0:y0 + bh, x0:x0 + bw] = rng.rand(bh, bw) >= drop
    m[y0, x0] = m[y0 + bh - 1, x0 + bw - 1] = 1                 # the box is the rectangle whatever was dropped
    return m


def voc_image(rng):
    h, w, top = 97, 131, 55
    masks = []
    bad = set(mismatch_extents(131))
    assert {2, 4, 8, 16, 32, 64, 128} <= bad and not ({1, 3, 5, 7, 13, 50, 100, 131} & bad)
    widths = [2, 4, 8, 16, 32, 64, 128, 1, 3, 5, 7, 13, 50, 100, 131]
    heights = [1, 2, 4, 8, 16, 32, 3, 5, 7, 11, 55]
    for i, bw in enumerate(widths):
        for bh in (heights[i % len(heights)], heights[(3 * i + 5) % len(heights)]):
            masks.append(rect(h, w, rng.randint(0, top - bh + 1), rng.randint(0, w - bw + 1), bh, bw, rng))
    for _ in range(3):                                           # 1-pixel masks
        m = np.zeros((h, w), dtype=np.uint8)
        m[rng.randint(0, top), rng.randint(0, w)] = 1
        masks.append(m)
    ell, _ = synthetic.make_masks(24, top, w, rng, min_side=2)
    for e in ell:
        m = np.zeros((h, w), dtype=np.uint8)
        m[:top] = e
        masks.append(m)
    # ---- the crafted cluster, rows 58..: R = rows 60..79 x cols 10..49 (800 pixels)
    first = len(masks)
    for k in range(10):
        m = np.zeros((h, w), dtype=np.uint8)
        m[60:80, 10:50] = 1
        if k < 7:
            m[60:80, 50:52] = 1                                  # in 7 of 10: coverage exactly 0.7, not above it
        if k < 8:
            m[60:80, 52:54] = 1                                  # in 8 of 10: part of the average mask (840 pixels)
        m[58, 10 + k] = 1                                        # the ten differ
        masks.append(m)
    half = np.zeros((h, w), dtype=np.uint8)                      # 430 pixels inside the average mask + 20 outside:
    half[60:80, 29:50] = 1                                       #   420
    half[60:70, 52] = 1                                          #   + 10 (strip of 8)
    half[81, 60:80] = 1                                          #   20 outside: 430 / (840 + 20) = 0.5 exactly
    masks.append(half)
    half2 = half.copy()
    half2[82, 60:64] = 1
    masks.append(half2)
    extra = np.zeros((h, w), dtype=np.uint8)                     # covers the second point only
    extra[60:80, 10:20] = 1
    masks.append(extra)
    graze = np.zeros((h, w), dtype=np.uint8)                     # small non-zero IoU with every average mask: background
    graze[78:92, 44:50] = 1
    masks.append(graze)
    masks = np.stack(masks)
    # (x, y, class, conf): p0 in R right of `half` and `extra`; p1 in `extra`; p2 uncovered; p3 in the tail of `half`
    points = [(25.5, 65.2, 3, 0.9), (12.0, 70.9, 7, 0.8), (125.7, 95.1, 11, 0.7), (70.3, 81.0, 19, 0.6)]
    assert masks[:, 95, 125].sum() == 0 and masks[:, 65, 25].sum() == 10 and masks[:, 70, 12].sum() == 11
    assert masks[:, 81, 70].sum() == 2
    return masks, points, first


def coco_image(rng):
    h, w = 40, 1400
    bad = [e for e in mismatch_extents(1400) if e > 128]
    good = [7, 700, 1399]
    assert len(mismatch_extents(1399)) == 26 and {256, 512, 1024} <= set(bad)
    masks = [np.ones((h, w), dtype=np.uint8)]                    # the full image
    heights = [1, 2, 4, 8, 16, 32, 40, 9]
    for i, bw in enumerate(bad + good):
        bh = heights[i % len(heights)]
        masks.append(rect(h, w, rng.randint(0, h - bh + 1), rng.randint(0, w - bw + 1), bh, bw, rng, drop=0.2))
    m = np.zeros((h, w), dtype=np.uint8)
    m[39, 1399] = 1
    masks.append(m)
    ell, _ = synthetic.make_masks(20, h, w, rng, min_side=4)
    masks.extend(e.astype(np.uint8) for e in ell)
    masks = np.stack(masks)
    points = [(float(rng.randint(0, w)) + 0.4, float(rng.randint(0, h)) + 0.6, int(rng.randint(0, 20)), 1.0) for _ in range(5)]
    return masks, points


class FakeCOCO(object):
    """pycocotools.coco.COCO as the three functions use it."""
    table = {}                                                   # img_id -> (file_name, [category ids])

    def __init__(self, *a, **k):
        pass

    def getImgIds(self):
        return sorted(self.table)

    def loadImgs(self, img_id):
        return [{"file_name": self.table[img_id][0]}]

    def getAnnIds(self, imgIds=None):
        return [(imgIds, c) for c in self.table[imgIds][1]]

    def loadAnns(self, ann_ids):
        return [{"category_id": c} for _, c in ann_ids]


def install():
    _ref_shims.install()                                         # chainer.backends.cuda -> numpy, among others
    _ref_shims._module("pycocotools")
    sys.modules["pycocotools"].coco = _ref_shims._module("pycocotools.coco", COCO=FakeCOCO)
    # lib/ has no __init__.py: a namespace package with stubs for the PRM modules (imported, never called by assign_voc2012)
    lib = types.ModuleType("lib")
    lib.__path__ = [os.path.join(_ref_shims.REF_ROOT, "lib")]
    sys.modules["lib"] = lib
    prm = types.ModuleType("lib.prm")
    prm.__path__ = []
    sys.modules["lib.prm"] = prm
    _ref_shims._module("lib.prm.prm_model_gt", peak_response_mapping=None, fc_resnet50=None)
    _ref_shims._module("lib.prm.prm_configs", open_transform=None)
    if not hasattr(np, "bool"):
        np.bool = bool                                           # generate_7_7_voc.py:32
    sys.path.insert(0, os.path.join(_ref_shims.REF_ROOT, "tools", "pre"))


def write_voc_mat(masks, img_id, points):
    s = str(img_id)
    name = s[:4] + "_" + s[4:]
    cell = np.empty((len(masks), 1), dtype=object)
    for i, m in enumerate(masks):
        cell[i, 0] = m
    scipy.io.savemat(os.path.join("data", "VOC2012", "COB_SBD_trainaug", name + ".mat"), {"maskmat": cell})
    with open(os.path.join("data", "VOC2012", "Center_points", name + ".txt"), "w") as f:
        for x, y, c, conf in points:
            f.write("%r %r %d %r\n" % (x, y, c, conf))
    FakeCOCO.table[img_id] = (name + ".jpg", sorted({c + 1 for _, _, c, _ in points}))


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps (a rerun gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def record(masks, points, boxes, small, mat):
    bits, shape = ppn.pack_bits(masks)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    return {"mask_bits": bits, "mask_shape": shape, "boxes": boxes, "small": small, "points": pts, "mat": mat}


def check_situations(masks, points, first, mat):
    """The crafted situations of the voc image really occur (seen through the restatement's intermediate values)."""
    n = masks.shape[0]
    flat = masks.reshape(n, -1) != 0
    area = flat.sum(1)
    rows, cols = [int(p[1]) for p in points], [int(p[0]) for p in points]
    ious, nsel, exact = [], [], False
    for r, c in zip(rows, cols):
        sel = flat[:, r * masks.shape[2] + c]
        cnt = flat[sel].sum(0)
        exact = exact or bool(sel.sum() and np.any(10 * cnt == 7 * sel.sum()))
        avg = ppn.covered(cnt, int(sel.sum()))
        inter = (flat & avg[None]).sum(1)
        with np.errstate(invalid="ignore"):
            ious.append((inter / (area + avg.sum() - inter)).astype(np.float32))
        nsel.append(int(sel.sum()))
    assert exact, "no pixel at coverage exactly 7/10"
    assert nsel[0] == 10 and nsel[2] == 0
    half = first + 10
    assert ious[0][half] == np.float32(0.5) and ious[3][half] > 0.5, "the IoU-0.5 proposal"
    assert mat[half, 19 + 1] == 4 and mat[half].sum() == 4, "background for point 0, assigned by point 3 (cluster 4)"
    both = (ious[0] > 0.5) & (ious[1] > 0.5)
    assert both.sum() >= 8 and np.all(mat[both, 3 + 1] == 0) and np.sum(mat[both, 7 + 1] == 2) >= 8, "the last point wins"
    assert np.all(ious[2] == 0), "an uncovered point assigns nothing"
    assert np.any(mat[:, 0] == len(points) + 1), "a background row"
    assert np.any(mat.sum(1) == 0), "an untouched row"


def main():
    install()
    rng = np.random.RandomState(20241)
    voc_masks, voc_points, first = voc_image(rng)
    coco_masks, coco_points = coco_image(rng)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for d in ("VOC2012/COB_SBD_trainaug", "VOC2012/COB_SBD_val", "VOC2012/Center_points", "coco2017/COB-COCO", "trash"):
                os.makedirs(os.path.join("data", d))
            write_voc_mat(voc_masks, VOC_ID, voc_points)
            write_voc_mat(coco_masks, COCO_ID, coco_points)
            write_voc_mat(voc_masks, NOPOINTS_ID, [])
            coco_key = 42
            FakeCOCO.table[coco_key] = ("000000000042.jpg", [])
            scipy.io.savemat(os.path.join("data", "coco2017", "COB-COCO", "000000000042.mat"), {"maskmat": coco_masks})

            gen_voc = importlib.import_module("generate_7_7_voc")
            gen_voc.mask_size = S                                # set under __main__ in the reference
            gen_voc.generate_pkl_voc2012([VOC_ID], 0)
            voc_out = pickle.load(open(os.path.join("data", "trash", "voc_0.pkl"), "rb"))
            gen_coco = importlib.import_module("generate_7_7_coco")
            gen_coco.mask_size = S
            gen_coco.cocoGt = FakeCOCO()                         # a module global of the reference's __main__
            gen_coco.generate_pkl_coco2017([coco_key], 0)
            coco_out = pickle.load(open(os.path.join("data", "trash", "coco_0.pkl"), "rb"))
            assign = importlib.import_module("point_level_label_assign")
            assign.assign_voc2012([VOC_ID, COCO_ID, NOPOINTS_ID], 0, "voc", FakeCOCO())
            mats = pickle.load(open(os.path.join("data", "trash", assign.useless_file.format(0)), "rb"))
        finally:
            os.chdir(cwd)
    assert mats["indexes"] == [VOC_ID, COCO_ID, NOPOINTS_ID]
    voc_boxes, voc_small = voc_out["boxes"][0], voc_out["masks"][0]
    coco_boxes, coco_small = coco_out["boxes"][0], coco_out["masks"][0]
    assert voc_boxes.dtype == np.uint16 and voc_small.dtype == bool and mats["mat"][0].dtype == np.float32
    check_situations(voc_masks, voc_points, first, mats["mat"][0])
    wv = set((voc_boxes[:, 2] - voc_boxes[:, 0]).tolist()) | set((voc_boxes[:, 3] - voc_boxes[:, 1]).tolist())
    assert {1, 2, 4, 8, 16, 32, 64, 128, 3, 5, 7} <= wv
    assert np.any(np.all(coco_boxes == (0, 0, 1400, 40), axis=1))
    save_npz(os.path.join(HERE, "proposal_prep_voc.npz"), record(voc_masks, voc_points, voc_boxes, voc_small, mats["mat"][0]))
    save_npz(os.path.join(HERE, "proposal_prep_coco.npz"), record(coco_masks, coco_points, coco_boxes, coco_small, mats["mat"][1]))
    save_npz(os.path.join(HERE, "proposal_prep_nopoints.npz"), record(voc_masks, [], voc_boxes, voc_small, mats["mat"][2]))
    for name in ("voc", "coco", "nopoints"):
        path = os.path.join(HERE, "proposal_prep_%s.npz" % name)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
