"""lib/datasets/voc_eval.py of the reference on the device: the PASCAL VOC devkit's per-class AP from a results file and
the XML annotations.  Same name, arguments and return values; the matching, the sort, precision / recall and the AP run in
cim_amd.box_eval (csrc/box_eval.hip).  After cim_amd.install_as_lib() the reference's
voc_dataset_evaluator imports this module as datasets.voc_eval.

Differences, all stated in DESIGN.md 4.14: equal confidences are visited grouped by image (images in order of their first
line, lines in file order: the file's order when it is image-major, as the reference writes it; the reference's unstable
argsort leaves them undefined); the annotation cache in `cachedir` is this module's own file (<image set>_annots_cim.pkl).
"""
import logging
import os
import pickle
import xml.etree.ElementTree as ET

import numpy as np

from .. import box_eval

logger = logging.getLogger(__name__)


def parse_rec(filename):
    """The objects of one PASCAL VOC XML file: [{'name', 'difficult', 'bbox': [xmin, ymin, xmax, ymax]}] in file order."""
    objects = []
    for obj in ET.parse(filename).getroot().iter("object"):
        box = obj.find("bndbox")
        difficult = obj.find("difficult")
        objects.append({"name": obj.find("name").text,
                        "difficult": int(difficult.text) if difficult is not None else 0,
                        "bbox": [int(box.find(tag).text) for tag in ("xmin", "ymin", "xmax", "ymax")]})
    return objects


def load_annotations(annopath, imagesetfile, cachedir):
    """-> (image names of the set, {name: parse_rec(...)}), read once per (cachedir, image set)."""
    with open(imagesetfile) as f:
        imagenames = [line.strip() for line in f if line.strip()]
    cachefile = None
    if cachedir is not None:
        os.makedirs(cachedir, exist_ok=True)
        cachefile = os.path.join(cachedir, os.path.splitext(os.path.basename(imagesetfile))[0] + "_annots_cim.pkl")
        if os.path.isfile(cachefile):
            with open(cachefile, "rb") as f:
                recs = pickle.load(f)
            if set(recs) == set(imagenames):
                return imagenames, recs
    recs = {name: parse_rec(annopath.format(name)) for name in imagenames}
    if cachefile is not None:
        logger.info("Saving cached annotations to %s", cachefile)
        with open(cachefile, "wb") as f:
            pickle.dump(recs, f, pickle.HIGHEST_PROTOCOL)
    return imagenames, recs


def read_detections(detfile):
    """'<image> <confidence> <x1> <y1> <x2> <y2>' lines -> (image names, confidences f64, boxes f64 [n, 4])."""
    ids, conf, boxes = [], [], []
    with open(detfile) as f:
        for line in f:
            parts = line.strip().split(" ")
            if len(parts) < 6:
                continue
            ids.append(parts[0])
            conf.append(float(parts[1]))
            boxes.append([float(z) for z in parts[2:6]])
    return ids, np.asarray(conf, np.float64), np.asarray(boxes, np.float64).reshape(-1, 4)


def class_evaluator(detpath, annopath, imagesetfile, classname, cachedir, ovthresh, use_07_metric):
    """One class's files as a one-class VocBoxEvaluator; images in the order of their first line in the results file (for an
    image-major file the stable tie rule then is the file's order), the images without detection after them.  None when no box is non-zero
    (the reference's early return)."""
    imagenames, recs = load_annotations(annopath, imagesetfile, cachedir)
    ids, conf, boxes = read_detections(detpath.format(classname))
    if not boxes.any():
        return None
    ev = box_eval.VocBoxEvaluator([classname], ovthresh=ovthresh, use_07_metric=use_07_metric, text_round_trip=False)
    rows = {}
    for j, name in enumerate(ids):
        rows.setdefault(name, []).append(j)
    for name in list(rows) + [n for n in imagenames if n not in rows]:
        objs = [o for o in recs[name] if o["name"] == classname]
        j = rows.get(name, [])
        ev.add_parsed(name, [o["bbox"] for o in objs], [0] * len(objs), [o["difficult"] for o in objs],
                      [(0, boxes[j], conf[j])] if j else [])
    return ev


def voc_eval(detpath, annopath, imagesetfile, classname, cachedir, ovthresh=0.5, use_07_metric=False):
    """rec, prec, ap = voc_eval(detpath, annopath, imagesetfile, classname, cachedir, [ovthresh], [use_07_metric]):
    detpath.format(classname) is the results file, annopath.format(imagename) an image's XML, imagesetfile lists the images."""
    ev = class_evaluator(detpath, annopath, imagesetfile, classname, cachedir, ovthresh, use_07_metric)
    if ev is None:
        logger.info("%s is None", classname)
        return 0, 0, 0
    rec, prec, ap = ev.evaluate()[0][classname]
    return rec, prec, ap
