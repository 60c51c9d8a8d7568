"""lib/datasets/dis_eval.py of the reference on the device: CorLoc of one class from a results file and the XML
annotations - sum(tp) / (images with a ground truth of the class), tp where the best overlap exceeds ovthresh.  Same name,
arguments and return value; cim_amd.box_eval does the work (mode 1 of cim_voc_match)."""
import numpy as np

from .voc_eval import class_evaluator, load_annotations, parse_rec  # noqa: F401


def dis_eval(detpath, annopath, imagesetfile, classname, cachedir, ovthresh=0.5):
    ev = class_evaluator(detpath, annopath, imagesetfile, classname, cachedir, ovthresh, False)
    if ev is None:                                                       # no non-zero box: nothing is a true positive
        _, recs = load_annotations(annopath, imagesetfile, cachedir)
        nimgs = float(sum(1 for objs in recs.values() if any(o["name"] == classname for o in objs)))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float64(0.0) / np.float64(nimgs)
    return ev.corloc()[0][classname]
