"""References for the cases of loss_cases.py, computed on the CPU once per process and shared by tests/test_loss_cases_cpu.py
and tests/test_gpu_losses_edges.py: values from oracle/losses.py, gradients from the ATen formulation of
cim_amd/modeling/heads.py under autograd - float64, or float32 for the cases that saturate the clamps (1 - 1e-6 is no fp32
number: the fp64 clamp gates other elements than the fp32 one)."""
import os
import sys

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)

from loss_cases import UP4, UP6, loss_case  # noqa: E402
from oracle import losses as oracle_losses  # noqa: E402

_CACHE = {}


def bag_first_max(fused, pseudo_labels, padded, loss_weight):
    """loss_weight_bag_loss (heads.py) with both arg-max vectors taken from np.argmax - the FIRST maximum, the rule
    cim_amd/csrc/losses.hip documents and oracle/losses.py uses; torch.max(dim=0) promises no particular index among equal
    maxima.  The values are gathered at those rows, so autograd sends the gradient there."""
    member = (pseudo_labels != 0).to(fused.dtype)
    masked = fused * member
    cols = torch.arange(fused.shape[1])
    fi = torch.from_numpy(np.argmax(masked.detach().numpy(), axis=0))
    ui = torch.from_numpy(np.argmax(fused.detach().numpy(), axis=0))
    labels = padded.reshape(-1)
    seen = labels == 1
    agg = (masked[fi, cols] * labels + fused[ui, cols] * (1 - labels)).clamp(1e-6, 1 - 1e-6)
    weight = torch.where(seen, loss_weight[torch.where(seen, fi, ui)], torch.ones_like(agg))
    return (-(labels * torch.log(agg) + (1 - labels) * torch.log(1 - agg)) * weight).mean()


def oracle_values(name):
    """(bag, pcl, cls, iou) of oracle/losses.py in the case's reference precision, as Python floats."""
    key = ("oracle", name)
    if key not in _CACHE:
        case = loss_case(name)
        dt = np.float32 if case["fp32"] else np.float64
        bag = oracle_losses.mil_bag_loss(case["pc"], case["pd"], case["labels"], dt)
        cls = iou = dt(0)
        for i in range(case["R"]):
            if case["valid"][i]:
                y, t16, w = case["pseudo"][i]
                c, io, b = oracle_losses.cls_iou_loss(case["rc"][i], case["ri"][i], y, t16, dt(case["scales"][i]) * w.astype(dt),
                                                      case["labels"], dt)
                bag, cls, iou = bag + b, cls + c, iou + io
        pcl = oracle_losses.pcl_loss(case["pc"], case["mat"], dt)
        _CACHE[key] = tuple(float(x) for x in (bag, pcl, cls, iou))
    return _CACHE[key]


class AtenTerms:
    """The ATen formulation on CPU leaves of `dtype`: leaves = [pc, pd, rc.., ri..]; mil, pcl and the per-layer cls / iou / bag
    terms (None for a layer that is not valid)."""

    def __init__(self, case, dtype):
        from cim_amd.modeling import heads
        leaf = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
        R = case["R"]
        self.pc, self.pd = leaf(case["pc"]), leaf(case["pd"])
        self.rc, self.ri = [leaf(a) for a in case["rc"]], [leaf(a) for a in case["ri"]]
        self.leaves = [self.pc, self.pd] + self.rc + self.ri
        labels = torch.from_numpy(case["labels"]).to(dtype)
        self.mil = heads.mil_bag_loss(self.pc, self.pd, labels)
        self.pcl = heads.PCL_loss(self.pc, torch.from_numpy(case["mat"]).to(dtype), labels)
        self.cls, self.iou, self.bag = [None] * R, [None] * R, [None] * R
        for i in range(R):
            if not case["valid"][i]:
                continue
            y, t16, w = (torch.from_numpy(a) for a in case["pseudo"][i])
            w = case["scales"][i] * w.to(dtype)
            self.cls[i], self.iou[i], self.bag[i] = heads.cls_iou_loss(self.rc[i], self.ri[i], y, t16, w, labels)
            if case["first_max"]:
                self.bag[i] = bag_first_max(heads._clamp(self.rc[i]) * heads._clamp(self.ri[i]), y, heads._pad_bg(labels), w)
        some = lambda xs: [x for x in xs if x is not None]
        zero = torch.zeros((), dtype=dtype)
        self.four = (sum(some(self.bag), self.mil), self.pcl, sum(some(self.cls), zero), sum(some(self.iou), zero))

    def grad(self, term, leaf):
        if term is None or not term.requires_grad:
            return np.zeros(tuple(leaf.shape))
        g, = torch.autograd.grad(term, leaf, retain_graph=True, allow_unused=True)
        return np.zeros(tuple(leaf.shape)) if g is None else g.numpy().astype(np.float64)

    def components(self):
        """The 3 + 4R gradient components in the order of the kernel's planes."""
        out = [self.grad(self.mil, self.pc), self.grad(self.pcl, self.pc), self.grad(self.mil, self.pd)]
        for i in range(len(self.rc)):
            out += [self.grad(self.cls[i], self.rc[i]), self.grad(self.bag[i], self.rc[i]),
                    self.grad(self.iou[i], self.ri[i]), self.grad(self.bag[i], self.ri[i])]
        return out

    def weighted_grads(self, up):
        """d(weighted sum)/d leaf for up = weights of (bag, pcl, cls, iou[, 3 iou, total]), total = bag + pcl + cls + 3 iou."""
        bag, pcl, cls, iou = self.four
        total = up[0] * bag + up[1] * pcl + up[2] * cls + up[3] * iou
        if len(up) == 6:
            total = total + up[4] * (3 * iou) + up[5] * (bag + pcl + cls + 3 * iou)
        gs = torch.autograd.grad(total, self.leaves, retain_graph=True, allow_unused=True)
        return [np.zeros(tuple(x.shape)) if g is None else g.numpy().astype(np.float64) for x, g in zip(self.leaves, gs)]


def aten(name, dtype=None):
    """AtenTerms of the named case (in its reference precision unless dtype is given), built once."""
    case = loss_case(name)
    dtype = dtype or (torch.float32 if case["fp32"] else torch.float64)
    key = ("aten", name, dtype)
    if key not in _CACHE:
        _CACHE[key] = AtenTerms(case, dtype)
    return _CACHE[key]


def aten_values(name, dtype=None):
    return tuple(float(x.detach()) for x in aten(name, dtype).four)


def reference_grads(name, up=UP4):
    key = ("grads", name, tuple(up))
    if key not in _CACHE:
        _CACHE[key] = aten(name).weighted_grads(up)
    return _CACHE[key]


__all__ = ["UP4", "UP6", "AtenTerms", "aten", "aten_values", "bag_first_max", "oracle_values", "reference_grads"]
