#!/usr/bin/env python3
"""Batch-statistics BatchNorm on the device (ops.bn_act_train, csrc/bn_train.hip): forward + backward of the
operator on the BatchNorm shapes of ResNet-50 at 16 x 448 x 448 (the PRM training batch), beside the ATen formulation the
frozen-statistics operator falls back to when it is allowed to (`bn_act` on a module in train() mode under fallback.allowed:
F.batch_norm(training=True) (+ residual) + ReLU through autograd).  HIP-event ms, warm, median of --repeats, the two candidates
interleaved in one process on one device.  ATen is printed, NOT credited; no threshold is applied.

Bytes: what the launches must move per element - statistics 4, normalisation 8 (+ 4 with a residual), backward sums 12, dx 16
(+ 4 for dres) - over the measured time; the second read of the statistics launch is counted as cache traffic, not here.

    python tools/bench_bn_train.py [--repeats 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cim_amd import _lib  # noqa: E402
from cim_amd.ops import bn_act, bn_act_train, fallback  # noqa: E402

HBM_BYTES_PER_S = 6.3e12          # achievable HBM3E rate of the MI355X (8 TB/s spec)
BATCH = 16
# (name, channels, side, residual): every distinct BatchNorm of torchvision's ResNet-50 (stride on the 3 x 3) at 448 x 448
SHAPES = [
    ("stem.bn1", 64, 224, False),
    ("layer1.bn1/bn2", 64, 112, False),
    ("layer1.bn3", 256, 112, True),
    ("layer2.0.bn1", 128, 112, False),
    ("layer2.bn1/bn2", 128, 56, False),
    ("layer2.bn3", 512, 56, True),
    ("layer3.0.bn1", 256, 56, False),
    ("layer3.bn1/bn2", 256, 28, False),
    ("layer3.bn3", 1024, 28, True),
    ("layer4.0.bn1", 512, 28, False),
    ("layer4.bn1/bn2", 512, 14, False),
    ("layer4.bn3", 2048, 14, True),
]


def interleaved_ms(fns, repeats):
    """name -> [median, min, max] ms, the candidates taking turns inside every repeat (neighbours on the device hit all alike)."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)] for k, v in times.items()}


def one_shape(c, side, with_res, repeats):
    dev = torch.device("cuda:0")
    shape = (BATCH, c, side, side)
    g = torch.Generator().manual_seed(c + side)
    x = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
    res = torch.randn(shape, generator=g).to(dev).requires_grad_(True) if with_res else None
    dy = torch.randn(shape, generator=g).to(dev)
    bn_hip = torch.nn.BatchNorm2d(c).to(dev)
    bn_aten = torch.nn.BatchNorm2d(c).to(dev).train()
    grads = {}

    def run(op, bn, key):
        for t in (x, res, bn.weight, bn.bias):
            if t is not None:
                t.grad = None
        op(x, bn, residual=res, relu=True).backward(dy)
        grads[key] = x.grad

    def hip():
        run(bn_act_train, bn_hip, "hip")

    def aten():
        with fallback.allowed("bn_act"):
            run(bn_act, bn_aten, "aten")

    ms = interleaved_ms({"hip_bn_act_train": hip, "aten_batch_norm_relu": aten}, repeats)
    per_element = (4 + 8 + 12 + 16) + (8 if with_res else 0)
    nbytes = per_element * x.numel()
    rel = float((grads["hip"] - grads["aten"]).norm() / grads["aten"].norm())
    return {"shape_N_C_H_W": list(shape), "residual": with_res, "chunks": _lib.load().cim_bn_train_chunks(BATCH, c, side * side),
            "ms_fwd_bwd_median_min_max": ms, "bytes": nbytes, "bytes_per_element": per_element,
            "achieved_bytes_per_s": {k: round(nbytes / (v[0] * 1e-3), 1) for k, v in ms.items()},
            "fraction_of_hbm_rate": round(nbytes / (ms["hip_bn_act_train"][0] * 1e-3) / HBM_BYTES_PER_S, 3),
            "hip_over_aten_time": round(ms["hip_bn_act_train"][0] / ms["aten_batch_norm_relu"][0], 3), "dx_hip_vs_aten_rel_fro": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the record to this file")
    args = ap.parse_args()
    rec = dict(bench="bn_train", repeats=args.repeats, device=torch.cuda.get_device_name(0), batch=BATCH,
               method="HIP events, warm, median, interleaved in one process; forward + backward of one layer")
    fallback.reset()
    rec["shapes"] = {name: one_shape(c, side, with_res, args.repeats) for name, c, side, with_res in SHAPES}
    rec["slower_than_aten"] = [k for k, v in rec["shapes"].items() if v["hip_over_aten_time"] > 1.0]
    rec["note"] = "shared pool: neighbours move these numbers by several per cent; ATen is printed, not credited"
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
