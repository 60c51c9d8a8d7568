#!/usr/bin/env python3
"""The trainable ResNet stem on the device (ops.conv7x7_bn_act_train, csrc/conv7x7_dw.hip): HIP-event ms, warm,
median of --repeats, candidates interleaved in one process on one device.

  1. The 7 x 7 weight gradient alone (cim_conv7x7_dw_f32, both launches) at the PRM workload (B = 16, 448 x 448, stride 2) and the
     detector's (B = 1, 800 x 1200, stride 2), beside ATen's torch.nn.grad.conv2d_weight on the same operands - printed, NOT
     credited - and a floor from the shapes: the operands read once at the HBM rate, or the product's FLOPs at the fp32 matrix
     rate, whichever is larger.
  2. The whole PRM training step (prm_train.loss, backward, cim_amd.optim.SGD; 448 x 448, B = 16, full width) after
     prm_train.unfreeze (every layer trains) and after prm_train.freeze (stem and layer1 frozen).

    python tools/bench_stem_train.py [--repeats 20] [--no-step] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cim_amd import _lib, prm, prm_train  # noqa: E402
from cim_amd.optim import SGD  # noqa: E402

HBM_BYTES_PER_S = 6.3e12          # achievable HBM3E rate of the MI355X (8 TB/s spec)
FP32_MATRIX_FLOPS = 155e12        # v_mfma_f32_*_f32: 64 FLOP per clock and SIMD
WORKLOADS = {"prm_B16_448x448_s2": (16, 3, 64, 448, 448, 2), "detector_B1_800x1200_s2": (1, 3, 64, 800, 1200, 2)}


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


def weight_gradient(shape, repeats):
    dev = torch.device("cuda:0")
    b, cin, cout, h, w, s = shape
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    g = torch.Generator().manual_seed(b)
    x = torch.randn(b, cin, h, w, generator=g).to(dev)
    dconv = torch.randn(b, cout, ho, wo, generator=g).to(dev)
    ws = torch.empty(_lib.call("cim_conv7x7_dw_workspace", *shape) // 4, dtype=torch.float32, device=dev)
    dw = torch.empty(cout, cin, 7, 7, device=dev)

    def hip():
        _lib.call("cim_conv7x7_dw_f32", dconv.data_ptr(), x.data_ptr(), dw.data_ptr(), *shape, ws.data_ptr(), _lib.stream_ptr())

    ref = []

    def aten():
        ref[:] = [torch.nn.grad.conv2d_weight(x, (cout, cin, 7, 7), dconv, stride=s, padding=3)]

    ms = interleaved_ms({"hip_conv7x7_dw": hip, "aten_conv2d_weight": aten}, repeats)
    rel = float((dw - ref[0]).norm() / ref[0].norm())
    operand_bytes = 4 * (dconv.numel() + x.numel())
    flops = 2 * cout * cin * 49 * b * ho * wo
    floor_ms = max(operand_bytes / HBM_BYTES_PER_S, flops / FP32_MATRIX_FLOPS) * 1e3
    return {"shape_B_cin_cout_H_W_stride": list(shape), "splits": _lib.load().cim_conv7x7_dw_splits(*shape), "ms_median_min_max": ms,
            "operand_bytes": operand_bytes, "workspace_bytes": ws.numel() * 4, "flops": flops,
            "floor_ms": {"bytes_at_hbm_rate": round(operand_bytes / HBM_BYTES_PER_S * 1e3, 4),
                         "flops_at_fp32_matrix_rate": round(flops / FP32_MATRIX_FLOPS * 1e3, 4)},
            "fraction_of_floor": round(floor_ms / ms["hip_conv7x7_dw"][0], 3), "hip_vs_aten_rel_fro": rel}


def training_steps(repeats):
    dev = torch.device("cuda:0")
    target = (torch.rand(16, 20, device=dev) < 0.2).float()
    x = torch.randn(16, 3, prm.INPUT_SIZE, prm.INPUT_SIZE, device=dev)
    steps = {}
    for name, prepare in (("unfreeze", prm_train.unfreeze), ("freeze", prm_train.freeze)):
        torch.manual_seed(0)
        model = prepare(prm.PeakResponseMapping(prm.fc_resnet50(20))).to(dev)
        opt = SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4, momentum=0.9, weight_decay=1e-4)

        def step(model=model, opt=opt):
            opt.zero_grad()
            prm_train.loss(model, x, target).backward()
            opt.step()

        steps[name] = step
    ms = interleaved_ms(steps, repeats)
    return {k: {"ms_median_min_max": v, "images_per_second": round(16 / v[0] * 1e3, 1)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="skip the whole training steps")
    ap.add_argument("--out", default=None, help="also write the record to this file")
    args = ap.parse_args()
    rec = dict(bench="stem_train", repeats=args.repeats, device=torch.cuda.get_device_name(0), method="HIP events, warm, median, interleaved in one process")
    for name, shape in WORKLOADS.items():
        rec[name] = weight_gradient(shape, args.repeats)
    rec["training_step_448_B16"] = "not measured" if args.no_step else training_steps(args.repeats)
    rec["note"] = "shared pool: neighbours move these numbers by several per cent; ATen is printed, not credited"
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
