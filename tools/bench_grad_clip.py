#!/usr/bin/env python3
"""Gradient clipping alone on the trainable parameters of the resnet50_voc model (cfg2) with random gradients, on one device:
    (a) norm            cim_amd.optim.GradClipper.norm()                        reads 4 B per element
    (b) clip_coef_1     GradClipper.clip(max_norm far above the norm)           reads 4 B per element, the scale launch returns at once
    (c) clip_scaling    GradClipper.clip(max_norm below the norm)               4 B read + 4 B read + 4 B written per element
    (d) torch_clip      cim_amd.utils.net._clip_gradient_torch, the reference's arithmetic on the same tensors: one ATen norm
                        and one mul_ per tensor, and the `.item()` in between
HIP-event ms per call.  The candidates are interleaved (one call of each per round, the same gradient tensors), --warmup rounds
first; every call starts on a device that has finished the previous one (`.item()` makes (d) wait anyway).  (c) and (d) get a
threshold 1 % below the CURRENT norm each time, so every round really scales.  A second table for (a) - (c): --chain calls
enqueued back to back over the chain length - the host's table refresh of call k + 1 runs under the launches of call k, so this
is the launches' own time, the figure the share of the 6.3 TB/s streaming rate is computed from.  About 1 GB of gradients, far
beyond the 256 MiB last-level cache.  One JSON line.

    python tools/bench_grad_clip.py [--rounds 5] [--warmup 3] [--chain 8]"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from cim_amd import optim  # noqa: E402
from cim_amd.core.config import cfg  # noqa: E402
from cim_amd.core.presets import apply_preset  # noqa: E402
from cim_amd.modeling.model_builder import Generalized_RCNN  # noqa: E402
from cim_amd.utils import net  # noqa: E402

HBM_TB_PER_S = 6.3      # achievable streaming rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    apply_preset("resnet50_voc")
    torch.manual_seed(cfg.RNG_SEED)
    model = Generalized_RCNN()
    bench.init_for_synthetic(model)
    model = model.to(dev)
    params = [p for g in optim.param_groups(model) for p in g["params"]]
    n = sum(p.numel() for p in params)
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
    grads = [p.grad for p in params]
    clipper = optim.GradClipper(params)
    state = {"norm": float(clipper.norm()[0])}          # (between timed calls only: the thresholds of (c) and (d) follow the norm)

    def shrink():
        state["norm"] *= 0.99
        return state["norm"]

    cands = {"norm": (lambda: clipper.norm(), 4), "clip_coef_1": (lambda: clipper.clip(1e30), 4),
             "clip_scaling": (lambda: clipper.clip(shrink()), 12), "torch_clip": (lambda: net._clip_gradient_torch(grads, shrink()), None)}
    times = {k: [] for k in cands}
    for r in range(args.warmup + args.rounds):
        for name, (fn, _) in cands.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b))
    chained = {k: [] for k in cands if k != "torch_clip"}
    for r in range(args.rounds):
        for name in chained:
            fn = cands[name][0]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()                        # (the chain starts behind a running call, not on an idle device)
            a.record()
            for _ in range(args.chain):
                fn()
            b.record()
            b.synchronize()
            chained[name].append(a.elapsed_time(b) / args.chain)
    out = clipper.norm().tolist()
    rec = dict(config="resnet50_voc", tensors=len(params), elements=n, rounds=args.rounds, warmup=args.warmup, chain=args.chain,
               device=torch.cuda.get_device_name(0), torch=torch.__version__, final_norm=out[0], tracked_norm=state["norm"])
    for name, (_, nbytes) in cands.items():
        rec[name] = dict(call_ms=[round(t, 4) for t in times[name]], call_min_max_ms=[round(min(times[name]), 4), round(max(times[name]), 4)])
        if name in chained:
            best = min(chained[name])
            rec[name].update(bytes_per_element=nbytes, chained_ms=[round(t, 4) for t in chained[name]],
                             chained_min_max_ms=[round(best, 4), round(max(chained[name]), 4)],
                             tb_per_s=round(n * nbytes / best / 1e9, 3), share_of_hbm_rate=round(n * nbytes / best / 1e9 / HBM_TB_PER_S, 3))
    fastest_torch = min(times["torch_clip"])
    rec["slowest_over_fastest_torch"] = {k: round(max(times[k]) / fastest_torch, 4) for k in chained}
    rec["every_round_faster_than_torch"] = all(max(times[k]) < fastest_torch for k in chained)
    print(json.dumps(rec), flush=True)
    if not rec["every_round_faster_than_torch"]:
        sys.exit("a GradClipper call was slower than the fastest torch clip")


if __name__ == "__main__":
    main()
