#!/usr/bin/env python3
"""The optimizer step alone on the trainable parameters of the resnet50_voc model (cfg2) with synthetic gradients, on one
device: cim_amd.optim.SGD, cim_amd.optim.Adam, torch.optim.Adam(foreach=True) and - where this torch build accepts it -
torch.optim.Adam(fused=True).  HIP-event ms per step; the candidates are interleaved (one step of each per round, the same
parameters and gradients), median / min / max of --repeats rounds after --warmup.  Bytes are what the rule has to move:
20 B per parameter for SGD with momentum (p, g, buf read; p, buf written), 28 B for Adam (p, g, m, v read; p, m, v written);
about 1 GB of parameters, far beyond the 256 MiB last-level cache, so no round re-reads warm lines.  Two figures per
candidate: one step() from an idle device (the host's table refresh in front of the launch included) and --chain steps
enqueued back to back over the chain length (the launch's own time; the bandwidth to compare kernels by).  One JSON line.

    python tools/bench_optim.py [--repeats 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from cim_amd import optim  # noqa: E402
from cim_amd.core.config import cfg  # noqa: E402
from cim_amd.core.presets import apply_preset  # noqa: E402
from cim_amd.modeling.model_builder import Generalized_RCNN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=8, help="steps enqueued back to back per timing of the second table")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    apply_preset("resnet50_voc")
    torch.manual_seed(cfg.RNG_SEED)
    model = Generalized_RCNN()
    bench.init_for_synthetic(model)
    model = model.to(dev)
    groups = lambda: [dict(g) for g in optim.param_groups(model)]
    params = [p for g in groups() for p in g["params"]]
    n = sum(p.numel() for p in params)
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
    lr = 1e-6           # (small: 20 + 3 steps of four optimizers on the same weights leave them where they were)
    cands = {"cim_sgd": (optim.SGD(groups(), lr=lr, momentum=0.9), 20), "cim_adam": (optim.Adam(groups(), lr=lr), 28),
             "torch_adam_foreach": (torch.optim.Adam(groups(), lr=lr, foreach=True), 28)}
    skipped = {}
    try:
        fused = torch.optim.Adam(groups(), lr=lr, fused=True)
        fused.step()
        torch.cuda.synchronize()
        cands["torch_adam_fused"] = (fused, 28)
    except Exception as e:           # this torch build has no fused Adam for the device: reported, not hidden
        skipped["torch_adam_fused"] = "%s: %s" % (type(e).__name__, str(e)[:200])
    for g in [g for opt, _ in cands.values() for g in opt.param_groups]:
        g["lr"] = lr * (2 if g["weight_decay"] == 0 else 1)
    times = {k: [] for k in cands}
    for r in range(args.warmup + args.repeats):
        for name, (opt, _) in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opt.step()
            b.record()
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b))
    # the same steps enqueued back to back (--chain per event pair): the host's table refresh of step k + 1 runs under the kernel of
    # step k, so the interval over the chain length is the launch's own time on the device
    chained = {k: [] for k in cands}
    for r in range(args.repeats):
        for name, (opt, _) in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            opt.step()                  # (the chain starts behind a running step, not on an idle device)
            a.record()
            for _ in range(args.chain):
                opt.step()
            b.record()
            b.synchronize()
            chained[name].append(a.elapsed_time(b) / args.chain)
    rec = dict(config="resnet50_voc", tensors=len(params), parameters=n, repeats=args.repeats, warmup=args.warmup, chain=args.chain,
               device=torch.cuda.get_device_name(0), torch=torch.__version__, skipped=skipped)
    for name, (_, nbytes) in cands.items():
        med = float(np.median(times[name]))
        rec[name] = dict(ms=round(med, 4), min_max_ms=[round(min(times[name]), 4), round(max(times[name]), 4)],
                         bytes_per_parameter=nbytes, tb_per_s=round(n * nbytes / med / 1e9, 3))
        ch = float(np.median(chained[name]))
        rec[name].update(chained_ms=round(ch, 4), chained_min_max_ms=[round(min(chained[name]), 4), round(max(chained[name]), 4)],
                         chained_tb_per_s=round(n * nbytes / ch / 1e9, 3))
    others = [rec[k]["ms"] for k in rec if k.startswith("torch_adam")]
    rec["cim_adam_over_fastest_torch_adam"] = round(rec["cim_adam"]["ms"] / min(others), 4)
    rec["cim_adam_over_fastest_torch_adam_chained"] = round(rec["cim_adam"]["chained_ms"] / min(rec[k]["chained_ms"] for k in rec if k.startswith("torch_adam")), 4)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
