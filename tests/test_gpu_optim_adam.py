"""-m gpu: cim_amd.optim.Adam (csrc/adam.hip) - the update rule against torch.optim.Adam evaluated in float64, and the
machinery it shares with cim_amd.optim.SGD (version counters, matrix-mode scales, overlap_update, replaced state, step_early,
a whole training run).

The bound of every comparison with torch is derived, not chosen: X_f64 is torch.optim.Adam(foreach=False) in float64 on the CPU
from the same fp32 inputs, d_torch the max-abs deviation of torch.optim.Adam(foreach=False) in fp32 on the CPU from it, floor one
fp32 ulp of max |X_f64|; required: max |hip - X_f64| <= 4 * max(d_torch, floor) for every parameter, exp_avg and exp_avg_sq.
The factor 4 covers a different FMA contraction and order of operations (an independently written fp32 Adam stayed at 1.0 - 1.55)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()          # fail loudly if the HIP extension is missing
    return torch.device("cuda:0")


def _ratio(hip, f32, f64):
    """max |hip - f64| over max(d_torch, one fp32 ulp of max |f64|)."""
    hip, f32 = hip.detach().cpu().double(), f32.detach().double()
    d_torch = float((f32 - f64).abs().max())
    floor = float(np.spacing(np.float32(f64.abs().max())))
    return float((hip - f64).abs().max()) / max(d_torch, floor), d_torch, floor


class _Trio:
    """The same parameters under torch.optim.Adam in float64 and in fp32 on the CPU and under cim_amd.optim.Adam on the device."""

    def __init__(self, base, dev, groups, hip_params=None):
        from cim_amd.optim import Adam
        self.dev = dev
        self.p64 = [b.double().clone().requires_grad_(True) for b in base]
        self.p32 = [b.clone().requires_grad_(True) for b in base]
        self.hip = hip_params if hip_params is not None else [b.clone().to(dev).requires_grad_(True) for b in base]
        self.o64 = torch.optim.Adam(groups(self.p64), foreach=False)
        self.o32 = torch.optim.Adam(groups(self.p32), foreach=False)
        self.ohip = Adam(groups(self.hip))

    def step(self, grads):
        """grads: per parameter an fp32 CPU tensor or None."""
        for a, b, c, g in zip(self.p64, self.p32, self.hip, grads):
            a.grad, b.grad, c.grad = (None, None, None) if g is None else (g.double(), g.clone(), g.clone().to(self.dev))
        self.o64.step()
        self.o32.step()
        self.ohip.step()

    def check(self, names):
        worst = {}
        for name, a, b, c in zip(names, self.p64, self.p32, self.hip):
            if a not in self.o64.state:
                assert c not in self.ohip.state or not self.ohip.state[c]
                continue
            assert float(self.ohip.state[c]["step"]) == float(self.o64.state[a]["step"]), name       # its OWN count
            for what, x64, x32, xh in (("param", a.detach(), b, c), ("exp_avg", self.o64.state[a]["exp_avg"], self.o32.state[b]["exp_avg"], self.ohip.state[c]["exp_avg"]),
                                       ("exp_avg_sq", self.o64.state[a]["exp_avg_sq"], self.o32.state[b]["exp_avg_sq"], self.ohip.state[c]["exp_avg_sq"])):
                r, d_torch, floor = _ratio(xh, x32, x64)
                worst["%s %s" % (name, what)] = dict(ratio=round(r, 4), d_torch=d_torch, floor=floor)
        print("ADAM_PARITY " + json.dumps(worst))
        bad = {k: v for k, v in worst.items() if not v["ratio"] <= FACTOR}
        assert not bad, bad


def test_fused_adam_matches_torch_adam_in_float64(dev):
    """Seven steps on tensors of odd sizes (tails, chunk boundaries), a view at a 4-byte-aligned offset and a matrix-mode weight
    ragged against the 64 x 1024 tiles; two groups (weight decay 0.01 / lr 0.05 and none / lr 0.1); gradients alternating between
    ~1 and ~1e-4 so that sqrt(v) lags |m|; gradient elements that are exactly zero in the group without weight decay (their
    parameters must not move); an lr change in the middle; one parameter whose first gradient arrives at step 3."""
    g = torch.Generator().manual_seed(3)
    shapes = [(1000, 50), (16384,), (16385,), (7,), (3, 5, 7), (40000,), (1036, 1028)]
    names = ["%s" % (s,) for s in shapes] + ["view+4B"]
    base = [torch.randn(*s, generator=g) for s in shapes]
    storage = torch.randn(1001, generator=g)
    big = storage.clone().to(dev)
    hip_p = [b.clone().to(dev).requires_grad_(True) for b in base] + [big[1:].detach().requires_grad_(True)]
    base.append(storage[1:].clone())
    decayed = (0, 1, 2, 6)                                  # group 0: weight decay; group 1: (7,), (3, 5, 7), (40000,), the view
    groups = lambda ps: [dict(params=[ps[i] for i in decayed], lr=0.05, weight_decay=0.01),
                         dict(params=[ps[i] for i in range(len(ps)) if i not in decayed], lr=0.1, weight_decay=0.0)]
    trio = _Trio(base, dev, groups, hip_p)
    assert hip_p[7].data_ptr() % 16 == 4
    late, frozen = 2, 5                                     # (16385,): first gradient at step 3; (40000,): every third element's gradient is 0
    start = hip_p[frozen].detach().clone()
    for step in range(7):
        scale = 1.0 if step % 2 == 0 else 1e-4
        grads = [torch.randn(b.shape, generator=g) * scale for b in base]
        grads[frozen][::3] = 0.0
        if step < 2:
            grads[late] = None
        if step == 4:
            for opt in (trio.o64, trio.o32, trio.ohip):
                for grp in opt.param_groups:
                    grp["lr"] *= 0.1
        before = [(p._version, trio.ohip.state[p]["exp_avg"]._version, trio.ohip.state[p]["exp_avg_sq"]._version) if trio.ohip.state.get(p) else None
                  for p in hip_p]
        trio.step(grads)
        for i, (p, b) in enumerate(zip(hip_p, before)):    # the raw-pointer update is visible to the version counters
            if b is not None:
                st = trio.ohip.state[p]
                assert p._version > b[0] and st["exp_avg"]._version > b[1] and st["exp_avg_sq"]._version > b[2], (step, i)
    assert float(trio.ohip.state[hip_p[late]]["step"]) == 5.0 and float(trio.ohip.state[hip_p[0]]["step"]) == 7.0
    st = trio.ohip.state[hip_p[0]]                          # laid out as torch.optim.Adam lays it out
    ref = trio.o32.state[trio.p32[0]]
    assert list(st.keys()) == list(ref.keys()) and st["step"].dtype == ref["step"].dtype and st["step"].device == ref["step"].device
    assert torch.equal(hip_p[frozen].detach()[::3], start[::3])                 # zero gradient, no decay: not a bit moves
    assert not torch.equal(hip_p[frozen].detach()[1::3], start[1::3])
    from cim_amd.ops import gemm
    assert gemm._registered_scales(hip_p[6], 1036, 1028) is not None          # the big weight did take matrix mode
    trio.check(names)


def test_fused_adam_matrix_mode_hands_scales_to_the_contractions(dev):
    """Weights of >= 2^20 elements take the kernel's matrix mode: the row / column max |w_new| it registers are exactly what
    cim_amax_rowcol computes - valid for this version of the weight only."""
    from cim_amd.optim import Adam
    from cim_amd.ops import gemm as G
    from experiments import engines as X
    g = torch.Generator().manual_seed(5)
    rows, cols = 1036, 1028
    hp = [torch.randn(rows, cols, generator=g).to(dev).requires_grad_(True), torch.randn(77, generator=g).to(dev).requires_grad_(True)]
    hip = Adam(hp, lr=0.01, weight_decay=0.01)
    for _ in range(3):
        for b in hp:
            b.grad = torch.randn(b.shape, generator=g).to(dev)
        hip.step()
    reg = G._registered_scales(hp[0], rows, cols)
    assert reg is not None
    ra, ca = X.amax(hp[0].detach(), rows, cols, cols, True, True)
    assert torch.equal(reg[0], ra) and torch.equal(reg[1], ca)
    x = torch.randn(50, cols, generator=g).to(dev)
    y_reg = X.linear(x, hp[0])                               # uses the registered scales
    with torch.no_grad():
        hp[0].mul_(1.0)                                      # any other in-place change invalidates them
    assert G._registered_scales(hp[0], rows, cols) is None
    assert torch.equal(y_reg, X.linear(x, hp[0]))


def test_fused_adam_overlapped_update_is_the_same_update(dev):
    """overlap_update: the big weight (exactly TRAIL_MIN elements, matrix mode) is updated by a walking launch on the package's
    side stream; weights, both moments and the registered scales equal the one-stream update bit for bit, for 256, 7 and 0
    (= one per tile) workgroups; the pending update is registered by step() and waited for by state_dict()."""
    from cim_amd.optim import Adam, sgd as sgd_mod
    from cim_amd.ops import gemm
    g = torch.Generator().manual_seed(5)
    rows, cols = 4096, sgd_mod.TRAIL_MIN // 4096
    base = [torch.randn(rows, cols, generator=g) * 0.1, torch.randn(1000, 50, generator=g), torch.randn(777, generator=g)]

    def run(overlap, wgs):
        ps = [b.clone().to(dev).requires_grad_(True) for b in base]
        opt = Adam([dict(params=ps[:2], lr=0.05, weight_decay=0.01), dict(params=ps[2:], lr=0.1, weight_decay=0.0)])
        opt.overlap_update, opt.trail_workgroups = overlap, wgs
        gg = torch.Generator().manual_seed(6)
        scales = None
        for step in range(3):
            for p_ in ps:
                p_.grad = torch.randn(p_.shape, generator=gg).to(dev)
            if step == 2:
                for grp in opt.param_groups:
                    grp["lr"] *= 0.5
            opt.step()
            if overlap:
                assert gemm._PENDING_UPDATES, "the big weight's update did not go to the side stream"
            opt.zero_grad()
            scales = gemm._registered_scales(ps[0], rows, cols)
        sd = opt.state_dict()                                       # (waits for the side stream by itself)
        assert not gemm._PENDING_UPDATES
        out = [p_.detach().clone() for p_ in ps] + [sd["state"][i][k].clone() for i in range(3) for k in ("exp_avg", "exp_avg_sq")]
        torch.cuda.synchronize()
        return out + [scales[0].clone(), scales[1].clone()]

    ref = run(False, 0)
    for wgs in (256, 7, 0):
        got = run(True, wgs)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (wgs, i)


def test_fused_adam_follows_replaced_state_and_storage(dev):
    """The fast path caches raw pointers of parameters and moments.  load_state_dict() replaces the moment tensors and
    `p.data = ...` the parameter storage: the next step must use the NEW tensors, as torch.optim.Adam does."""
    g = torch.Generator().manual_seed(9)
    base = [torch.randn(300, 40, generator=g), torch.randn(1234, generator=g)]
    trio = _Trio(base, dev, lambda ps: [dict(params=ps, lr=0.01)])
    step = lambda: trio.step([torch.randn(b.shape, generator=g) for b in base])
    step()
    step()
    for opt in (trio.o64, trio.o32, trio.ohip):                 # checkpoint round trip with DIFFERENT moments
        sd = opt.state_dict()
        for st in sd["state"].values():
            st["exp_avg"] = st["exp_avg"] * 0.5 + 0.25
            st["exp_avg_sq"] = st["exp_avg_sq"] * 2.0 + 0.125
        opt.load_state_dict(sd)
    step()
    trio.check(["(300, 40) reloaded", "(1234,) reloaded"])
    for ps in (trio.p64, trio.p32, trio.hip):                   # the parameter's storage is swapped
        for p in ps:
            p.data = p.data.clone()
    step()
    trio.check(["(300, 40) swapped", "(1234,) swapped"])
    got = trio.ohip.state_dict()["state"]
    assert all(torch.equal(st[k], trio.ohip.state[p][k]) for st, p in zip(got.values(), trio.hip) for k in ("exp_avg", "exp_avg_sq"))


def test_fused_adam_refuses_a_captured_step(dev):
    """The bias corrections are host numbers: a step under stream capture raises before anything is launched or counted."""
    from cim_amd import _lib
    from cim_amd.optim import Adam
    p = torch.randn(64, device=dev).requires_grad_(True)
    p.grad = torch.randn(64, device=dev)
    opt = Adam([p], lr=0.1)
    opt.step()
    torch.cuda.synchronize()
    before = p.detach().clone()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.CimHipError):
                opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[p]["step"]) == 1.0 and torch.equal(p.detach(), before)


def test_early_adam_step_is_identical():
    """nn.DataParallel.attach_optimizer works through step_early alone: MaskFuse / heads parameters updated inside the backward
    pass on a side stream, the rest by step() - weights and both moments equal the plain step() run bit for bit."""
    import test_gpu_dp as T
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling.model_builder import Generalized_RCNN
    from cim_amd.nn import DataParallel
    from cim_amd.optim import Adam
    dev = torch.device("cuda:0")
    batches = [T._small_batch(300 + i, n=40, dev=dev) for i in range(3)]

    def run(early):
        apply_preset("vgg16_voc")
        torch.manual_seed(5)
        model = Generalized_RCNN().to(dev).train()
        dp = DataParallel(model, cpu_keywords=["im_info", "roidb"], minibatch=True)
        bias = [p for n, p in model.named_parameters() if p.requires_grad and "bias" in n]
        rest = [p for n, p in model.named_parameters() if p.requires_grad and "bias" not in n]
        opt = Adam([dict(params=rest, lr=1e-5, weight_decay=5e-4), dict(params=bias, lr=2e-5, weight_decay=0.0)])
        if early:
            assert dp.attach_optimizer(opt)
        for k in range(3):
            dp.zero_grad()
            np.random.seed(40 + k)
            T._loss(dp(**batches[k])).backward()
            if early:
                assert opt._early is not None and len(opt._early[0]) > 10, "the early update did not start inside backward"
            opt.step()
            assert opt._early is None
        torch.cuda.synchronize()
        return ({n: p.detach().clone() for n, p in model.named_parameters()},
                {n + "." + k: opt.state[p][k].clone() for n, p in model.named_parameters() if p in opt.state for k in ("exp_avg", "exp_avg_sq")})

    p0, m0 = run(False)
    p1, m1 = run(True)
    assert len(m0) == len(m1) > 20
    for n in p0:
        assert torch.equal(p1[n], p0[n]), n
    for n in m0:
        assert torch.equal(m1[n], m0[n]), n


ADAM_RUN_LR = 1e-5      # see the docstring below


def test_stream_scheduling_does_not_change_an_adam_training_run(dev, monkeypatch):
    """test_stream_scheduling_does_not_change_a_training_run with make_optimizer under SOLVER.TYPE Adam: resnet50_voc preset,
    300 proposals, 40 steps; scheduling options on and off give the same loss trajectory, final weights and exp_avg of the
    largest weight bit for bit; all gradients stay finite.
    The learning rate: 1e-5 is a per-element step of ~1e-5 (Adam normalises the gradient), 4e-4 over the 40 steps, against
    MaskFuse weights of ~1e-2.  NOT YET RUN ON HARDWARE: neither the sweep over 1e-6 / 1e-5 / 1e-4 nor this test reached a device,
    so no trajectory is recorded here; the test prints it (ADAM_RUN) and asserts loss[-1] < loss[0] as specified."""
    import bench
    from cim_amd import mask_iou, synthetic
    from cim_amd.core.config import cfg
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling import heads
    from cim_amd.modeling.model_builder import Generalized_RCNN
    from cim_amd.ops import gemm, maskfuse_pair
    from cim_amd.optim import Adam, make_optimizer, sgd as _sgd
    from cim_amd.utils import net as net_utils

    def run(flag):
        monkeypatch.setattr(gemm, "HIGH_PRIO", flag)
        monkeypatch.setattr(maskfuse_pair, "DEFER_DW", flag)
        monkeypatch.setattr(maskfuse_pair, "DW_WGS", 256 if flag else 0)
        apply_preset("resnet50_voc")
        torch.manual_seed(cfg.RNG_SEED)
        model = Generalized_RCNN()
        bench.init_for_synthetic(model)
        model = model.to(dev).train()
        cfg.SOLVER.TYPE = "Adam"
        try:
            opt = make_optimizer(model)
        finally:
            cfg.SOLVER.TYPE = "SGD"
        assert type(opt) is Adam
        net_utils.update_learning_rate(opt, 0, ADAM_RUN_LR)     # (group 1 = biases: x2; touches no momentum_buffer)
        assert opt.param_groups[0]["lr"] == ADAM_RUN_LR and not any("momentum_buffer" in st for st in opt.state.values())
        opt.overlap_update = flag
        inp = synthetic.make_image_inputs("resnet50_voc", seed=3, n=300)
        iou, asy = mask_iou.mask_iou_maps(torch.from_numpy(inp["full_masks"]).to(dev))
        t = lambda a: torch.from_numpy(a).unsqueeze(0).to(dev)
        batch = dict(data=torch.from_numpy(inp["data"]).to(dev), rois=t(inp["rois"]), masks=t(inp["masks"]), labels=t(inp["labels"]),
                     mat=t(inp["mat"]), index=t(inp["index"]), iou_map=iou, asy_iou_map=asy, gtrois=None)
        np.random.seed(cfg.RNG_SEED)
        hist = []
        for s in range(40):
            opt.zero_grad(set_to_none=True)
            out = model(**batch)
            loss = sum(v.sum() for v in out["losses"].values())
            loss.backward()
            if s % 8 == 7:
                torch.cuda.synchronize()
                for n, p in model.named_parameters():
                    assert p.grad is None or bool(torch.isfinite(p.grad).all()), (s, n)
            opt.step()
            hist.append(float(loss))
        heads.settle_rng()
        sd = model.state_dict()            # (waits for an update still running on the side stream by itself)
        osd = opt.state_dict()
        big = max(model.parameters(), key=lambda p: p.numel())
        k = max(osd["state"], key=lambda k: osd["state"][k]["exp_avg"].numel())
        return hist, {k_: v.detach().clone() for k_, v in sd.items()}, osd["state"][k]["exp_avg"].clone(), big.numel()

    (on, sd_on, mom_on, nbig), (off, sd_off, mom_off, _) = run(True), run(False)
    print("ADAM_RUN " + json.dumps(dict(lr=ADAM_RUN_LR, losses=[round(x, 5) for x in on])))
    assert all(np.isfinite(on))
    assert on == off, [(i, a, b) for i, (a, b) in enumerate(zip(on, off)) if a != b][:3]
    assert nbig >= _sgd.TRAIL_MIN                                   # (the run did take the side-stream update)
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_off[k]), k                  # the trained weights, bit for bit
    assert torch.equal(mom_on, mom_off)
    assert on[-1] < on[0]
