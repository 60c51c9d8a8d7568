"""-m gpu: the trainable ResNet stem.  The 7 x 7 weight gradient of csrc/conv7x7_dw.hip straight at the C ABI -
against the float64 restatement (tests/golden/stem_dw_np.py) inside the worst-case bound of any fp32 summation order, bit for bit
on integer data, with poisoned outputs, guard words, determinism, two streams and every refusal - then the operator
`ops.conv7x7_bn_act_train`, the PRM training step after `prm_train.unfreeze`, and the detector body at FREEZE_AT = 0, each
against the same modules on the CPU in float64."""
import copy
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prm_cases
import stem_dw_np as sdn
from cases import GRAD_RTOL, VANISHING, VANISHING_ATOL          # tests/golden/cases.py: the project's rule for parameter gradients

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EPS = 2.0 ** -24
SENT = 0x7FC0BEEF        # a quiet NaN: what every output and workspace float holds before a call
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class _Guarded:
    """n floats preset to SENT between two runs of GUARD sentinel words."""

    def __init__(self, n, dev):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        self.ptr = self.raw.data_ptr() + 4 * GUARD

    def values(self):
        return self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def untouched(self):
        return bool((self.raw[GUARD:GUARD + self.n] == SENT).all())

    def guards_ok(self):
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.n:] == SENT).all())


def _sizes(shape):
    from cim_amd import _lib
    lib = _lib.load()
    b, cin, cout, h, w, s = shape
    ws_bytes, splits = lib.cim_conv7x7_dw_workspace(*shape), lib.cim_conv7x7_dw_splits(*shape)
    assert splits >= 1 and ws_bytes == splits * cout * cin * 49 * 4
    return ws_bytes // 4, splits


def run_dw(dev, shape, dconv, x, stream=None):
    """One cim_conv7x7_dw_f32 call on poisoned, guarded buffers -> dw [cout,cin,7,7] float32 on the host."""
    from cim_amd import _lib
    b, cin, cout, h, w, s = shape
    n_ws, _ = _sizes(shape)
    d, xx = torch.from_numpy(dconv).to(dev), torch.from_numpy(x).to(dev)
    out, ws = _Guarded(cout * cin * 49, dev), _Guarded(n_ws, dev)
    _lib.call("cim_conv7x7_dw_f32", d.data_ptr(), xx.data_ptr(), out.ptr, b, cin, cout, h, w, s, ws.ptr,
              _lib.stream_ptr() if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    got = out.values().clone()
    assert bool(torch.isfinite(got).all()), "an element of dw was not written (or is not finite)"
    assert out.guards_ok() and ws.guards_ok(), "a store outside dw or outside the workspace"
    return got.cpu().numpy().reshape(cout, cin, 7, 7)


_REF = {}


def reference(shape, integers):
    key = (shape, integers)
    if key not in _REF:
        dconv, x = sdn.seeded(shape, 11 + len(_REF), integers)
        _REF[key] = (dconv, x) + sdn.dw_and_abs(dconv, x, shape[5])
    return _REF[key]


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sdn.SHAPES)
def test_dw_within_the_fp32_summation_bound(dev, shape):
    dconv, x, ref, mag = reference(shape, False)
    got = run_dw(dev, shape, dconv, x).astype(np.float64)
    t = sdn.terms(shape)
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(EPS * mag, 1e-300)).max()) if mag.max() > 0 else 0.0
    print("shape %s  T = %d  worst err / (2^-24 sum|term|) = %.3f" % (shape, t, ratio))
    assert np.all(err <= (t + 1) * EPS * mag)


# ---- 2. exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sdn.SHAPES)
def test_dw_of_small_integers_is_exact(dev, shape):
    dconv, x, ref, mag = reference(shape, True)
    assert mag.max() < 2 ** 24
    got = run_dw(dev, shape, dconv, x)
    want = np.rint(ref).astype(np.int64)
    bad = got.astype(np.float64) != want
    assert not bad.any(), "%d of %d elements differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[0])
    assert np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, want.astype(np.float32).view(np.uint32) & 0x7FFFFFFF)


# ---- 3. layout, determinism, refusals ------------------------------------------------------------------------------------------------
def test_two_calls_and_two_streams_give_the_same_bits(dev):
    shapes = [(2, 3, 64, 75, 100, 2), (4, 1, 8, 112, 200, 1)]
    single = []
    for shape in shapes:
        dconv, x, _, _ = reference(shape, False)
        a, b = run_dw(dev, shape, dconv, x), run_dw(dev, shape, dconv, x)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        single.append(a)
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            dconv, x, _, _ = reference(shapes[k], False)
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(5):
                    got = run_dw(dev, shapes[k], dconv, x, stream)
                    assert np.array_equal(got.view(np.uint32), single[k].view(np.uint32)), (k, it)
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


REFUSED = {
    # name -> (argument overrides, what the message must name)
    "dconv": ({"dconv": None}, "dconv"),
    "x": ({"x": None}, "x"),
    "dw": ({"dw": None}, "dw"),
    "workspace": ({"workspace": None}, "workspace"),
    "B0": ({"B": 0}, "B"),
    "cin0": ({"cin": 0}, "cin"),
    "cin5": ({"cin": 5}, "cin"),
    "cout0": ({"cout": 0}, "cout"),
    "cout257": ({"cout": 257}, "cout"),
    "stride0": ({"stride": 0}, "stride"),
    "stride3": ({"stride": 3}, "stride"),
    "W4097": ({"H": 1, "W": 4097}, "W"),
    "HW": ({"H": 1024, "W": 1024}, "H * W"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_launch_nothing(dev, what):
    from cim_amd import _lib
    lib = _lib.load()
    over, names = REFUSED[what]
    a = {"B": 1, "cin": 3, "cout": 4, "H": 7, "W": 9, "stride": 1}
    d, x = torch.zeros(4 * 7 * 9, device=dev), torch.zeros(3 * 7 * 9, device=dev)
    out, ws = _Guarded(4 * 3 * 49, dev), _Guarded(4 * 3 * 49, dev)
    a.update({"dconv": d.data_ptr(), "x": x.data_ptr(), "dw": out.ptr, "workspace": ws.ptr})
    a.update(over)
    rc = lib.cim_conv7x7_dw_f32(a["dconv"], a["x"], a["dw"], a["B"], a["cin"], a["cout"], a["H"], a["W"], a["stride"], a["workspace"],
                                _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.cim_last_error().decode()
    assert rc == -1 and "cim_conv7x7_dw_f32" in msg and names in msg, msg
    assert out.untouched() and ws.untouched() and out.guards_ok() and ws.guards_ok()
    if not any(k in over for k in ("dconv", "x", "dw", "workspace")):
        shape = (a["B"], a["cin"], a["cout"], a["H"], a["W"], a["stride"])
        assert lib.cim_conv7x7_dw_workspace(*shape) == -1 and lib.cim_conv7x7_dw_splits(*shape) == -1


def test_splits_are_a_function_of_the_shape(dev):
    assert _sizes((2, 3, 64, 75, 100, 2))[1] == 40 and _sizes((4, 1, 8, 112, 200, 1))[1] == 392 and _sizes((1, 1, 1, 1, 1, 1))[1] == 1
    assert _sizes((16, 3, 64, 448, 448, 2))[1] == 697           # 6272 tiles, 9 per split


# ---- 4. the operator -----------------------------------------------------------------------------------------------------------------
def _stem(seed, stride, dev):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(3, 64, 7, stride=stride, padding=3, bias=False)
    bn = torch.nn.BatchNorm2d(64).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    return conv, bn


def _deviation(name, got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    err, norm = float((got - want).norm()), float(want.norm())
    print("%-40s |g| %.3e  err / |g| %.2e" % (name, norm, err / max(norm, 1e-300)))
    if norm / np.sqrt(want.numel()) < VANISHING:
        assert err / np.sqrt(want.numel()) <= VANISHING_ATOL, name
    else:
        assert err <= GRAD_RTOL * norm, name


@pytest.mark.parametrize("case", [(2, 3, 75, 100, 2), (2, 3, 31, 45, 1)])
def test_operator_against_float64_modules(dev, case):
    from cim_amd.ops import conv7x7_bn_act, conv7x7_bn_act_train, fallback
    b, cin, h, w, stride = case
    conv, bn = _stem(3 + stride, stride, dev)
    rconv, rbn = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    conv, bn = conv.to(dev), bn.to(dev)
    x = torch.randn(b, cin, h, w)
    ref = F.relu(rbn(rconv(x.double())))
    weight = torch.randn(ref.shape, dtype=torch.float64)
    (ref * weight).sum().backward()

    fallback.reset()
    y = conv7x7_bn_act_train(x.to(dev), conv, bn, relu=True)
    (y * weight.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert fallback.counts() == {}
    assert float((y.detach().cpu().double() - ref).abs().max()) <= 5e-6 * float(ref.abs().max())
    _deviation("conv.weight", conv.weight.grad, rconv.weight.grad)
    _deviation("bn.weight", bn.weight.grad, rbn.weight.grad)
    _deviation("bn.bias", bn.bias.grad, rbn.bias.grad)

    # refusals
    with pytest.raises(ValueError, match="data gradient"):
        conv7x7_bn_act_train(x.to(dev).requires_grad_(True), conv, bn)
    bn.train()
    with pytest.raises(ValueError, match="eval"):
        conv7x7_bn_act_train(x.to(dev), conv, bn)
    bn.eval()
    biased = torch.nn.Conv2d(3, 64, 7, stride=stride, padding=3, bias=True).to(dev)
    with pytest.raises(ValueError, match="bias"):
        conv7x7_bn_act_train(x.to(dev), biased, bn)

    # nothing to train: the frozen launch, bit for bit
    for p in list(conv.parameters()) + list(bn.parameters()):
        p.requires_grad = False
    a, c = conv7x7_bn_act_train(x.to(dev), conv, bn), conv7x7_bn_act(x.to(dev), conv, bn)
    assert torch.equal(a, c) and not a.requires_grad
    assert fallback.counts() == {}


# ---- 5. PRM, whole chain -------------------------------------------------------------------------------------------------------------
def test_unfrozen_thin_network_training_step_against_float64(dev):
    """prm_train.unfreeze, then one prm_train.loss(...).backward() of the thin fc_resnet50 of DESIGN.md 4.21 against the same modules
    on the CPU in float64 with the device's peak map as a constant mask: every parameter, the stem and layer1 included."""
    from cim_amd import prm, prm_train
    from cim_amd.ops import fallback
    d = np.load(os.path.join(GOLDEN, "prm_net.npz"))
    seed, gain = int(d["seed"]), float(d["gain"])
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, seed, gain / 10.0)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    prm_train.unfreeze(model)
    ref = copy.deepcopy(model).double()
    model = model.to(dev)
    h, w = prm_cases.NET_SHAPE
    x = prm_cases.normalise(prm_cases.seeded_images(seed, 2, h, w))
    target = (np.random.RandomState(2).rand(2, prm_cases.NUM_CLASSES) < 0.3).astype(np.float32)

    fallback.reset()
    agg, state = prm_train.aggregate(model, torch.from_numpy(x).to(dev))
    loss = prm_train.multilabel_soft_margin_loss(agg, torch.from_numpy(target).to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert fallback.counts() == {}
    assert int(state.status.abs().sum()) == 0

    crm = ref[0](torch.from_numpy(x).double())
    up = F.interpolate(crm, scale_factor=8, mode="bilinear", align_corners=True)
    mask = state.peak_map().cpu().double()
    ref_loss = F.multilabel_soft_margin_loss((up * mask).sum((2, 3)) / mask.sum((2, 3)), torch.from_numpy(target).double())
    ref_loss.backward()
    print("loss", float(loss), "float64", float(ref_loss))
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    names = []
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.requires_grad and p.grad is not None and q.grad is not None, name
        names.append(name)
        _deviation(name, p.grad, q.grad)
    for must in ("0.features.0.weight", "0.features.1.weight", "0.features.1.bias", "0.features.4.0.conv1.weight", "0.classifier.0.bias"):
        assert must in names


# ---- 6. the detector body at FREEZE_AT = 0 -------------------------------------------------------------------------------------------
def test_detector_body_trains_from_the_stem(dev):
    from cim_amd.core.config import cfg
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling import resnet50
    from cim_amd.ops import fallback
    apply_preset("resnet50_voc")
    old = cfg.ResNet.FREEZE_AT
    try:
        cfg.ResNet.FREEZE_AT = 0
        torch.manual_seed(5)
        body = resnet50.resnet().train()
        assert all(p.requires_grad for p in body.parameters())
        ref = copy.deepcopy(body).double()
        body = body.to(dev)
        x = torch.randn(1, 3, 64, 96)
        out_ref = ref(x.double())
        weight = torch.randn(out_ref.shape, dtype=torch.float64)
        (out_ref * weight).sum().backward()

        fallback.reset()
        out = body(x.to(dev))
        (out * weight.float().to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert fallback.counts() == {}
        # (ten fused layers deep, each held to 5e-6 of its maximum by its own test: 1e-4 is twice their sum)
        assert float((out.detach().cpu().double() - out_ref).abs().max()) <= 1e-4 * float(out_ref.abs().max())
        checked = 0
        for (name, p), (_, q) in zip(body.named_parameters(), ref.named_parameters()):
            if name.startswith(("res1.", "res2.")):
                assert p.grad is not None, name
                _deviation(name, p.grad, q.grad)
                checked += 1
        assert checked == 3 + 3 * 9 + 3                        # stem 3; three bottlenecks of 3 conv + 3 x 2 affine; downsample 3
    finally:
        cfg.ResNet.FREEZE_AT = old
