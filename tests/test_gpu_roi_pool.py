"""-m gpu: RoIPool.  csrc/roi_pool.hip straight at the C ABI - forward bit for bit against the restatement
(tests/golden/roi_pool_np.py) on seeded, tie-ridden and -inf / NaN data, plain and mask-cat, with and without the argmax;
backward exact on integers and inside the bound of any summation order otherwise, with poisoned outputs and scratch, guard
words, determinism, K == 0 and two streams - then the operators, MaskFuse under ROI_XFORM_METHOD = RoIPoolF against float64,
and the resnet50_voc model with that method."""
import threading

import numpy as np
import pytest
import torch

import roi_pool_np as rp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # unit roundoff of fp32
SENT = 0x7FC0BEEF        # a quiet NaN (as an index: far outside any map): what every output and scratch word holds before a call
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class _Guarded:
    """n 4-byte words preset to SENT between two runs of GUARD sentinel words."""

    def __init__(self, n, dev):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        self.ptr = self.raw.data_ptr() + 4 * GUARD

    def untouched(self):
        return bool((self.raw == SENT).all())

    def guards_ok(self):
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.n:] == SENT).all())

    def host(self, shape, dtype=np.float32):
        body = self.raw[GUARD:GUARD + self.n]
        assert self.guards_ok(), "a store outside an output or outside the scratch"
        assert not bool((body == SENT).any()), "an output element was not written"
        return body.cpu().numpy().view(dtype).reshape(shape)


def _nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def _nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _st(stream):
    from cim_amd import _lib
    return _lib.stream_ptr() if stream is None else stream.cuda_stream


def run_fwd(dev, feat, rois, P, scale, masks=None, with_argmax=True, stream=None):
    """One forward call on poisoned, guarded buffers; NCHW host arrays in and out -> (out or cat, argmax or None)."""
    from cim_amd import _lib
    B, C, H, W = feat.shape
    K, OC = len(rois), C if masks is None else 2 * C
    f, r = _t(_nhwc(feat), dev), _t(np.asarray(rois, np.float32), dev)
    out, arg = _Guarded(K * P * P * OC, dev), _Guarded(K * P * P * C, dev)
    if masks is None:
        _lib.call("cim_roi_pool_fwd", f.data_ptr(), r.data_ptr(), out.ptr, arg.ptr if with_argmax else None, B, C, H, W, K, P, scale,
                  _st(stream))
    else:
        m = _t(np.asarray(masks, np.float32), dev)
        _lib.call("cim_roi_pool_maskcat_fwd", f.data_ptr(), r.data_ptr(), m.data_ptr(), out.ptr, arg.ptr if with_argmax else None,
                  B, C, H, W, K, P, scale, _st(stream))
    (stream or torch.cuda.current_stream()).synchronize()
    if not with_argmax:
        assert arg.untouched()
    return _nchw(out.host((K, P, P, OC))), _nchw(arg.host((K, P, P, C), np.int32)) if with_argmax else None


def run_bwd(dev, dy, rois, argmax, shape, P, scale, masks=None, stream=None):
    """One backward call: grad_in and the scratch poisoned and guarded -> grad_in [B,C,H,W]."""
    from cim_amd import _lib
    B, C, H, W = shape
    K = len(rois)
    g, r, a = _t(_nhwc(dy), dev), _t(np.asarray(rois, np.float32), dev), _t(_nhwc(argmax).astype(np.int32), dev)
    nbytes = _lib.call("cim_roi_pool_bwd_scratch", K, B, C, H, W, P)
    assert nbytes % (4 * B * C * H * W) == 0
    gin, scratch = _Guarded(B * H * W * C, dev), _Guarded(nbytes // 4, dev)
    if masks is None:
        _lib.call("cim_roi_pool_bwd", g.data_ptr(), r.data_ptr(), a.data_ptr(), gin.ptr, B, C, H, W, K, P, scale,
                  scratch.ptr if nbytes else None, _st(stream))
    else:
        m = _t(np.asarray(masks, np.float32), dev)
        _lib.call("cim_roi_pool_maskcat_bwd", g.data_ptr(), r.data_ptr(), m.data_ptr(), a.data_ptr(), gin.ptr, B, C, H, W, K, P, scale,
                  scratch.ptr if nbytes else None, _st(stream))
    (stream or torch.cuda.current_stream()).synchronize()
    assert scratch.guards_ok(), "a store outside the scratch"
    return _nchw(gin.host((B, H, W, C)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the cases: inputs and references, computed once and shared (never modified) ----------------------------------------------------
_CASES = {}
A_KEYS = [("A", C, P, s) for C in rp.A_CHANNELS for P, s in rp.A_VARIANTS]
B_KEY = ("B", rp.B_CHANNELS, rp.B_P, rp.B_SCALE)


def case(key, kind="normal"):
    full = key + (kind,)
    if full not in _CASES:
        name, C, P, scale = key
        (B, H, W), rois = (rp.A_SHAPE, rp.A_ROIS) if name == "A" else (rp.B_SHAPE, rp.b_rois())
        seed = 100 + len(_CASES)
        rs = np.random.RandomState(seed)
        feat = rp.seeded_feat((B, C, H, W), seed, kind)
        out, arg = rp.forward(feat, rois, P, scale)
        K = len(rois)
        d = {"feat": feat, "rois": rois, "P": P, "scale": scale, "out": out, "arg": arg, "shape": (B, C, H, W),
             "dy_int": rs.randint(-3, 4, (K, C, P, P)).astype(np.float32), "dy": rs.standard_normal((K, C, P, P)).astype(np.float32),
             "dcat_int": rs.randint(-3, 4, (K, 2 * C, P, P)).astype(np.float32),
             "dcat": rs.standard_normal((K, 2 * C, P, P)).astype(np.float32),
             "m01": (rs.rand(K, P, P) > 0.4).astype(np.float32), "mfrac": rs.uniform(-1.5, 1.5, (K, P, P)).astype(np.float32)}
        _CASES[full] = d
    return _CASES[full]


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", A_KEYS + [B_KEY], ids=lambda k: "%s-C%d-P%d-s%g" % k)
def test_forward_is_the_restatement_bit_for_bit(dev, key):
    kinds = ("normal", "ints", "special") if key[0] == "A" else ("normal", "ints")
    for kind in kinds:
        d = case(key, kind)
        out, arg = run_fwd(dev, d["feat"], d["rois"], d["P"], d["scale"])
        assert np.array_equal(arg, d["arg"]), kind
        assert np.array_equal(_bits(out), _bits(d["out"])), kind
        out2, none = run_fwd(dev, d["feat"], d["rois"], d["P"], d["scale"], with_argmax=False)       # inference: argmax == NULL
        assert none is None and np.array_equal(_bits(out2), _bits(d["out"])), kind
        if kind == "special" and d["P"] == 7 and d["scale"] == 1 / 16.0:
            lost = out == -rp.FLT_MAX
            assert lost.sum() > 100 and np.all(arg[lost] == -1) and lost[5, 1].all()


@pytest.mark.parametrize("key", [("A", 8, 7, 1 / 16.0), ("A", 6, 7, 1 / 16.0), ("A", 6, 14, 1 / 16.0), B_KEY], ids=lambda k: "%s-C%d-P%d-s%g" % k)
def test_maskcat_forward(dev, key):
    """cat[:, :C] = v and cat[:, C:] = fl(v * m), bit for bit, with {0, 1} and with fractional masks; argmax as the plain form's."""
    for kind in ("normal", "special") if key[0] == "A" else ("normal",):
        d = case(key, kind)
        C = key[1]
        for masks in (d["m01"], d["mfrac"]):
            want, _ = rp.maskcat_forward(d["feat"], d["rois"], masks, d["P"], d["scale"])
            cat, arg = run_fwd(dev, d["feat"], d["rois"], d["P"], d["scale"], masks=masks)
            assert np.array_equal(arg, d["arg"])
            assert np.array_equal(_bits(cat[:, :C]), _bits(d["out"]))
            assert np.array_equal(_bits(cat[:, C:]), _bits(want[:, C:]))
            cat2, _ = run_fwd(dev, d["feat"], d["rois"], d["P"], d["scale"], masks=masks, with_argmax=False)
            assert np.array_equal(_bits(cat2), _bits(cat))


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def _within(got, want, n, mag, extra=0):
    bound = (n + extra) * U * mag
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("   worst err / bound %.3g (most terms on one element: %d)" % (worst, int(n.max())))
    assert np.all(err <= bound)


@pytest.mark.parametrize("key", A_KEYS + [B_KEY], ids=lambda k: "%s-C%d-P%d-s%g" % k)
def test_backward_exact_on_integers_and_inside_the_summation_bound(dev, key):
    from cim_amd import _lib
    d = case(key)
    shape, rois, P, scale, arg = d["shape"], d["rois"], d["P"], d["scale"], d["arg"]
    if key == B_KEY:
        assert _lib.call("cim_roi_pool_bwd_scratch", len(rois), *shape, P) >= 2 * 4 * int(np.prod(shape))      # several ROI groups
    # plain: small integers - every sum exact
    want, n, mag = rp.backward(d["dy_int"], arg, rois, shape)
    got = run_bwd(dev, d["dy_int"], rois, arg, shape, P, scale)
    assert np.array_equal(got.astype(np.float64), want)
    assert (int(n.max()) > 1 or P == 1) and np.all(got[n == 0] == 0)         # (from P 7 on, bins of one ROI share pixels)
    # plain: normal dy - any order of n terms; two calls, the same bits
    want, n, mag = rp.backward(d["dy"], arg, rois, shape)
    got = run_bwd(dev, d["dy"], rois, arg, shape, P, scale)
    _within(got, want, n, mag)
    assert np.array_equal(_bits(got), _bits(run_bwd(dev, d["dy"], rois, arg, shape, P, scale)))
    # mask-cat: integers and {0, 1} masks exact; normal dcat and fractional masks inside the bound with one more rounding
    want, n, mag = rp.maskcat_backward(d["dcat_int"], d["m01"], arg, rois, shape)
    got = run_bwd(dev, d["dcat_int"], rois, arg, shape, P, scale, masks=d["m01"])
    assert np.array_equal(got.astype(np.float64), want)
    want, n, mag = rp.maskcat_backward(d["dcat"], d["mfrac"], arg, rois, shape)
    got = run_bwd(dev, d["dcat"], rois, arg, shape, P, scale, masks=d["mfrac"])
    _within(got, want, n, mag, extra=1)
    assert np.array_equal(_bits(got), _bits(run_bwd(dev, d["dcat"], rois, arg, shape, P, scale, masks=d["mfrac"])))


@pytest.mark.parametrize("C", rp.A_CHANNELS)
def test_no_rois(dev, C):
    """K == 0: the forward writes nothing, the backward an all-zero grad_in (every per-ROI pointer NULL)."""
    from cim_amd import _lib
    B, H, W = rp.A_SHAPE
    feat = torch.ones(B * H * W * C, device=dev)
    out, arg, gin = _Guarded(49 * C, dev), _Guarded(49 * C, dev), _Guarded(B * H * W * C, dev)
    masks = torch.ones(49, device=dev)
    assert _lib.call("cim_roi_pool_bwd_scratch", 0, B, C, H, W, 7) == 0
    for maskcat in (False, True):
        m = (masks.data_ptr(),) if maskcat else ()
        _lib.call("cim_roi_pool_maskcat_fwd" if maskcat else "cim_roi_pool_fwd", feat.data_ptr(), None, *m, out.ptr, arg.ptr,
                  B, C, H, W, 0, 7, 1 / 16.0, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert out.untouched() and arg.untouched()
        gin.raw.fill_(SENT)
        _lib.call("cim_roi_pool_maskcat_bwd" if maskcat else "cim_roi_pool_bwd", None, None, *((None,) if maskcat else ()), None, gin.ptr,
                  B, C, H, W, 0, 7, 1 / 16.0, None, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert np.all(gin.host((B, H, W, C)) == 0)


def _both(dev, key, stream=None):
    d = case(key)
    out, arg = run_fwd(dev, d["feat"], d["rois"], d["P"], d["scale"], masks=d["mfrac"], stream=stream)
    g1 = run_bwd(dev, d["dy"], d["rois"], arg, d["shape"], d["P"], d["scale"], stream=stream)
    g2 = run_bwd(dev, d["dcat"], d["rois"], arg, d["shape"], d["P"], d["scale"], masks=d["mfrac"], stream=stream)
    return [out, arg.view(np.float32), g1, g2]


def test_two_streams_give_the_same_bits(dev):
    """The re-entrancy the header promises: the same calls from two host threads on two streams at once."""
    keys = [B_KEY, ("A", 8, 7, 1 / 16.0)]
    single = [_both(dev, k) for k in keys]
    torch.cuda.synchronize()
    errors = []

    def worker(i):
        try:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(3):
                    got = _both(dev, keys[i], stream)
                    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(got, single[i])), (i, it)
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- the operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("A", 8, 7, 1 / 16.0), ("A", 6, 14, 1 / 16.0), B_KEY], ids=lambda k: "%s-C%d-P%d-s%g" % k)
def test_operator_against_the_restatement(dev, key):
    from cim_amd import ops
    d = case(key)
    B, C, H, W = d["shape"]
    P, scale, rois = d["P"], d["scale"], _t(d["rois"], dev)
    # a non-contiguous input: the map is a slice of a wider tensor
    wide = torch.zeros(B, C, H, W + 3, device=dev)
    wide[..., 1:W + 1] = _t(d["feat"], dev)
    x = wide[..., 1:W + 1].requires_grad_(True)
    assert not x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
    for call in (lambda t: ops.roi_pool(t, rois, P, scale), ops.RoIPool(P, scale), lambda t: ops.roi_pool(t, rois, (P, P), spatial_scale=scale)):
        x.grad = None
        out = call(x, rois) if isinstance(call, torch.nn.Module) else call(x)
        assert tuple(out.shape) == (len(d["rois"]), C, P, P)
        assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(d["out"]))
        out.backward(_t(d["dy_int"], dev))
        want, n, mag = rp.backward(d["dy_int"], d["arg"], d["rois"], d["shape"])
        assert tuple(x.grad.shape) == (B, C, H, W) and np.array_equal(x.grad.cpu().numpy().astype(np.float64), want)
    with torch.no_grad():                                       # inference: no argmax is kept
        out = ops.roi_pool(x, rois, P, scale)
    assert not out.requires_grad and np.array_equal(_bits(out.cpu().numpy()), _bits(d["out"]))
    out = ops.roi_pool(x.detach(), rois, P, scale)
    assert out.grad_fn is None
    with pytest.raises(ValueError, match="square"):
        ops.roi_pool(x, rois, (P, P + 1), scale)
    with pytest.raises(TypeError, match="float32"):
        ops.roi_pool(x.detach().double(), rois, P, scale)
    # the mask-cat operator: values, and the fold of the two halves' gradients
    masks = _t(d["m01"], dev)
    x.grad = None
    cat = ops.roi_pool_maskcat(x, rois, masks, P, scale)
    want_cat, _ = rp.maskcat_forward(d["feat"], d["rois"], d["m01"], P, scale)
    assert np.array_equal(_bits(cat.detach().cpu().numpy()), _bits(want_cat))
    cat.backward(_t(d["dcat_int"], dev))
    want, n, mag = rp.maskcat_backward(d["dcat_int"], d["m01"], d["arg"], d["rois"], d["shape"])
    assert np.array_equal(x.grad.cpu().numpy().astype(np.float64), want)


# ---- MaskFuse -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def roipoolf():
    """The resnet50_voc preset with ROI_XFORM_METHOD = RoIPoolF; the method is put back afterwards."""
    from cim_amd.core.config import cfg
    from cim_amd.core.presets import apply_preset
    apply_preset("resnet50_voc")
    before = cfg.FAST_RCNN.ROI_XFORM_METHOD
    cfg.FAST_RCNN.ROI_XFORM_METHOD = "RoIPoolF"
    yield cfg
    cfg.FAST_RCNN.ROI_XFORM_METHOD = before


def test_maskfuse_under_roipoolf_against_float64(dev, roipoolf):
    """seg_x and the gradients of x and the six parameters within 1e-5 (relative) of float64: box_x gathered by the restatement's
    argmax (a differentiable index gather), concat, conv, ReLU, the two linear layers.  As tests/test_gpu_gemm_pair.py does, the
    instance is drawn so that no ReLU pre-activation lies within 4e-6 of zero: one flipped mask is a property of ReLU, not of
    either evaluation."""
    from cim_amd.modeling.maskfuse import MaskFuse
    from cim_amd.ops import gemm
    _, H, W = rp.A_SHAPE
    C, P, scale = 64, 7, 1 / 16.0
    rois = rp.A_ROIS[rp.A_ROIS[:, 0] == 0]
    K = len(rois)
    lin = torch.nn.functional.linear
    for seed in range(64):
        torch.manual_seed(seed)
        rs = np.random.RandomState(seed)
        feat = rs.standard_normal((1, C, H, W)).astype(np.float32)
        masks = (rs.rand(K, P, P) > 0.4).astype(np.float32)
        head = MaskFuse(C, None, scale)
        dy = torch.randn(K, head.dim_out)
        params = [head.mask_branch[0].weight, head.mask_branch[0].bias, head.seg_fc[0].weight, head.seg_fc[0].bias,
                  head.seg_fc[2].weight, head.seg_fc[2].bias]
        _, arg = rp.forward(feat, rois, P, scale)
        x64 = torch.from_numpy(feat).double().requires_grad_(True)
        p64 = [t.detach().double().requires_grad_(True) for t in params]
        idx = torch.from_numpy(arg.astype(np.int64))                                    # [K,C,P,P]
        flat = x64[0].reshape(C, H * W)
        box = torch.gather(flat.unsqueeze(0).expand(K, C, H * W), 2, idx.clamp(min=0).reshape(K, C, P * P)).reshape(K, C, P, P)
        box = box * (idx >= 0)
        cat = torch.cat([box, box * torch.from_numpy(masks).double()[:, None]], 1)
        z0 = torch.nn.functional.conv2d(cat, p64[0], p64[1], padding=1)
        z1 = lin(z0.relu().reshape(K, -1), p64[2], p64[3])
        z2 = lin(z1.relu(), p64[4], p64[5])
        if min(float(z.detach().abs().min()) for z in (z0, z1, z2)) > 4e-6:
            break
    else:
        raise AssertionError("no instance with unambiguous ReLU masks in 64 draws")
    want = z2.relu()
    want.backward(dy.double())

    head = head.to(dev)
    x = torch.from_numpy(feat).to(dev).requires_grad_(True)
    out = head(x, torch.from_numpy(rois).to(dev), torch.from_numpy(masks).to(dev))
    out.backward(dy.to(dev))
    gemm.join_side()
    torch.cuda.synchronize()
    e = float((out.detach().cpu().double() - want.detach()).abs().max() / want.detach().abs().max())
    print("seed %d  seg_x: %.3g of max" % (seed, e))
    assert e < 1e-5, "seg_x deviates from float64 by %.3g" % e
    dev_params = [head.mask_branch[0].weight, head.mask_branch[0].bias, head.seg_fc[0].weight, head.seg_fc[0].bias,
                  head.seg_fc[2].weight, head.seg_fc[2].bias]
    for name, got, ref in zip(["x", "wc", "bc", "w1", "b1", "w2", "b2"], [x] + dev_params, [x64] + p64):
        assert got.grad is not None, name
        e = float((got.grad.cpu().double() - ref.grad).norm() / ref.grad.norm())
        print("   gradient of %s: %.3g of its norm" % (name, e))
        assert e < 1e-5, "gradient of %s deviates from float64 by %.3g" % (name, e)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _small_batch(seed, n, dev):
    from cim_amd import mask_iou, synthetic
    inp = synthetic.make_image_inputs("resnet50_voc", seed=seed, n=n)
    inp["data"] = inp["data"][:, :, :160, :224].copy()
    inp["rois"][:, 1:] *= np.float32(0.3)
    iou, asy = mask_iou.mask_iou_maps(torch.from_numpy(inp["full_masks"]).to(dev))
    return inp, iou, asy


def test_model_trains_and_infers_with_roipoolf(dev, roipoolf):
    from cim_amd import ops
    from cim_amd.modeling.model_builder import Generalized_RCNN
    from cim_amd.ops import gemm
    torch.manual_seed(0)
    model = Generalized_RCNN().to(dev).train()
    inp, iou, asy = _small_batch(77, 40, dev)
    t = lambda a: torch.from_numpy(a).unsqueeze(0).to(dev)
    np.random.seed(9)
    out = model(data=torch.from_numpy(inp["data"]).to(dev), rois=t(inp["rois"]), masks=t(inp["masks"]), labels=t(inp["labels"]),
                gtrois=None, mat=t(inp["mat"]), index=t(inp["index"]), iou_map=iou, asy_iou_map=asy)
    assert set(out["losses"]) == {"bag_loss", "pcl_loss", "cls_loss", "iou_loss"}
    assert all(v.shape == (1,) and bool(torch.isfinite(v).all()) for v in out["losses"].values())
    sum(v.sum() for v in out["losses"].values()).backward()
    gemm.join_side()
    torch.cuda.synchronize()
    last = [p for p in model.Conv_Body.parameters() if p.requires_grad and p.dim() == 4][-1]
    assert last.grad is not None and bool(torch.isfinite(last.grad).all()) and float(last.grad.abs().max()) > 0

    model.eval()
    data, rois, masks = (torch.from_numpy(inp[k]).to(dev) for k in ("data", "rois", "masks"))
    runs = [model(data=data, rois=rois, masks=masks, labels=None, gtrois=None, mat=None)["refine_score"] for _ in range(2)]
    assert len(runs[0]) == 3 and all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(*runs))

    with torch.no_grad():
        x = model.Conv_Body(data)
        got = model.roi_feature_transform(x, rois)                    # the signature's default method: RoIPoolF
        assert tuple(got.shape) == (40, x.shape[1], 7, 7) and torch.equal(got, ops.roi_pool(x, rois, 7, 1 / 16.0))
