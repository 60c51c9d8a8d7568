"""-m gpu: the PRM peak back-propagation (cim_amd/prm_backprop.py, csrc/prm_backprop.hip).

The stages straight at the C ABI inside guarded, NaN-poisoned memory (tests/golden/abi_guards.py) on data chosen so that the fp32
result is exact - gate, minimum / shift, seed, stem bit for bit against their definitions - then the thin network against the
peak response maps captured from the reference (tests/golden/prm_backprop.npz) within the reference's own fp32 error, batching,
the high-level call, and one full-size run on invariants."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prm_backprop_np as bp
import prm_cases
import prm_np
from abi_guards import NAN, _Out, _Ws, _poisoned16, _same

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EPS = np.float32(1e-10)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def call(name, *args):
    from cim_amd import _lib
    return _lib.call(name, *args)


def guarded(a, dev):
    """A dense float32 array inside NaN, 16-byte aligned."""
    return _poisoned16(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev))


# ---- 1. gate ----------------------------------------------------------------------------------------------------------------
def gate_reference(g, mul, y, a, n):
    """The definition in float64 on data whose every intermediate is exact in fp32 -> (dconv, dres) float32."""
    g = g.astype(np.float64) * (mul.astype(np.float64)[None] if mul is not None else 1.0)
    t = np.where(y[None] > 0, g, 0.0) if y is not None else g
    d = t * a.astype(np.float64)[None, :, None] if a is not None else t
    n32 = n.astype(np.float32)
    den = (np.abs(n32) + EPS).astype(np.float32).astype(np.float64)          # |n| + 1e-10 rounded to fp32: n itself for n >= 2^-8
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(n32[None] < EPS, 0.0, d / den[None])
    return out.astype(np.float32), t.astype(np.float32)


def run_gate(dev, g, mul, y, a, n, want_res):
    p, c, hw = g.shape
    bufs = [None if v is None else guarded(v, dev) for v in (g, mul, y, a, n)]
    ptr = [None if b is None else b.data_ptr() for b in bufs]
    dconv = _Out(p, c * hw, 0, dev, shift=0)
    dres = _Out(p, c * hw, 0, dev, shift=0) if want_res else None
    call("cim_prmb_gate", ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], dconv.ptr, dres.ptr if dres else None, p, c, hw, None)
    torch.cuda.synchronize()
    return dconv.check().reshape(p, c, hw).cpu(), (dres.check().reshape(p, c, hw).cpu() if dres else None)


@pytest.mark.parametrize("hw", [1, 63, 64, 65])
@pytest.mark.parametrize("p", [1, 3])
def test_gate_is_the_definition_bit_for_bit(dev, p, hw):
    """g dyadic; a, n and mul powers of two (n >= 2^-8: |n| + 1e-10 rounds to n, the quotient is exact).  Every combination of
    y / a / mul given or NULL, dres on and off; a < 0 and closed ReLU gates among the values.  HW = 64 takes the float4 path."""
    c = 4
    rng = np.random.RandomState(100 * p + hw)
    g = rng.randint(-64, 65, (p, c, hw)).astype(np.float32) / 8
    n = np.ldexp(1.0, rng.randint(-8, 4, (c, hw))).astype(np.float32)
    y = np.where(rng.rand(c, hw) < 0.4, 0.0, rng.rand(c, hw) + 0.5).astype(np.float32)      # y = 0: the gate is closed
    y.reshape(-1)[0] = 0.0
    a = (np.ldexp(1.0, rng.randint(-3, 3, c)) * np.array([1, -1, 1, -1])).astype(np.float32)
    mul = np.ldexp(1.0, rng.randint(-2, 3, (c, hw))).astype(np.float32)
    for has_y in (True, False):
        for has_a in (True, False):
            for has_mul, want_res in ((False, True), (True, False), (False, False)):
                args = (g, mul if has_mul else None, y if has_y else None, a if has_a else None, n)
                want, want_res_v = gate_reference(*args)
                got, got_res = run_gate(dev, *args, want_res)
                _same(got, torch.from_numpy(want), "dconv y=%s a=%s mul=%s" % (has_y, has_a, has_mul))
                if want_res:
                    _same(got_res, torch.from_numpy(want_res_v), "dres y=%s a=%s" % (has_y, has_a))


def test_gate_named_normalisers(dev):
    """n = 0, 5e-11 and -1 give 0 (n < 1e-10); n = 2e-10 is kept: within 1 ulp of the fp32 formula g a / (|n| + 1e-10)."""
    c, hw, p = 4, 63, 3
    rng = np.random.RandomState(7)
    g = rng.randint(1, 65, (p, c, hw)).astype(np.float32) / 8
    n = np.ldexp(1.0, rng.randint(-8, 4, (c, hw))).astype(np.float32)
    n[0, :4] = [0.0, 5e-11, -1.0, 2e-10]
    n[3, -4:] = [2e-10, -1.0, 5e-11, 0.0]
    a = np.array([2.0, -0.5, 1.0, -4.0], dtype=np.float32)
    y = np.ones((c, hw), dtype=np.float32)
    got, _ = run_gate(dev, g, None, y, a, n, False)
    got = got.numpy()
    for ch, cols in ((0, (0, 1, 2)), (3, (hw - 3, hw - 2, hw - 1))):
        assert (got[:, ch, list(cols)] == 0).all()
    for ch, col in ((0, 3), (3, hw - 4)):
        want = (g[:, ch, col] * a[ch]).astype(np.float32) / (np.abs(n[ch, col]) + EPS).astype(np.float32)
        ulp = np.spacing(np.abs(want).astype(np.float32))
        assert (np.abs(got[:, ch, col].astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (got[:, ch, col], want)
        assert np.isfinite(got[:, ch, col]).all() and (got[:, ch, col] != 0).all()
    rest = np.ones((c, hw), dtype=bool)
    rest[0, :4] = rest[3, -4:] = False
    want, _ = gate_reference(g, None, y, a, n)
    assert np.array_equal(got[:, rest], want[:, rest])


# ---- 2. minimum / shift -------------------------------------------------------------------------------------------------------
MIN_CASES = {"one": np.array([3.5]), "ragged": np.arange(1000, 0, -1) / 4.0, "last_negative": np.r_[np.arange(1, 700) / 2.0, -7.25],
             "all_equal": np.full(513, 2.0), "beyond_the_grid": None}


@pytest.mark.parametrize("name", list(MIN_CASES))
def test_minimum_and_shift(dev, name):
    """One element; a length that is no multiple of the 256-thread block; a negative minimum in the last element; all equal; more
    elements than CIM_PRMB_MIN_MAX_PARTS blocks cover in one pass (the strided loop), the minimum behind the first pass."""
    x = MIN_CASES[name]
    if x is None:
        x = np.random.RandomState(3).randint(-1000, 1000, 256 * 1024 + 77).astype(np.float64)
        x[-5] = -4096.0
    x = x.astype(np.float32)
    n = x.size
    parts = call("cim_prmb_min_parts", n)
    assert parts == min((n + 255) // 256, 1024)
    xd = guarded(x, dev)
    out, part, xs = _Out(1, 1, 0, dev, shift=0), _Ws(parts, dev, shift=0), _Out(1, n, 0, dev, shift=0)
    call("cim_prmb_min", xd.data_ptr(), n, out.ptr, part.ptr, None)
    call("cim_prmb_shift", xd.data_ptr(), out.ptr, xs.ptr, n, None)
    torch.cuda.synchronize()
    part.check()
    assert float(out.check()[0, 0]) == float(x.min())
    _same(xs.check().cpu().reshape(-1), torch.from_numpy(x - x.min()), "xs")


# ---- 2b. scale ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("p", [1, 3])
def test_scale_is_the_definition_bit_for_bit(dev, p, n):
    """dx = xs * dxraw (+ add) on dyadic data: exact.  n = 64 takes the float4 path, the others the scalar one; `add` on and off."""
    rng = np.random.RandomState(10 * n + p)
    xs = rng.randint(0, 33, n).astype(np.float32) / 4
    dxraw = rng.randint(-64, 65, (p, n)).astype(np.float32) / 8
    add = rng.randint(-64, 65, (p, n)).astype(np.float32) / 16
    xd, rd, ad = guarded(xs, dev), guarded(dxraw, dev), guarded(add, dev)
    for has_add in (False, True):
        want = xs.astype(np.float64)[None] * dxraw + (add if has_add else 0.0)
        out = _Out(p, n, 0, dev, shift=0)
        call("cim_prmb_scale", xd.data_ptr(), rd.data_ptr(), ad.data_ptr() if has_add else None, out.ptr, p, n, None)
        torch.cuda.synchronize()
        _same(out.check().cpu(), torch.from_numpy(want), "scale add=%s" % has_add)


# ---- 3. seed --------------------------------------------------------------------------------------------------------------------
def seed_peaks(h, w, factor):
    """The four corners, one weight (a source pixel), between four (where the grid has them), in classes 0..2."""
    H, W = h * factor, w * factor
    pts = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (min(3, H - 1), min(5, W - 1)), (H - 1, W // 3)}
    return np.array([(i % 3, y, x) for i, (y, x) in enumerate(sorted(pts))], dtype=np.int32)


@pytest.mark.parametrize("factor", [1, 8])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (14, 14)])
def test_seed_is_the_adjoint_of_the_upsampling(dev, hw, factor):
    h, w = hw
    c = 3
    peaks = seed_peaks(h, w, factor)
    p = len(peaks)
    rng = np.random.RandomState(10 * h + factor)
    n = np.ldexp(1.0, rng.randint(-8, 4, (c, h, w))).astype(np.float32)
    if h * w > 1:
        n.reshape(-1)[::5] = 0.0                                  # no gradient passes where the normaliser vanishes
    crm = rng.randint(-20, 21, (1, c, h, w)).astype(np.float32)
    up = prm_np.upsample(crm, [(0, k) for k in range(c)], factor)
    want = np.zeros((p, c, h, w), dtype=np.float32)
    weights = 0
    for k, pk in enumerate(peaks):
        adj = bp.upsample_adjoint(pk, h, w, factor)
        weights = max(weights, int((adj != 0).sum()))
        # the adjoint: <adj, crm> is the up-sampled value at the peak, to the rounding of four products and three sums
        dot = float((adj.astype(np.float64) * crm[0, pk[0]]).sum())
        assert abs(dot - float(up[pk[0], pk[1], pk[2]])) <= 8 * 2.0 ** -24 * 20
        assert abs(float(adj.astype(np.float64).sum()) - 1.0) <= 4 * 2.0 ** -24
        with np.errstate(divide="ignore", invalid="ignore"):
            want[k, pk[0]] = np.where(n[pk[0]] < EPS, np.float32(0), adj / (np.abs(n[pk[0]]) + EPS).astype(np.float32))
    assert weights == (1 if factor == 1 or h * w == 1 else 4)
    pk_dev = torch.from_numpy(peaks).to(dev)
    nd = guarded(n, dev)
    out = _Out(p, c * h * w, 0, dev, shift=0)
    call("cim_prmb_seed", pk_dev.data_ptr(), nd.data_ptr(), out.ptr, p, c, h, w, factor, None)
    torch.cuda.synchronize()
    _same(out.check().cpu().reshape(p, c, h, w), torch.from_numpy(want), "seed")


# ---- 4. stem ------------------------------------------------------------------------------------------------------------------
def stem_reference(ghat, wpos, xs):
    """float64 on integer data: exact.  -> s [P, H, W] before the division."""
    H, W = xs.shape[1:]
    ho, wo = ghat.shape[2:]
    op = (H - ((ho - 1) * 2 - 6 + 7), W - ((wo - 1) * 2 - 6 + 7))
    dx = F.conv_transpose2d(torch.from_numpy(ghat).double(), torch.from_numpy(wpos).double(), None, 2, 3, op)
    return (dx * torch.from_numpy(xs).double()[None]).sum(1).clamp(min=0).numpy()


@pytest.mark.parametrize("shape", [(1, 1), (9, 11), (16, 16), (9, 40)])
@pytest.mark.parametrize("cout", [4, 16, 20])
def test_stem_is_the_definition_bit_for_bit(dev, cout, shape):
    """Integer data: every product and sum is exact in fp32, so is the float64 reference.  cout = 20: two channel groups of the
    LDS patch; 16 x 16 and 9 x 40: more than one workgroup per axis; 1 x 1 and the odd sides: ragged tiles, taps outside the grid.
    The dividing launch against the float64 sum."""
    H, W = shape
    p = 2
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rng = np.random.RandomState(1000 * cout + 10 * H + W)
    ghat = rng.randint(-2, 4, (p, cout, ho, wo)).astype(np.float32)
    wpos = rng.randint(0, 4, (cout, 3, 7, 7)).astype(np.float32)
    xs = rng.randint(0, 5, (3, H, W)).astype(np.float32)
    s = stem_reference(ghat, wpos, xs)
    assert s.max() < 2 ** 24
    gd, wd, xd = guarded(ghat, dev), guarded(wpos, dev), guarded(xs, dev)
    nbytes = call("cim_prmb_stem_workspace", p, H, W)
    assert nbytes == 8 * p * ((H + 7) // 8) * ((W + 31) // 32)
    for normalise in (0, 1):
        out = _Out(p, H * W, 0, dev, shift=0)
        ws = torch.full((nbytes // 8,), NAN, dtype=torch.float64, device=dev)
        call("cim_prmb_stem", gd.data_ptr(), wd.data_ptr(), xd.data_ptr(), out.ptr, ws.data_ptr(), p, cout, H, W, normalise, None)
        torch.cuda.synchronize()
        got = out.check(finite=False).cpu().numpy().reshape(p, H, W)
        if normalise:
            total = s.reshape(p, -1).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                want = s.astype(np.float32) / total.astype(np.float32)[:, None, None]
            assert np.array_equal(ws.cpu().numpy().reshape(p, -1).sum(1), total)
        else:
            want = s.astype(np.float32)
        np.testing.assert_array_equal(got, want)


# ---- 5. the thin network against the reference ------------------------------------------------------------------------------------
def thin_model(golden, dev, edit=None):
    from cim_amd import prm
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, int(golden["seed"]), float(golden["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    if edit is not None:
        edit(model)
    return model.to(dev)


@pytest.fixture(scope="module")
def net(dev):
    """The golden, the model, the two images and - computed ONCE - the maps of all peaks of each image in one call."""
    from cim_amd import prm
    g = load("prm_backprop")
    model = thin_model(g, dev)
    h, w = prm_cases.NET_SHAPE
    x = torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(int(g["seed"]), 2, h, w))).to(dev)
    maps = [prm.backprop(model, x[i:i + 1], g["peaks_%d" % i]) for i in range(2)]
    return g, model, x, maps


def deviation(got, g, i, k):
    """(max |got - prm32| / max prm64, the bound 4 max |prm32 - prm64| / max prm64 + 1e-12) of map k of image i."""
    p32, p64 = g["prm32_%d" % i][k].astype(np.float64), g["prm64_%d" % i][k]
    scale = p64.max()
    return np.abs(got.astype(np.float64) - p32).max() / scale, 4 * np.abs(p32 - p64).max() / scale + 1e-12


def within_bound(maps, g, i, what):
    maps = maps.cpu().numpy()
    assert maps.shape == g["prm32_%d" % i].shape and maps.dtype == np.float32
    for k in range(maps.shape[0]):
        dev_err, bound = deviation(maps[k], g, i, k)
        print("%s image %d map %d: deviation %.3e, bound %.3e, ratio %.3f" % (what, i, k, dev_err, bound, dev_err / bound))
        assert dev_err <= bound, (what, i, k, dev_err, bound)


def test_the_device_routes_the_max_pool_as_the_reference_does(net):
    """The arg-max of every max-pool window on the device against the restatement's (float64; the generator asserts that fp32 and
    float64 agree).  The smallest lead of a winner at this seed (`pool_margins`) is about the forward bound itself and the device's
    stem sums in another order, so equal routing is not guaranteed by a margin: it is checked here, and a window that flips is
    reported as that, not as an unexplained deviation of the maps."""
    from cim_amd import prm_backprop
    g, model, x, maps = net
    cpu = thin_model(g, torch.device("cpu"))
    ref = bp.Network(cpu[0].features, cpu[0].classifier[0], torch.float64)
    for i in range(2):
        ref.forward(x[i:i + 1].cpu())
        got = prm_backprop.Forward(model, x[i:i + 1]).pool_idx.cpu().numpy().astype(np.int64)
        want = ref.idx[0].numpy()
        flips = np.argwhere(got != want)
        assert flips.size == 0, "image %d: %d max-pool windows route to another pixel than the reference's, the first (c, oy, ox) = %s" % (
            i, len(flips), flips[0].tolist())


def test_thin_network_matches_the_reference_maps(net):
    """Per map: max |device - prm32| / max prm64 <= 4 max |prm32 - prm64| / max prm64 + 1e-12 - the rule tests/test_prm_cpu.py
    applies to this network's forward: the reference's own fp32 error bounds what summation order may move."""
    g, model, x, maps = net
    import cases
    rows = []
    for i in range(2):
        got = maps[i].cpu().numpy()
        for k in range(got.shape[0]):
            d, bound = deviation(got[k], g, i, k)
            rows.append({"image": i, "map": k, "deviation": float(d), "bound": float(bound), "ratio": float(d / bound)})
    cases.record_deviation("prm peak response maps vs reference | thin network, fp32",
                           {"rule": "per map: max |device - prm32| / max prm64 <= 4 max |prm32 - prm64| / max prm64 + 1e-12",
                            "maps": rows, "worst_ratio": max(r["ratio"] for r in rows)})
    for i in range(2):
        assert np.isfinite(maps[i].cpu().numpy()).all()
        within_bound(maps[i], g, i, "all peaks")


def test_batching_each_alone_and_chunks(net):
    from cim_amd import prm
    g, model, x, maps = net
    for i in range(2):
        peaks = g["peaks_%d" % i]
        p = len(peaks)
        alone = torch.cat([prm.backprop(model, x[i:i + 1], peaks[k:k + 1]) for k in range(p)])
        within_bound(alone, g, i, "each alone")
        within_bound(prm.backprop(model, x[i:i + 1], peaks, chunk=1), g, i, "chunk 1")
        again = prm.backprop(model, x[i:i + 1], peaks, chunk=p)
        within_bound(again, g, i, "chunk P")
        assert torch.equal(again, maps[i]), "two calls with the same arguments differ"
        print("image %d: each alone bit-equal to one call: %s; chunk 1: %s" % (
            i, torch.equal(alone, maps[i]), torch.equal(prm.backprop(model, x[i:i + 1], peaks, chunk=1), maps[i])))


def test_peaks_as_a_device_tensor_and_reversed_order(net):
    from cim_amd import prm
    g, model, x, maps = net
    peaks = torch.from_numpy(g["peaks_1"]).to(x.device)
    assert torch.equal(prm.backprop(model, x[1:2], peaks), maps[1])
    within_bound(prm.backprop(model, x[1:2], g["peaks_1"][::-1].copy()).flip(0), g, 1, "reversed")


def test_high_level_call_returns_the_rows_of_peaks_and_aligned_maps(net):
    from cim_amd import prm
    g, model, x, maps = net
    labels = [load("prm_net")["labels"][i].tolist() for i in range(2)]
    sizes = [(50, 70), (64, 96)]
    want, run = prm.peaks(model, x, labels, prm_cases.THRESHOLD, sizes, details=True)
    got = prm.peak_response_maps(model, x, labels, prm_cases.THRESHOLD, sizes)
    assert len(got) == 2
    for i in range(2):
        for a, b in zip(got[i][:4], want[i]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        pm = got[i][4]
        ys, xs = run.ys_xs[i]
        peaks = np.stack([want[i][2], ys, xs], 1)
        assert pm.is_cuda and tuple(pm.shape) == (len(peaks),) + prm_cases.NET_SHAPE
        # row k of the maps belongs to row k of the peaks: the same peak sent back by the low-level call, and the golden's map
        assert torch.equal(pm, prm.backprop(model, x[i:i + 1], peaks))
        order = [g["peaks_%d" % i].tolist().index(list(pk)) for pk in peaks.tolist()]
        for k, j in enumerate(order):
            d, bound = deviation(pm[k].cpu().numpy(), g, i, j)
            assert d <= bound, (i, k, d, bound)


def test_high_level_call_on_an_image_without_classes(net):
    """P = 0 for one image of the batch: its first four entries are what `prm.peaks` returns for it (empty), its maps [0, S, S'];
    the other image is untouched by its neighbour.  Every list empty is the ValueError `prm.peaks` raises."""
    from cim_amd import prm
    g, model, x, maps = net
    labels = load("prm_net")["labels"]
    for lab in ([labels[0].tolist(), []], [[], labels[1].tolist()]):
        want = prm.peaks(model, x, lab, prm_cases.THRESHOLD)
        got = prm.peak_response_maps(model, x, lab, prm_cases.THRESHOLD)
        for i in range(2):
            for a, b in zip(got[i][:4], want[i]):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
            pm = got[i][4]
            assert pm.is_cuda and pm.dtype == torch.float32 and tuple(pm.shape) == (len(want[i][0]),) + prm_cases.NET_SHAPE
            if not lab[i]:
                assert pm.shape[0] == 0
            else:
                full = prm.peak_response_maps(model, x[i:i + 1], [lab[i]], prm_cases.THRESHOLD)[0][4]
                assert pm.shape[0] > 0 and torch.equal(pm, full)
    for entry in (prm.peaks, prm.peak_response_maps):
        with pytest.raises(ValueError, match="every image has an empty class list"):
            entry(model, x, [[], []])


def test_a_class_without_a_positive_weight_gives_nan_and_leaves_its_neighbours(net):
    from cim_amd import prm
    g, model, x, maps = net
    c_nan = int(g["nan_class"])

    def edit(m):
        with torch.no_grad():
            wt = m[0].classifier[0].weight
            wt[c_nan] = -wt[c_nan].abs()
    edited = thin_model(g, x.device, edit)
    peaks = g["nan_peaks"]
    got = prm.backprop(edited, x[0:1], peaks)
    plain = prm.backprop(model, x[0:1], peaks)
    ref = g["nan_prm32"]
    hit = 0
    for k, pk in enumerate(peaks.tolist()):
        if pk[0] == c_nan:
            assert bool(torch.isnan(got[k]).all()) and np.isnan(ref[k]).all()
            hit += 1
        else:
            assert torch.equal(got[k], plain[k]), "a map next to the NaN map changed"
            j = g["peaks_0"].tolist().index(pk)
            d, bound = deviation(got[k].cpu().numpy(), g, 0, j)
            assert d <= bound and np.array_equal(ref[k], g["prm32_0"][j])
    assert 0 < hit < len(peaks)
    # the high-level call on the same model: the class's rows are NaN, the others are not
    labels = g["nan_labels"].tolist()
    rows, cols, classes, scores, pm = prm.peak_response_maps(edited, x[0:1], [labels], prm_cases.THRESHOLD)[0]
    nan_rows = torch.isnan(pm).reshape(len(classes), -1)
    assert np.array_equal(nan_rows.all(1).cpu().numpy(), classes == c_nan) and np.array_equal(nan_rows.any(1).cpu().numpy(), classes == c_nan)
    assert (classes == c_nan).any() and (classes != c_nan).any()


def test_no_peak_returns_an_empty_result_and_prepares_nothing(net):
    """P = 0 -> [0, H, W]; on a model that has never been walked neither the forward pass nor the cached W+ is made for it."""
    from cim_amd import prm, prm_backprop
    g, model, x, maps = net
    fresh = thin_model(g, x.device)
    out = prm.backprop(fresh, x[0:1], np.zeros((0, 3), dtype=np.int64))
    assert tuple(out.shape) == (0,) + prm_cases.NET_SHAPE and id(fresh) not in prm_backprop._PLANS
    out = prm.peak_response_maps(fresh, x, [[], [0]])[0]
    assert tuple(out[4].shape) == (0,) + prm_cases.NET_SHAPE and id(fresh) in prm_backprop._PLANS          # (image 1 was walked)
    for empty in (np.zeros((0, 3), dtype=np.int64), [], torch.zeros((0, 3), dtype=torch.int64)):
        out = prm.backprop(model, x[0:1], empty)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (0,) + prm_cases.NET_SHAPE


def test_refusals_on_the_device(net):
    from cim_amd import prm
    g, model, x, maps = net
    with pytest.raises(ValueError, match="one image at a time"):
        prm.backprop(model, x, g["peaks_0"])
    with pytest.raises(ValueError, match="outside the 16 x 24"):
        prm.backprop(model, x[0:1], [[0, 16, 0]])
    with pytest.raises(ValueError, match="class 20"):
        prm.backprop(model, x[0:1], torch.tensor([[20, 0, 0]], device=x.device))


# ---- 6. full size ---------------------------------------------------------------------------------------------------------------
def test_full_size_invariants(dev):
    """448 x 448, width 64, two peaks: finite, non-negative, each map sums to 1 within 1e-5.  No reference at that size."""
    from cim_amd import prm
    torch.manual_seed(5)
    model = prm.PeakResponseMapping(prm.fc_resnet50(20)).to(dev)
    x = torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(9, 1, 448, 448))).to(dev)
    maps = prm.backprop(model, x, [[3, 5, 100], [17, 111, 0]])
    assert tuple(maps.shape) == (2, 448, 448)
    m = maps.double().cpu()
    assert bool(torch.isfinite(m).all()) and bool((m >= 0).all())
    sums = m.reshape(2, -1).sum(1)
    print("full size sums - 1:", (sums - 1).tolist())
    assert bool(((sums - 1).abs() <= 1e-5).all())
