"""-m gpu: cim_amd.prm_train (csrc/prm_train.hip).  Peak set, aggregation, gradient and loss bit for bit against
the NumPy restatement (tests/golden/prm_train_np.py) and the golden captured from the reference; the thin network's training
step against the same modules on the CPU in float64; determinism, re-entrancy, and the unchanged peak entry of cim_amd.prm."""
import copy
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prm_cases
import prm_np
import prm_train_cases as cases
import prm_train_np as ptn
from cases import GRAD_RTOL, VANISHING, VANISHING_ATOL          # tests/golden/cases.py: the project's rule for parameter gradients

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_device(dev, crm, factor, bias=None, grad=None):
    """One forward (and backward for `grad` [B,C]) on the device -> dict of host arrays + the state."""
    from cim_amd import prm_train
    x = torch.from_numpy(crm).to(dev).requires_grad_(True)
    b = torch.from_numpy(bias).to(dev).requires_grad_(True) if bias is not None else None
    agg, state = prm_train.peak_stimulation(x, factor, b)
    out = {"agg": agg.detach().cpu().numpy(), "count": state.count.cpu().numpy(), "status": state.status.cpu().numpy(),
           "median": state.median.cpu().numpy(), "bitmap": state.bitmap.cpu().numpy().view(np.uint32), "state": state}
    if grad is not None:
        agg.backward(torch.from_numpy(grad).to(dev))
        out["dcrm"] = x.grad.cpu().numpy()
        out["dbias"] = b.grad.cpu().numpy() if b is not None else None
    return out


def check_against_restatement(got, want, crm_shape, factor, grad=None, with_bias=False):
    b, c, h, w = crm_shape
    np.testing.assert_array_equal(got["bitmap"], ptn.pack_bits(want["peaks"]))
    np.testing.assert_array_equal(got["count"], want["count"])
    np.testing.assert_array_equal(got["status"], want["status"])
    np.testing.assert_array_equal(bits(got["median"]), bits(want["median"]))
    np.testing.assert_array_equal(bits(got["agg"]), bits(want["agg"]))
    np.testing.assert_array_equal(got["state"].peak_list().cpu().numpy(), ptn.peak_list(want["peaks"]))
    if grad is not None:
        res = ptn.backward(grad, want["peaks"], h, w, factor, with_bias=with_bias)
        dcrm, dbias = res if with_bias else (res, None)
        np.testing.assert_array_equal(bits(got["dcrm"]), bits(dcrm))
        if with_bias:
            np.testing.assert_array_equal(bits(got["dbias"]), bits(dbias))


# ---- 1. crafted maps at factor 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_crafted_maps_equal_reference_and_restatement(dev, shape):
    g, key = load("prm_train"), "%dx%d" % shape
    maps, grad = cases.crafted_batch(shape), cases.grad_output(shape)
    want = ptn.stimulate(maps, 1)
    got = run_device(dev, maps, 1, grad=grad)
    check_against_restatement(got, want, maps.shape, 1, grad)
    # the reference's own peak list and counts: nothing left out, the degenerate maps included
    np.testing.assert_array_equal(got["state"].peak_list().cpu().numpy(), g[key + "__peak_list"])
    counts = np.zeros((cases.BATCH, cases.CLASSES), dtype=np.int64)
    np.add.at(counts, (g[key + "__peak_list"][:, 0], g[key + "__peak_list"][:, 1]), 1)
    np.testing.assert_array_equal(got["count"], counts)
    # dyadic values: the reference's aggregation is exact up to its one division, and so is the device's
    ok = got["status"] == 0
    np.testing.assert_array_equal(bits(got["agg"][ok]), bits(g[key + "__agg"][ok]))
    ref = g[key + "__grad"].astype(np.float64) / np.maximum(counts, 1)[:, :, None, None]      # (prm_modules.py:50 leaves the division out)
    assert np.all(np.abs(got["dcrm"][ok].astype(np.float64) - ref[ok]) <= 2 * 3 * EPS * np.abs(ref[ok]))
    # the degenerate maps: NaN aggregation, the status says why, the others of the call are untouched (checked above)
    names = dict(zip(cases.MAP_NAMES, zip(got["agg"].reshape(-1), got["status"].reshape(-1), got["count"].reshape(-1))))
    for name in ("neg_inf", "one_nan"):
        assert np.isnan(names[name][0]) and names[name][1] == ptn.STATUS_NAN and names[name][2] == 0
    assert (~ok).sum() == 2 and not got["dcrm"][~ok].any()
    with pytest.raises(ValueError, match="image 1, class 1"):                                  # neg_inf is map 6 = (1, 1)
        got["state"].check()
    assert by_name_peaks(got, shape)["constant"] == [(0, 0)]


def by_name_peaks(got, shape):
    pk = got["state"].peak_map().cpu().numpy().reshape((-1,) + shape)
    return {n: [tuple(p) for p in np.argwhere(m)] for n, m in zip(cases.MAP_NAMES, pk)}


def test_check_passes_on_ordinary_maps(dev):
    got = run_device(dev, cases.seeded_crm(3, 5, 1, 2, 1), 8)
    assert got["state"].check() is got["state"] and np.all(got["count"] >= 1)


# ---- 2. the up-sampling forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(2, 3), (1, 1)])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("form", cases.UPSAMPLE_FORMS)
def test_upsampling_forms_equal_restatement(dev, form, with_bias, bc):
    h, w, factor = form
    b, c = bc
    crm = cases.seeded_crm(h, w, b, c, 100 * h + 10 * w + factor)
    bias = (np.random.RandomState(c).randn(c) * 2).astype(np.float32) if with_bias else None
    grad = np.random.RandomState(b).randn(b, c).astype(np.float32)
    want = ptn.stimulate(crm, factor, bias)
    got = run_device(dev, crm, factor, bias, grad)
    check_against_restatement(got, want, crm.shape, factor, grad, with_bias)
    if h > 1 and w > 1:                                                                        # a border peak: two taps on one pixel
        assert want["peaks"][..., 0, :].any() or want["peaks"][..., -1, :].any() or want["peaks"][..., :, 0].any() or want["peaks"][..., :, -1].any()


# ---- 3. real-size calls: the LDS footprint of the workload, and the limit ---------------------------------------------------------
@pytest.mark.parametrize("h,c", [(14, 2), (16, 1)])
def test_real_size_maps_equal_restatement(dev, h, c):
    from cim_amd import prm_train
    assert (8 * 16) ** 2 == prm_train.STIM_MAX_HW and (8 * 17) ** 2 > prm_train.STIM_MAX_HW       # 16: the largest square h
    rng = np.random.RandomState(h)
    yy, xx = np.mgrid[0:h, 0:h]
    crm = np.stack([sum(rng.uniform(2, 9) * np.exp(-((yy - rng.uniform(0, h)) ** 2 + (xx - rng.uniform(0, h)) ** 2) / rng.uniform(2, 12))
                        for _ in range(12)) for _ in range(c)])[None].astype(np.float32)
    crm += rng.randn(*crm.shape).astype(np.float32) * np.float32(0.3)
    grad = rng.randn(1, c).astype(np.float32)
    want = ptn.stimulate(crm, 8)
    got = run_device(dev, crm, 8, grad=grad)
    check_against_restatement(got, want, crm.shape, 8, grad)
    assert np.all(want["count"] >= 2)
    with pytest.raises(ValueError, match="at most %d" % prm_train.STIM_MAX_HW):
        prm_train.peak_stimulation(torch.zeros(1, 1, 17, 17, device=dev), 8)


# ---- 4. the loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.loss_cases()))
def test_loss_equals_restatement_and_torch(dev, name):
    from cim_amd import prm_train
    x, t = cases.loss_cases()[name]
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    loss = prm_train.multilabel_soft_margin_loss(xd, torch.from_numpy(t).to(dev))
    (loss * 2.0).backward()
    want_loss, want_dagg = ptn.msm_loss(x, t)
    assert loss.dim() == 0 and bits(loss) == bits(want_loss)
    np.testing.assert_array_equal(bits(xd.grad), bits(want_dagg * np.float32(2.0)))
    xt = torch.from_numpy(x).double().requires_grad_(True)
    ref = F.multilabel_soft_margin_loss(xt, torch.from_numpy(t).double())
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert np.abs(xd.grad.cpu().numpy().astype(np.float64) / 2 - xt.grad.numpy()).max() <= 16 * EPS / x.size


# ---- 5. the network ------------------------------------------------------------------------------------------------------------------
def test_thin_network_training_step_against_float64(dev):
    """One prm_train.loss(...).backward() of the thin fc_resnet50 (width 16: every trained layer takes the HIP backward) on two
    64 x 96 images (CRM 2 x 3, up-sampled 16 x 24) against the same modules on the CPU (their ATen branch) in float64, whose
    head is the torch composition with the DEVICE's peak map as a constant mask."""
    from cim_amd import prm, prm_train
    from cim_amd.ops import fallback
    g = load("prm_net")
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, int(g["seed"]), float(g["gain"]) / 10.0)            # responses of a few units: no saturated loss
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    prm_train.freeze(model)
    ref = copy.deepcopy(model).double()
    model = model.to(dev)
    h, w = prm_cases.NET_SHAPE
    x = prm_cases.normalise(prm_cases.seeded_images(int(g["seed"]), 2, h, w))
    target = (np.random.RandomState(2).rand(2, prm_cases.NUM_CLASSES) < 0.3).astype(np.float32)

    fallback.reset()
    agg, state = prm_train.aggregate(model, torch.from_numpy(x).to(dev))
    loss = prm_train.multilabel_soft_margin_loss(agg, torch.from_numpy(target).to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert fallback.counts() == {}
    assert state.shape == (2, prm_cases.NUM_CLASSES, 2, 3) and state.up_shape == (16, 24) and int(state.status.abs().sum()) == 0
    again = prm_train.loss(model, torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev))
    assert bits(again) == bits(loss)                                                           # `loss` is aggregate + the loss

    crm = ref[0](torch.from_numpy(x).double())
    up = F.interpolate(crm, scale_factor=8, mode="bilinear", align_corners=True)
    mask = state.peak_map().cpu().double()
    ref_loss = F.multilabel_soft_margin_loss((up * mask).sum((2, 3)) / mask.sum((2, 3)), torch.from_numpy(target).double())
    ref_loss.backward()
    print("loss", float(loss), "float64", float(ref_loss))
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    trained = 0
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if not p.requires_grad:
            assert p.grad is None and q.grad is None, name
            continue
        trained += 1
        got, want = p.grad.cpu().double(), q.grad
        err, norm = float((got - want).norm()), float(want.norm())
        print("%-40s |g| %.3e  err / |g| %.2e" % (name, norm, err / max(norm, 1e-300)))
        if norm / np.sqrt(want.numel()) < VANISHING:
            assert err / np.sqrt(want.numel()) <= VANISHING_ATOL, name
        else:
            assert err <= GRAD_RTOL * norm, name
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert "0.classifier.0.weight" in names and "0.classifier.0.bias" in names and "0.features.5.0.conv2.weight" in names
    assert trained == len(names) and not any(n.startswith(("0.features.0", "0.features.1", "0.features.4")) for n in names)


# ---- 6. determinism and re-entrancy -------------------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bits(dev):
    crm, grad = cases.seeded_crm(5, 7, 2, 3, 9), np.random.RandomState(1).randn(2, 3).astype(np.float32)
    bias = np.array([0.5, -1.25, 2.0], dtype=np.float32)
    a, b = run_device(dev, crm, 8, bias, grad), run_device(dev, crm, 8, bias, grad)
    for k in ("agg", "median", "dcrm", "dbias"):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]))
    for k in ("count", "status", "bitmap"):
        np.testing.assert_array_equal(a[k], b[k])


def test_two_threads_two_streams(dev):
    from cim_amd import prm_train
    inputs = [(cases.seeded_crm(3, 5, 2, 3, 40 + k), np.random.RandomState(k).randn(2, 3).astype(np.float32),
               cases.loss_cases()["soft" if k else "hard"]) for k in range(2)]
    wants = []
    for crm, grad, (lx, lt) in inputs:
        res = ptn.stimulate(crm, 8)
        wants.append((res, ptn.backward(grad, res["peaks"], 3, 5, 8), ptn.msm_loss(lx, lt)))
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            crm, grad, (lx, lt) = inputs[k]
            res, dcrm, (wl, wd) = wants[k]
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(10):
                    x = torch.from_numpy(crm).to(dev).requires_grad_(True)
                    agg, state = prm_train.peak_stimulation(x, 8)
                    agg.backward(torch.from_numpy(grad).to(dev))
                    xl = torch.from_numpy(lx).to(dev).requires_grad_(True)
                    loss = prm_train.multilabel_soft_margin_loss(xl, torch.from_numpy(lt).to(dev))
                    loss.backward()
                    stream.synchronize()
                    assert np.array_equal(bits(agg), bits(res["agg"])) and np.array_equal(bits(x.grad), bits(dcrm)), (k, it)
                    assert np.array_equal(state.bitmap.cpu().numpy().view(np.uint32), ptn.pack_bits(res["peaks"])), (k, it)
                    assert bits(loss) == bits(wl) and np.array_equal(bits(xl.grad), bits(wd)), (k, it)
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- 7. the neighbour whose median select was hoisted -------------------------------------------------------------------------------
def test_peak_entry_of_prm_is_unchanged(dev):
    from cim_amd import prm
    crm = cases.seeded_crm(5, 7, 2, 4, 21) * np.float32(3.0)
    labels = [[0, 2], [3, 1]]
    res, run = prm.peaks_from_crm(torch.from_numpy(crm).to(dev), labels, 8, peak_threshold=prm_cases.THRESHOLD, details=True)
    first = 0
    for i, ls in enumerate(labels):
        maps = list(prm_np.upsample(crm, [(i, c) for c in ls], 8))
        want = prm_np.image_points(maps, ls, 40, 56, prm_cases.THRESHOLD)
        assert want["status"] == 0 and want["count"] >= 1
        rows, cols, classes, scores = res[i]
        np.testing.assert_array_equal(classes, want["classes"])
        np.testing.assert_array_equal(run.ys_xs[i][0], want["ys"])
        np.testing.assert_array_equal(run.ys_xs[i][1], want["xs"])
        np.testing.assert_array_equal(bits(scores), bits(want["scores"]))
        for q, m in enumerate(maps):
            med, npk, valid, flags = prm_np.pair_peaks(m, prm_cases.THRESHOLD)
            assert bits(run.median[first + q]) == bits(med) and run.pair_counts[first + q].tolist() == [npk, len(valid), flags]
        first += len(ls)
