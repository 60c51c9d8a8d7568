"""-m gpu: cim_amd.prm (csrc/prm.hip, the PRM network on the fused kernels).  The peak entry bit for bit against
the goldens captured from the reference (tests/golden/prm_peaks.npz) and the NumPy restatement (tests/golden/prm_np.py) on
crafted exact maps; the up-sampling bit for bit against the restatement; the thin network against the reference's class response
maps within the reference's own rounding error; `label_assign` end to end against the reference's `mat`; two host threads on two
streams; the refusals."""
import os
import threading

import numpy as np
import pytest
import torch

import prm_cases
import prm_np
import proposal_prep_np as ppn

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FACTOR = 8


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
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def thin_model(golden, dev):
    from cim_amd import prm
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, int(golden["seed"]), float(golden["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.to(dev)


def check_image(got, run, i, want, first_pair, maps, threshold):
    """One image of a device call against prm_np.image_points + pair_peaks on the same maps: bit for bit."""
    rows, cols, classes, scores = got
    np.testing.assert_array_equal(classes, want["classes"])
    np.testing.assert_array_equal(run.ys_xs[i][0], want["ys"])
    np.testing.assert_array_equal(run.ys_xs[i][1], want["xs"])
    np.testing.assert_array_equal(rows, want["rows"])
    np.testing.assert_array_equal(cols, want["cols"])
    np.testing.assert_array_equal(bits(scores), bits(want["scores"]))
    for q, m in enumerate(maps):
        med, npk, valid, flags = prm_np.pair_peaks(m, threshold)
        assert bits(run.median[first_pair + q]) == bits(med), (i, q)
        assert run.pair_counts[first_pair + q].tolist() == [npk, len(valid), flags], (i, q)


# ---- 1. the peak entry on given maps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in prm_cases.crafted() if n != "many_257"])
def test_peak_entry_equals_reference_and_restatement(dev, name):
    from cim_amd import prm
    g, case = load("prm_peaks"), prm_cases.crafted()[name]
    labels, thr = case["labels"], case["threshold"]
    maps = [case["maps"][c] for c in labels]
    h, w = maps[0].shape
    up = torch.from_numpy(np.stack(maps)).to(dev)
    res, run = prm.peaks_from_maps(up, [labels], image_sizes=[(3 * h + 1, 5 * w + 2)], peak_threshold=thr, details=True)
    rows, cols, classes, scores = res[0]
    order = g[name + "__order"]
    np.testing.assert_array_equal(np.stack([classes, run.ys_xs[0][0], run.ys_xs[0][1]], 1), g[name + "__valid"][order])
    np.testing.assert_array_equal(bits(scores), bits(g[name + "__scores"][order]))
    for q, c in enumerate(labels):
        assert run.pair_counts[q, 0] == int(np.sum(g[name + "__all"][:, 0] == c))
    check_image(res[0], run, 0, prm_np.image_points(maps, labels, 3 * h + 1, 5 * w + 2, thr), 0, maps, thr)


def test_two_images_in_one_call_and_equal_scores_keep_their_order(dev):
    """B = 2 with different pair counts and image sizes; image 1 holds equal scores in two classes: the order is stable
    (pairs, then row-major)."""
    from cim_amd import prm
    rng = np.random.RandomState(5)
    a = [rng.randint(0, 40, (9, 11)).astype(np.float32) for _ in range(3)]
    tie = np.zeros((9, 11), dtype=np.float32)
    tie[1, 1] = tie[1, 5] = tie[6, 3] = 25
    tie[4, 8] = 12
    labels = [[4, 0, 2], [3, 1]]
    maps = a + [tie, tie[::-1].copy()]
    sizes = [(375, 500), (60, 33)]
    res, run = prm.peaks_from_maps(torch.from_numpy(np.stack(maps)).to(dev), labels, image_sizes=sizes, details=True)
    check_image(res[0], run, 0, prm_np.image_points(maps[:3], labels[0], 375, 500, 10), 0, maps[:3], 10)
    want = prm_np.image_points(maps[3:], labels[1], 60, 33, 10)
    check_image(res[1], run, 1, want, 3, maps[3:], 10)
    assert want["scores"].tolist() == [12, 12, 25, 25, 25, 25, 25, 25] and want["classes"].tolist() == [3, 1, 3, 3, 3, 1, 1, 1]


def test_257_valid_peaks_and_nan_are_errors_naming_the_image(dev):
    from cim_amd import prm
    case = prm_cases.crafted()["many_257"]
    many = case["maps"][0]
    g = load("prm_peaks")
    assert g["many_257__scores"].size == 257                                       # the reference itself has no limit
    with pytest.raises(ValueError, match=r"image 0 has 257 valid peaks"):
        prm.peaks_from_maps(torch.from_numpy(many[None]).to(dev), [[0]])
    ok = np.zeros_like(many)
    ok[0, 3] = 11
    two = torch.from_numpy(np.stack([ok, many])).to(dev)
    with pytest.raises(ValueError, match=r"image 1 has 257 valid peaks"):
        prm.peaks_from_maps(two, [[0], [0]])
    split = many.copy()                                                            # 256 in one class + 1 in another: the IMAGE's count
    split[0, -1] = 0
    one = np.zeros_like(many)
    one[0, 7] = 30
    with pytest.raises(ValueError, match=r"image 0 has 257 valid peaks"):
        prm.peaks_from_maps(torch.from_numpy(np.stack([split, one])).to(dev), [[0, 1]])
    res = prm.peaks_from_maps(torch.from_numpy(split[None]).to(dev), [[0]])        # 256 are taken
    assert res[0][3].tolist() == (20 + np.arange(256)).tolist()
    bad = ok.copy()
    bad[0, 100] = np.nan
    with pytest.raises(ValueError, match=r"image 1 has a NaN"):
        prm.peaks_from_maps(torch.from_numpy(np.stack([ok, bad])).to(dev), [[0], [2]])
    with pytest.raises(ValueError, match=r"image 0 has a processed class response map without any peak"):
        prm.peaks_from_maps(torch.full((1, 3, 4), -np.inf, device=dev), [[0]])


def test_median_of_a_large_map_with_many_duplicates(dev):
    from cim_amd import prm
    m = prm_cases.duplicates_map()
    assert m.shape == (320, 416)
    res, run = prm.peaks_from_maps(torch.from_numpy(m[None]).to(dev), [[0]], peak_threshold=np.inf, details=True)
    k = (m.size - 1) // 2
    assert run.median[0] == np.partition(m.reshape(-1), k)[k]
    assert bits(run.median[0]) == bits(prm_np.lower_median(m))
    med, npk, valid, flags = prm_np.pair_peaks(m, np.inf)
    assert run.pair_counts[0].tolist() == [npk, 1, 0] and npk > 1                   # +inf is the fallback, an ordinary value
    assert (int(run.ys_xs[0][0][0]), int(run.ys_xs[0][1][0])) == valid[0][:2] and np.isinf(res[0][3][0])


# ---- 2. up-sampling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (2, 3), (5, 7), (14, 14)])
@pytest.mark.parametrize("factor", [1, 3, 8])
def test_upsample_equals_restatement(dev, hw, factor):
    from cim_amd import prm
    rng = np.random.RandomState(hw[0] * 100 + hw[1] * 10 + factor)
    crm = (rng.randn(2, 5, *hw) * 20).astype(np.float32)
    bias = (rng.randn(5) * 3).astype(np.float32)
    labels = [[3, 0], [4]]                                                         # a class subset, out of class order
    pairs = [(0, 3), (0, 0), (1, 4)]
    d = torch.from_numpy(crm).to(dev)
    up = prm.upsample(d, labels, factor)
    assert tuple(up.shape) == (3, hw[0] * factor, hw[1] * factor)
    np.testing.assert_array_equal(bits(up.cpu().numpy()), bits(prm_np.upsample(crm, pairs, factor)))
    up_b = prm.upsample(d, labels, factor, bias=torch.from_numpy(bias).to(dev))
    np.testing.assert_array_equal(bits(up_b.cpu().numpy()), bits(prm_np.upsample(crm, pairs, factor, bias)))
    if factor == 1:
        np.testing.assert_array_equal(up.cpu().numpy(), crm[[0, 0, 1], [3, 0, 4]])


# ---- 3. the network ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(dev):
    g = load("prm_net")
    model = thin_model(g, dev)
    h, w = prm_cases.NET_SHAPE
    x = torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(int(g["seed"]), 2, h, w))).to(dev)
    return g, model, x, model(x)


def test_thin_network_matches_the_reference_maps(net):
    """Per map: max |crm - ref32| <= 4 x max |ref32 - ref64|, both over max |ref64|: two fp32 evaluations of the same float64
    value, compared by the reference's own rounding error (four-fold: the fused kernels sum in another order)."""
    g, model, x, crm = net
    crm = crm.cpu().numpy()
    assert crm.shape == (2, 20, 2, 3)
    worst = 0.0
    for i in range(2):
        for c in range(20):
            scale = np.abs(g["crm64"][i, c]).max()
            ref_err = np.abs(g["crm32"][i, c].astype(np.float64) - g["crm64"][i, c]).max() / scale
            err = np.abs(crm[i, c].astype(np.float64) - g["crm32"][i, c]).max() / scale
            print("image %d class %2d: device-ref32 %.3e  ref32-ref64 %.3e  ratio %.2f" % (i, c, err, ref_err, err / ref_err))
            worst = max(worst, err / ref_err)
    print("largest ratio %.3f" % worst)
    assert worst <= 4.0


def test_batch_of_one_and_two_give_identical_maps(net):
    g, model, x, crm = net
    for i in range(2):
        assert torch.equal(model(x[i:i + 1])[0], crm[i])


def test_network_peaks_equal_the_reference(net):
    from cim_amd import prm
    g, model, x, crm = net
    labels = g["labels"].tolist()
    res, run = prm.peaks(model, x, labels, details=True)
    for i in range(2):
        order = g["order_%d" % i]
        np.testing.assert_array_equal(np.stack([res[i][2], run.ys_xs[i][0], run.ys_xs[i][1]], 1), g["valid_%d" % i][order])
        np.testing.assert_allclose(res[i][3], g["scores_%d" % i][order], rtol=1e-4, atol=1e-4)
    # the launches of csrc/prm.hip on the device's own maps: bit for bit the restatement on those maps
    host = crm.cpu().numpy()
    first = 0
    for i in range(2):
        up = prm_np.upsample(host[i][None], [(0, c) for c in labels[i]], FACTOR)
        want = prm_np.image_points(list(up), labels[i], up.shape[1], up.shape[2], prm_cases.THRESHOLD)
        check_image(res[i], run, i, want, first, list(up), prm_cases.THRESHOLD)
        first += len(labels[i])


def test_strict_load_with_the_reference_key_list(dev):
    from cim_amd import prm
    g = load("prm_net")
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH)).to(dev)
    sd = model.state_dict()
    assert list(sd) == g["keys"].tolist()
    model.load_state_dict({k: sd[k].clone() for k in g["keys"].tolist()}, strict=True)


def test_network_input_is_totensor_normalize_bit_for_bit(dev):
    from cim_amd import prm
    rgb = np.random.RandomState(2).randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    rgb[0, 0, :6, 0] = (0, 1, 127, 128, 254, 255)
    got = prm.network_input(torch.from_numpy(rgb).to(dev))
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(prm_cases.normalise(rgb)))
    np.testing.assert_array_equal(prm.network_input(rgb[1]).cpu().numpy()[0], got[1].cpu().numpy())


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def test_label_assign_equals_the_reference_mat(dev):
    from cim_amd import prm
    from cim_amd import proposal_prep as pp
    g = load("prm_e2e")
    model = thin_model(g, dev)
    images = [g["rgb_%d" % i] for i in range(3)]
    labels = [g["labels_%d" % i].tolist() for i in range(3)]
    masks = [ppn.unpack_bits(g["mask_bits_%d" % i], g["mask_shape_%d" % i]) for i in range(3)]
    mats = pp.label_assign(model, images, labels, [torch.from_numpy(m).to(dev) for m in masks])
    for i in range(3):
        assert mats[i].dtype == torch.float32 and tuple(mats[i].shape) == (masks[i].shape[0], 21)
        np.testing.assert_array_equal(mats[i].cpu().numpy(), g["mat_%d" % i])
    # peaks, the scores' order and the points
    from PIL import Image
    resized = np.stack([np.asarray(Image.fromarray(im).resize((448, 448), Image.BILINEAR)) for im in images])
    sizes = [m.shape[1:] for m in masks]
    res, run = prm.peaks(model, prm.network_input(torch.from_numpy(resized).to(dev)), labels, image_sizes=sizes, details=True)
    for i in range(3):
        order = g["order_%d" % i]
        valid = g["valid_%d" % i][order]
        np.testing.assert_array_equal(np.stack([res[i][2], run.ys_xs[i][0], run.ys_xs[i][1]], 1), valid)
        np.testing.assert_array_equal(res[i][0], [int(y * sizes[i][0] / 112) for y in valid[:, 1]])     # AGPL_label_assign.py:158
        np.testing.assert_array_equal(res[i][1], [int(x * sizes[i][1] / 112) for x in valid[:, 2]])
        np.testing.assert_allclose(res[i][3], g["scores_%d" % i][order], rtol=1e-4, atol=1e-4)
        assert np.all(np.diff(res[i][3]) > 0)
    assert len(res[1][3]) == 1 and res[1][3][0] < 10                               # the fallback image
    # an image without classes: the reference's `visual_cues == None` matrix
    mats = pp.label_assign(model, images[:2], [labels[0], []], [torch.from_numpy(m).to(dev) for m in masks[:2]])
    np.testing.assert_array_equal(mats[0].cpu().numpy(), g["mat_0"])
    want = np.zeros((masks[1].shape[0], 21), dtype=np.float32)
    want[:, 0] = 1
    np.testing.assert_array_equal(mats[1].cpu().numpy(), want)


# ---- 5. the full-size peak shapes ---------------------------------------------------------------------------------------------
def test_full_size_maps_equal_restatement(dev):
    from cim_amd import prm
    rng = np.random.RandomState(9)
    yy, xx = np.mgrid[0:14, 0:14]
    crm = np.zeros((1, 20, 14, 14), dtype=np.float32)
    for c in range(20):
        for _ in range(5):
            cy, cx, s = rng.uniform(0, 13), rng.uniform(0, 13), rng.uniform(0.8, 3)
            crm[0, c] += (rng.uniform(-25, 25) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))).astype(np.float32)
        crm[0, c] += (rng.randn(14, 14) * 0.5).astype(np.float32)
    labels = [[2, 11, 17]]
    res, run = prm.peaks_from_crm(torch.from_numpy(crm).to(dev), labels, FACTOR, image_sizes=[(375, 500)], details=True)
    up = prm_np.upsample(crm, [(0, c) for c in labels[0]], FACTOR)
    assert up.shape == (3, 112, 112)
    want = prm_np.image_points(list(up), labels[0], 375, 500, prm_cases.THRESHOLD)
    assert want["count"] >= 3
    check_image(res[0], run, 0, want, 0, list(up), prm_cases.THRESHOLD)


# ---- 6. two host threads on two streams ----------------------------------------------------------------------------------------
def test_two_threads_two_streams(dev):
    from cim_amd import prm
    rng = np.random.RandomState(4)
    crms = [(rng.randn(2, 6, 5, 7) * 12).astype(np.float32) for _ in range(2)]
    labels = [[[1, 4], [0, 2, 5]], [[3], [5, 1]]]
    wants = []
    for k in range(2):
        w = []
        for i in range(2):
            up = prm_np.upsample(crms[k][i][None], [(0, c) for c in labels[k][i]], FACTOR)
            w.append(prm_np.image_points(list(up), labels[k][i], 40, 56, prm_cases.THRESHOLD))
        wants.append(w)
    devs = [torch.from_numpy(c).to(dev) for c in crms]
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(20):
                    res, run = prm.peaks_from_crm(devs[k], labels[k], FACTOR, details=True)
                    for i in range(2):
                        np.testing.assert_array_equal(res[i][2], wants[k][i]["classes"])
                        np.testing.assert_array_equal(run.ys_xs[i][0], wants[k][i]["ys"])
                        np.testing.assert_array_equal(run.ys_xs[i][1], wants[k][i]["xs"])
                        np.testing.assert_array_equal(bits(res[i][3]), bits(wants[k][i]["scores"]))
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from cim_amd import _lib, prm
    crm = torch.zeros((2, 3, 2, 3), device=dev)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.peaks_from_crm(crm.cpu(), [[0], [1]])
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.upsample(crm.cpu(), [[0], [1]], 8)
    with pytest.raises(_lib.CimHipError, match="factor"):
        prm.upsample(crm, [[0], [1]], 0)
    with pytest.raises(ValueError, match="class 3, outside 0..2"):
        prm.peaks_from_crm(crm, [[0], [3]])
    with pytest.raises(ValueError, match="no .image, class. pair"):
        prm.peaks_from_crm(crm, [[], []])
    with pytest.raises(ValueError, match="at most"):
        prm.peaks_from_crm(torch.zeros((1, 1, 300, 300), device=dev), [[0]], factor=8)
    with pytest.raises(_lib.CimHipError, match="65535"):
        prm.peaks_from_crm(crm, [[0], [1]], image_sizes=[(10, 10), (70000, 10)])
    with pytest.raises(ValueError, match="2 maps for 3"):
        prm.peaks_from_maps(torch.zeros((2, 4, 4), device=dev), [[0, 1], [2]])
