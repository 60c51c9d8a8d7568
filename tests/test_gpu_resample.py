"""-m gpu: cim_amd.resample (csrc/resample.hip) - Pillow's antialiased resize on the device.  Every comparison
is exact: the uint8 output and the coefficient tables against the NumPy restatement (tests/golden/pil_resample_np.py, itself
checked against Pillow in tests/test_resample_cpu.py), the fp32 output against `prm.network_input` of the restatement's bytes,
a ragged batch against each image alone, `label_assign(resize="device")` against `resize="pillow"`, two host threads on two
streams, the refusals."""
import ctypes
import functools
import os
import threading
import zlib

import numpy as np
import pytest
import torch

import pil_resample_np as prn
import prm_cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(hw, size):
    """The three contents of a case and the restatement's result for each: computed once, shared, never written to."""
    seed = zlib.crc32(repr((hw, size)).encode()) % (1 << 31)
    images = [prn.content(kind, hw[0], hw[1], seed) for kind in prn.CONTENTS]
    wants = [prn.resize(im, size[0], size[1]) for im in images]
    for a in images + wants:
        a.setflags(write=False)
    return images, wants


IDS = ["%dx%d_to_%dx%d" % (c[0] + c[1]) for c in prn.CASES]


# ---- 1. the bytes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,size", prn.CASES, ids=IDS)
def test_uint8_output_equals_restatement(dev, hw, size):
    from cim_amd import resample
    images, wants = case(hw, size)
    for kind, im, want in zip(prn.CONTENTS, images, wants):
        got = resample.pil_resize(im, size)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, size[1], size[0], 3) and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy()[0], want, err_msg=kind)
    if hw == (448, 448):
        np.testing.assert_array_equal(wants[0], images[0])                             # the copy


def test_device_tensors_and_one_stacked_tensor_are_taken(dev):
    from cim_amd import resample
    images, wants = case((37, 53), (448, 448))
    got = resample.pil_resize([torch.from_numpy(im.copy()).to(dev) for im in images], 448)
    np.testing.assert_array_equal(got.cpu().numpy(), np.stack(wants))
    got = resample.pil_resize(torch.from_numpy(np.stack(images)).to(dev), (448, 448))
    np.testing.assert_array_equal(got.cpu().numpy(), np.stack(wants))


# ---- 2. the tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", prn.TABLE_CASES)
def test_tables_equal_restatement(dev, n_in, n_out):
    """Both axes at once: the widths take n_in -> n_out, the heights the same."""
    from cim_amd import resample
    (bx, cx, by, cy), = resample.tables([(n_in, n_in)], (n_out, n_out))
    bounds, kk = prn.coeffs(n_in, n_out)
    assert cx.dtype == np.int32 and cx.shape == kk.shape
    for got_b, got_k in ((bx, cx), (by, cy)):
        np.testing.assert_array_equal(got_b, bounds)
        np.testing.assert_array_equal(got_k, kk)


def test_tables_of_a_ragged_batch_share_the_longest_row(dev):
    from cim_amd import resample
    sizes = [(375, 500), (1000, 1300), (37, 53)]
    got = resample.tables(sizes, (448, 448))
    for (h, w), (bx, cx, by, cy) in zip(sizes, got):
        for n_in, b, k in ((w, bx, cx), (h, by, cy)):
            bounds, kk = prn.coeffs(n_in, 448)
            np.testing.assert_array_equal(b, bounds)
            np.testing.assert_array_equal(k, kk)


# ---- 3. the fp32 planes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(375, 500), (37, 53), (448, 448)])
def test_fp32_output_is_network_input_of_the_restatement_bytes(dev, hw):
    from cim_amd import prm
    images, wants = case(hw, (448, 448))
    got = prm.network_input_from_images(images)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 448, 448)
    want = prm.network_input(np.stack(wants))
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(prm_cases.normalise(np.stack(wants))))


def test_other_size_and_other_statistics(dev):
    from cim_amd import resample
    images, wants = case((640, 480), (7, 5))
    mean, std = (0.1, 0.5, 0.9), (0.3, 1.0, 2.5)
    got = resample.pil_resize(images[0], (7, 5), normalize=(mean, std)).cpu().numpy()
    x = wants[0].astype(np.float32) / np.float32(255.0)
    want = np.moveaxis(((x - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32)).astype(np.float32), -1, 0)
    assert got.shape == (1, 3, 5, 7)
    np.testing.assert_array_equal(bits(got[0]), bits(want))


# ---- 4. a ragged batch --------------------------------------------------------------------------------------------------------
def test_ragged_batch_equals_each_alone(dev):
    from cim_amd import prm, resample
    shapes = [(375, 500), (37, 53), (1000, 1300), (448, 448), (300, 3)]
    images = [case(hw, (448, 448))[0][0] for hw in shapes]
    wants = [case(hw, (448, 448))[1][0] for hw in shapes]
    got = resample.pil_resize(images, (448, 448))
    assert tuple(got.shape) == (5, 448, 448, 3)
    for i in range(5):
        np.testing.assert_array_equal(got[i].cpu().numpy(), wants[i], err_msg=str(shapes[i]))
        np.testing.assert_array_equal(got[i].cpu().numpy(), resample.pil_resize(images[i], 448)[0].cpu().numpy())
    x = prm.network_input_from_images(images)
    for i in range(5):
        assert torch.equal(x[i], prm.network_input_from_images(images[i])[0])


# ---- 5. label_assign ----------------------------------------------------------------------------------------------------------
def seeded_masks(seed, n, h, w):
    rng = np.random.RandomState(seed)
    masks = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        y0, x0 = rng.randint(0, h - 8), rng.randint(0, w - 8)
        y1, x1 = rng.randint(y0 + 4, h + 1), rng.randint(x0 + 4, w + 1)
        masks[i, y0:y1, x0:x1] = rng.rand(y1 - y0, x1 - x0) < 0.9
        masks[i, y0, x0] = True
    return masks


def test_label_assign_device_resize_equals_pillow_resize(dev):
    from PIL import Image

    from cim_amd import prm, resample
    from cim_amd import proposal_prep as pp
    d = np.load(os.path.join(GOLDEN, "prm_e2e.npz"))
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, int(d["seed"]), float(d["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model = model.to(dev)
    images = [prm_cases.seeded_images(31, 1, 375, 500)[0], prm_cases.seeded_images(32, 1, 500, 333)[0]]
    labels = [[2, 9, 14], [5]]
    masks = [torch.from_numpy(seeded_masks(41 + i, 12, *im.shape[:2])).to(dev) for i, im in enumerate(images)]
    # the resized bytes feeding both settings
    resized = np.stack([np.asarray(Image.fromarray(im).resize((448, 448), Image.BILINEAR)) for im in images])
    np.testing.assert_array_equal(resample.pil_resize(images, (448, 448)).cpu().numpy(), resized)
    np.testing.assert_array_equal(bits(prm.network_input_from_images(images).cpu().numpy()),
                                  bits(prm.network_input(resized).cpu().numpy()))
    on_device = pp.label_assign(model, images, labels, masks)                           # the default is the device path
    explicit = pp.label_assign(model, images, labels, masks, resize="device")
    on_host = pp.label_assign(model, images, labels, masks, resize="pillow")
    for i in range(2):
        assert tuple(on_device[i].shape) == (12, 21)
        np.testing.assert_array_equal(on_device[i].cpu().numpy(), on_host[i].cpu().numpy())
        np.testing.assert_array_equal(explicit[i].cpu().numpy(), on_host[i].cpu().numpy())
    print("cluster entries per image:", [int((m[:, 1:] != 0).sum()) for m in on_host])
    with pytest.raises(ValueError, match="'device' or 'pillow'"):
        pp.label_assign(model, images, labels, masks, resize="host")


# ---- 6. two host threads on two streams ---------------------------------------------------------------------------------------
def test_two_threads_two_streams(dev):
    from cim_amd import resample
    work = [[case((37, 53), (448, 448)), case((2, 3), (7, 5))], [case((61, 3000), (448, 448)), case((1, 1), (5, 4))]]
    sizes = [[(448, 448), (7, 5)], [(448, 448), (5, 4)]]
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(10):
                    for (images, wants), size in zip(work[k], sizes[k]):
                        got = resample.pil_resize(images, size)
                        np.testing.assert_array_equal(got.cpu().numpy(), np.stack(wants))
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
    from cim_amd import _lib, resample
    ok = np.zeros((4, 5, 3), dtype=np.uint8)
    resample.pil_resize(np.zeros((300, 3, 3), dtype=np.uint8), 4)                      # the allowed aspect limit
    with pytest.raises(_lib.CimHipError, match="h > 100 w"):
        resample.pil_resize(np.zeros((301, 3, 3), dtype=np.uint8), 4)
    with pytest.raises(_lib.CimHipError, match="h > 100 w"):
        resample.pil_resize([ok, np.zeros((301, 3, 3), dtype=np.uint8)], 4)            # anywhere in the batch
    for bad in (np.zeros((0, 5, 3), dtype=np.uint8), np.zeros((5, 0, 3), dtype=np.uint8)):
        with pytest.raises(_lib.CimHipError, match="sides must be 1..16384"):
            resample.pil_resize(bad, 4)
    for size in ((0, 4), (4, 0), (4097, 4)):
        with pytest.raises(_lib.CimHipError, match="sides must be 1..4096"):
            resample.pil_resize(ok, size)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        resample.pil_resize(torch.from_numpy(ok), 4)
    with pytest.raises(ValueError, match="no image"):
        resample.pil_resize([], 4)
    with pytest.raises(ValueError, match="uint8"):
        resample.pil_resize(ok.astype(np.float32), 4)
    # at the C ABI: both destinations NULL, descending offsets, B < 1
    run = resample._Batch([(4, 5), (4, 5)], 4, 4, dev, "test")
    src = torch.zeros(run.nbytes, dtype=torch.uint8, device=dev)
    out = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=dev)
    args = lambda desc, b, dst: (src.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), run.desc_dev.data_ptr(), b, 4, 4, dst, None, None,
                                 run.ws.data_ptr(), _lib.stream_ptr())
    _lib.call("cim_resample_rgb", *args(run.desc_host, 2, out.data_ptr()))
    with pytest.raises(_lib.CimHipError, match="both destinations are NULL"):
        _lib.call("cim_resample_rgb", *args(run.desc_host, 2, None))
    overlap = run.desc_host.copy()
    overlap[3] = 59                                                                    # image 1 starts inside image 0 (60 bytes)
    with pytest.raises(_lib.CimHipError, match="offsets must ascend"):
        _lib.call("cim_resample_rgb", *args(overlap, 2, out.data_ptr()))
    with pytest.raises(_lib.CimHipError, match="B = 0"):
        _lib.call("cim_resample_rgb", *args(run.desc_host, 0, out.data_ptr()))
    assert _lib.call("cim_resample_ws_bytes", 2, overlap.ctypes.data_as(ctypes.c_void_p), 4, 4) == -1
    torch.cuda.synchronize()
