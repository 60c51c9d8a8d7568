"""-m gpu: cim_image_prep (cim_amd/csrc/image_prep.hip) straight at the C ABI on the smallest sources: one pixel, one row, one
column, 2 x 2, and the scales that enlarge them eightfold or shrink them to one pixel.  The reference is
oracle.image_prep.prep_image; results are bit-identical.

  - w = 1: every output column takes the kernel's `edge` branch; h = 1: both source rows are row 0.
  - hflip: the second neighbour is the pixel to the LEFT (xb = xa - 1).  The "ends" source has columns 0 = 0 and w - 1 = 255 (rows
    likewise), so a neighbour taken from the wrong side changes the values next to either border.
  - The source lies inside a uint8 buffer whose bytes before it hold the complement of the first pixel and whose bytes after it
    the complement of the last one (pixel values stay out of 96 .. 159, so a complement is at least 64 away): a read outside the
    image changes a result.
  - dst is a sentinel buffer with row_stride = W + 3 and plane_stride = (H + 2) row_stride: everything in [3][H][W] must be
    written, everything else untouched."""
import ctypes

import numpy as np
import pytest
import torch

from abi_guards import GUARD, SENT, _poisoned_u8      # tests/golden/abi_guards.py

pytestmark = pytest.mark.gpu

SOURCES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 3)]
SCALES = [1, 4, 7.3, 0.5, 0.2]
# SOURCES x SCALES, less the combinations of which a side rounds (half to even, as the oracle and cv2 round) to 0:
# at 0.5 the sides 1 (0.5 -> 0), at 0.2 the sides 1 and 2 (0.2, 0.4 -> 0)
CASES = [((1, 1), 1), ((1, 1), 4), ((1, 1), 7.3),
         ((1, 9), 1), ((1, 9), 4), ((1, 9), 7.3),
         ((9, 1), 1), ((9, 1), 4), ((9, 1), 7.3),
         ((2, 2), 1), ((2, 2), 4), ((2, 2), 7.3), ((2, 2), 0.5),
         ((3, 5), 1), ((3, 5), 4), ((3, 5), 7.3), ((3, 5), 0.5), ((3, 5), 0.2),
         ((5, 3), 1), ((5, 3), 4), ((5, 3), 7.3), ((5, 3), 0.5), ((5, 3), 0.2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _mean_std():
    from oracle import image_prep as ip
    return (ctypes.c_float * 6)(*ip.MEAN, *ip.STD)


def _images(h, w):
    """-> [(name, uint8 [h, w, 3])]: random bytes outside 96 .. 159, and the same with the border rows / columns at 0 and 255"""
    rng = np.random.RandomState(16 * h + w)
    v = rng.randint(0, 192, size=(h, w, 3))
    rand = np.where(v < 96, v, v + 64).astype(np.uint8)
    ends = rand.copy()
    ends[0], ends[-1] = 0, 255
    ends[:, 0], ends[:, -1] = 0, 255
    return [("random", rand), ("ends", ends)]


def _source(dev, im):
    """im inside the complement of its first pixel (before) and of its last pixel (after)"""
    flat = torch.from_numpy(im.reshape(-1)).to(dev)
    return _poisoned_u8(flat, front=~flat[:3], back=~flat[-3:])


class _Dst:
    """[3][H][W] floats with row_stride = W + 3, plane_stride = (H + 2) row_stride between 64 sentinel floats"""

    def __init__(self, dev, H, W):
        self.H, self.W, self.rs = H, W, W + 3
        self.ps = (H + 2) * self.rs
        self.raw = torch.full((GUARD + 3 * self.ps + GUARD,), SENT, dtype=torch.int32, device=dev)
        self.ptr = self.raw.data_ptr() + 4 * GUARD

    def _inside(self, raw):
        return raw[GUARD:GUARD + 3 * self.ps].view(3, self.H + 2, self.rs)[:, :self.H, :self.W]

    def untouched(self):
        return bool((self.raw == SENT).all())

    def check(self):
        got = self._inside(self.raw).clone()
        left = int((got == SENT).sum())
        assert left == 0, "%d of [3][H][W] were not written, the first at %s" % (left, (got == SENT).nonzero()[0].tolist())
        rest = self.raw.clone()
        self._inside(rest).fill_(SENT)
        assert bool((rest == SENT).all()), "a store outside [3][H][W]: %d floats changed" % int((rest != SENT).sum())
        return got.cpu().numpy().view(np.float32)


def test_case_list_is_the_products_with_both_sides_at_least_one():
    want = [(s, k) for s in SOURCES for k in SCALES if int(np.round(s[0] * k)) >= 1 and int(np.round(s[1] * k)) >= 1]
    assert CASES == want and len(CASES) == 23


@pytest.mark.parametrize("hw,im_scale", CASES)
def test_image_prep_equals_the_oracle_on_tiny_sources(dev, hw, im_scale):
    from cim_amd import _lib
    from oracle import image_prep as ip
    ms = _mean_std()
    h, w = hw
    H, W = int(np.round(h * im_scale)), int(np.round(w * im_scale))
    for name, im in _images(h, w):
        src = _source(dev, im)
        for hflip in (0, 1):
            ref = ip.prep_image(im, im_scale, hflip=bool(hflip))
            assert ref.shape == (3, H, W)
            dst = _Dst(dev, H, W)
            _lib.call("cim_image_prep", src.data_ptr(), h, w, dst.ptr, H, W, dst.ps, dst.rs, 1.0 / float(im_scale), hflip,
                      ctypes.cast(ms, ctypes.c_void_p), _lib.stream_ptr())
            torch.cuda.synchronize()
            got = dst.check()
            bad = got.view(np.int32) != ref.view(np.int32)
            assert not bad.any(), "%s, hflip = %d: %d of %d differ, first at %s: got %r, want %r" % (
                name, hflip, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])],
                ref[tuple(np.argwhere(bad)[0])])


def test_image_prep_refusals(dev):
    from cim_amd import _lib
    ms = ctypes.cast(_mean_std(), ctypes.c_void_p)
    im = _images(3, 5)[0][1]
    src = _source(dev, im)
    dst = _Dst(dev, 3, 5)
    s = _lib.stream_ptr()
    ok = (src.data_ptr(), 3, 5, dst.ptr, 3, 5, dst.ps, dst.rs, 1.0, 0, ms)
    for at, value in ((7, 4),                                            # row_stride < W
                      (8, 0.0), (8, -1.0),                               # inv_scale <= 0
                      (0, None), (3, None), (10, None),                  # null pointers
                      (1, 0), (2, 0), (4, 0), (5, 0)):
        args = list(ok)
        args[at] = value
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_image_prep", *args, s)
    torch.cuda.synchronize()
    assert dst.untouched()
