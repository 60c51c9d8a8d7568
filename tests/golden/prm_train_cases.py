"""Inputs shared by make_golden_prm_train.py (which feeds them to the reference) and the PRM training tests (which feed them to
the restatement and the device).  The maps at factor 1 hold small dyadic values: every sum of them is exact in fp32, so the
reference's results do not depend on its summation order."""
import collections

import numpy as np

f32 = np.float32
SHAPES = ((5, 7), (15, 21), (24, 40))           # 35 pixels: less than a wave | 315: no multiple of 64 or 256 | 960
MAP_NAMES = ("constant", "plateau", "signed_zeros", "equal_maxima", "checkerboard", "corners_edges", "neg_inf", "one_nan",
             "seeded_ties", "seeded_fine")
BATCH, CLASSES = 2, 5                           # the ten maps of a shape as one [2, 5, H, W] call
# up-sampling forms: (h, w, factor)
UPSAMPLE_FORMS = ((3, 5, 8), (5, 7, 3), (1, 1, 8), (1, 4, 2))
# (h, w, factor) whose scales (n - 1) / (factor n - 1) are dyadic: the fp32 tap weights are exact, ATen's float64 ones are the same
DYADIC_FORMS = ((3, 3, 3), (3, 3, 11), (1, 3, 3), (4, 6, 1))


def crafted(shape):
    """name -> [H,W] f32 for one of SHAPES."""
    h, w = shape
    rng = np.random.RandomState(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    maps = collections.OrderedDict()
    maps["constant"] = np.full(shape, 3.5)                                                  # exactly one peak, at (0, 0)
    plateau = np.ones(shape)
    plateau[1:h - 1, 2:w - 1] = 2.0                                                         # two levels: the plateau's first pixel
    maps["plateau"] = plateau
    zeros = np.where((yy + xx) % 2 == 0, 0.0, -0.0)
    zeros[h // 2, w // 2] = -1.0
    maps["signed_zeros"] = zeros                                                            # -0.0 == +0.0: one peak, at (0, 0)
    eq = np.zeros(shape)
    eq[1, 1] = eq[1, 2] = 4.0                                                               # side by side: the left one
    eq[h - 3, w - 2] = eq[h - 2, w - 2] = 6.0                                               # one above the other: the upper one
    eq[h - 1, 0] = 4.0
    maps["equal_maxima"] = eq
    maps["checkerboard"] = np.where((yy % 2 == 0) & (xx % 2 == 0), 2.0 + ((yy // 2 + xx // 2) % 4) * 0.25, 1.0)   # a quarter are peaks
    ce = np.zeros(shape)
    for y, x, v in ((0, 0, 5), (0, w - 1, 6), (h - 1, 0, 7), (h - 1, w - 1, 8), (0, w // 2, 1.5), (h - 1, w // 2, 2.5),
                    (h // 2, 0, 3.25), (h // 2, w - 1, 4.75)):
        ce[y, x] = v
    maps["corners_edges"] = ce
    maps["neg_inf"] = np.full(shape, -np.inf)
    nan = rng.randint(-8, 9, shape) / 4.0
    nan[h // 2, w // 3] = np.nan
    maps["one_nan"] = nan
    maps["seeded_ties"] = rng.randint(0, 6, shape).astype(np.float64)                       # many equal neighbours
    maps["seeded_fine"] = rng.randint(-2048, 2049, shape) / 64.0
    assert tuple(maps) == MAP_NAMES
    return collections.OrderedDict((k, np.asarray(v, dtype=f32)) for k, v in maps.items())


def crafted_batch(shape):
    """The ten maps of `shape` as [BATCH, CLASSES, H, W] f32, in the order of MAP_NAMES."""
    return np.stack(list(crafted(shape).values())).reshape((BATCH, CLASSES) + tuple(shape))


def grad_output(shape):
    """A seeded dyadic gradient of the aggregation [BATCH, CLASSES] for the maps of `shape`."""
    rng = np.random.RandomState(7 + shape[0])
    return (rng.randint(-64, 65, (BATCH, CLASSES)) / 16.0).astype(f32)


def seeded_crm(h, w, b, c, seed):
    """Smooth-ish class response maps away from dyadic values (the up-sampling forms)."""
    rng = np.random.RandomState(seed)
    return (rng.randn(b, c, h, w) * 6.0).astype(f32)


def loss_cases():
    """name -> (x [B,C] f32, target [B,C] f32)."""
    rng = np.random.RandomState(5)
    cases = collections.OrderedDict()
    cases["one"] = (np.array([[0.75]], dtype=f32), np.array([[1.0]], dtype=f32))            # B C = 1
    x = (rng.randn(3, 20) * 4.0).astype(f32)
    x[0, :6] = [100.0, -100.0, 0.0, -0.0, 100.0, -100.0]                                   # +-100 and 0 among ordinary values
    x[1, :4] = [87.5, -80.0, 80.0, 1e-3]
    cases["zeros"] = (x, np.zeros((3, 20), dtype=f32))
    cases["ones"] = (x, np.ones((3, 20), dtype=f32))
    cases["hard"] = (x, (rng.rand(3, 20) < 0.3).astype(f32))
    cases["soft"] = (x, rng.uniform(0.01, 0.99, (3, 20)).astype(f32))
    return cases
