"""Inputs shared by make_golden_prm.py (which feeds them to the reference) and the PRM tests (which feed them to the restatement
and the device): the seeded weights of the thin network - regenerated on both sides, never stored - and the crafted exact maps
on which no float arithmetic precedes a decision."""
import collections

import numpy as np

WIDTH = 16                  # of the thin ResNet-50 body (64 = the real one)
NUM_CLASSES = 20
THRESHOLD = 10
NET_SHAPE = (64, 96)        # network case: CRM 2 x 3, up-sampled 16 x 24
f32 = np.float32


def seeded_weights(shapes, seed, cls_gain):
    """shapes: ordered {state_dict key: shape} -> {key: float32 / int64 array}, one RandomState walked in key order.  BatchNorm
    statistics and affine parameters away from the identity; the classifier scaled by `cls_gain` so that some response maps
    pass the peak threshold and some do not."""
    rng = np.random.RandomState(seed)
    out = collections.OrderedDict()
    for key, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[key] = np.array(100, dtype=np.int64)
        elif ".classifier." in key:
            if leaf == "weight":
                out[key] = (rng.randn(*shape) * cls_gain / np.sqrt(shape[1])).astype(f32)
            else:
                out[key] = (rng.randn(*shape) * 2.0).astype(f32)
        elif len(shape) == 4:                                              # a convolution
            fan_in = shape[1] * shape[2] * shape[3]
            out[key] = (rng.randn(*shape) * np.sqrt(2.0 / fan_in)).astype(f32)
        elif leaf == "running_var":
            out[key] = rng.uniform(0.5, 1.5, shape).astype(f32)
        elif leaf == "weight":                                             # BatchNorm gamma
            out[key] = rng.uniform(0.6, 1.4, shape).astype(f32)
        else:                                                              # BatchNorm beta, running_mean
            out[key] = (rng.randn(*shape) * 0.1).astype(f32)
    return out


def seeded_images(seed, count, height, width):
    """Smooth RGB uint8 images [count, height, width, 3] (sums of a few seeded blobs: a random image gives a flat response)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    out = np.empty((count, height, width, 3), dtype=np.uint8)
    for i in range(count):
        img = np.zeros((height, width, 3))
        for _ in range(6):
            cy, cx = rng.uniform(0, height), rng.uniform(0, width)
            s = rng.uniform(0.08, 0.3) * max(height, width)
            img += rng.uniform(-1, 1, 3)[None, None, :] * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))[:, :, None]
        img = (img - img.min()) / (img.max() - img.min() + 1e-9)
        out[i] = np.clip(np.round(img * 255.0 + rng.uniform(-6, 6, img.shape)), 0, 255).astype(np.uint8)
    return out


def normalise(rgb_u8):
    """ToTensor + Normalize of prm_configs.open_transform in fp32: [..., H, W, 3] uint8 -> [..., 3, H, W]."""
    mean = np.array([0.485, 0.456, 0.406], dtype=f32)
    std = np.array([0.229, 0.224, 0.225], dtype=f32)
    x = rgb_u8.astype(f32) / f32(255.0)
    x = ((x - mean) / std).astype(f32)
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


def _case(maps, labels, threshold=THRESHOLD):
    """One image: maps {class: [H,W] f32}, labels = the classes in the order they are processed."""
    return {"maps": {c: np.asarray(m, dtype=f32) for c, m in maps.items()}, "labels": list(labels), "threshold": threshold}


def crafted():
    """name -> case.  Every value is exact in fp32."""
    rng = np.random.RandomState(7)
    cases = collections.OrderedDict()
    cases["constant"] = _case({0: np.full((4, 5), 12.0)}, [0])                          # the single peak (0, 0)
    cases["plateau"] = _case({0: [[1, 2, 2, 1], [0, 2, 2, 0], [0, 0, 0, 0]]}, [0])        # peak (0, 1), below 10: the fallback
    cases["one_pixel"] = _case({0: [[11.0]]}, [0])
    cases["row"] = _case({0: [[3, 12, 5, 5, 14, 14, 2]]}, [0])
    cases["column"] = _case({0: [[15], [2], [2], [11], [13], [4]]}, [0])
    cases["odd"] = _case({0: rng.randint(0, 30, (3, 5))}, [0])
    z = np.array([[0.0, -0.0, -1.0, np.inf], [-0.0, 0.0, -2.0, 5.0], [-3.0, -0.0, 0.0, -0.0]], dtype=f32)
    cases["zeros_inf"] = _case({0: z}, [0])
    cases["signed_zero_peaks"] = _case({0: np.array([[-0.0, -1, 0.0, -1, -0.0], [-1, -1, -1, -1, -1]], dtype=f32)}, [0])
    above = np.nextafter(f32(10.0), f32(11.0))
    cases["at_threshold"] = _case({0: [[10.0, 1, above, 1, 9.5], [1, 1, 1, 1, 1], [10.0, 1, 1, 1, 1]]}, [0])
    cases["none_above"] = _case({0: [[4, 1, 7, 1, 7], [1, 1, 1, 1, 1], [5, 1, 7, 1, 3]]}, [0])   # the FIRST of the largest: (0, 2)
    a, b = rng.randint(0, 40, (5, 6)), rng.randint(0, 40, (5, 6))
    cases["two_pairs_out_of_order"] = _case({3: a, 1: b, 0: np.zeros((5, 6)), 2: np.zeros((5, 6))}, [3, 1])
    many = np.zeros((1, 2 * 257 - 1), dtype=f32)
    many[0, ::2] = 20 + np.arange(257)
    cases["many_257"] = _case({0: many}, [0])
    return cases


def duplicates_map(seed=11, shape=(320, 416)):
    """Many duplicates, drawn so that every radix pass of the median splits: values dense around +-1 (the low bytes differ),
    a few other magnitudes and signs (the high bytes differ)."""
    rng = np.random.RandomState(seed)
    fine = (f32(1.0) + rng.randint(0, 70000, 4000).astype(f32) * f32(2.0 ** -23)).astype(f32)
    pool = np.concatenate([fine, -fine[:1500], np.array([0.0, -0.0, 3.5, -7.25, 1e-3, 2e4, np.inf], dtype=f32)])
    return pool[rng.randint(0, pool.size, shape)].astype(f32)
