"""NumPy restatement of Pillow's antialiased resize, Image.resize((ow, oh), Image.BILINEAR) on 3-channel uint8 images
(src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc), the
arithmetic csrc/resample.hip repeats on the device.  Pillow itself is the arbiter: tests/test_resample_cpu.py
compares the two bit for bit.

Per axis the coefficient table is computed in IEEE double - no fused multiply-add, the sum of a row's weights taken in index
order - and rounded to 22-bit fixed point; a pass is integer arithmetic on bytes.  Horizontal pass first into a uint8
intermediate, then the vertical pass; an axis whose size does not change is skipped.  Pillow 12.2.0 runs the vertical pass first
when the source has h > 100 w (probed, not documented): `resize` refuses those shapes, as the device path does."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2
MAX_ASPECT = 100                    # h <= MAX_ASPECT * w: the horizontal pass comes first


def ksize(n_in, n_out):
    """Length of one row of the coefficient table."""
    support = 1.0 * max(float(n_in) / float(n_out), 1.0)
    return int(np.ceil(support)) * 2 + 1


def coeffs(n_in, n_out):
    """-> bounds [n_out, 2] int32 = (xmin, n), kk [n_out, ksize] int32 (entries from n on are 0)."""
    n_in, n_out = int(n_in), int(n_out)
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = np.float64(1.0) * fs
    ks = int(np.ceil(support)) * 2 + 1
    ss = np.float64(1.0) / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                # astype: C truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = xmax - xmin
    x = np.arange(ks, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (x < n[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for j in range(ks):                                                            # the sum in index order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    fixed = np.where(w < 0.0, -0.5 + w * float(1 << PRECISION_BITS), 0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    fixed = np.where(x < n[:, None], fixed, 0)
    return np.stack([xmin, n], axis=1).astype(np.int32), fixed.astype(np.int32)


def _pass(img, bounds, kk):
    """One pass along axis 1 of img [rows, n_in, ch] uint8 -> [rows, n_out, ch] uint8."""
    src = img.astype(np.int32)
    out = np.empty((img.shape[0], bounds.shape[0], img.shape[2]), dtype=np.uint8)
    for xx in range(bounds.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        s = np.int32(1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, x0:x0 + n, :], kk[xx, :n], axes=([1], [0]))
        out[:, xx, :] = np.clip(s >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, out_w, out_h):
    """img [h, w, 3] uint8 -> [out_h, out_w, 3] uint8: np.asarray(Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR))."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    if h > MAX_ASPECT * w:
        raise ValueError("pil_resample_np.resize: %d x %d has h > %d w: Pillow runs the vertical pass first there" % (h, w, MAX_ASPECT))
    if w != out_w:
        img = _pass(img, *coeffs(w, out_w))
    if h != out_h:
        img = _pass(img.transpose(1, 0, 2), *coeffs(h, out_h)).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


# (h, w) -> (out_w, out_h): the fixed cases of the CPU and the GPU tests
CASES = [((1, 1), (5, 4)), ((1, 7), (448, 448)), ((7, 1), (448, 448)), ((2, 3), (7, 5)), ((37, 53), (448, 448)),
         ((375, 500), (448, 448)), ((500, 375), (448, 448)), ((448, 500), (448, 448)), ((333, 448), (448, 448)),
         ((448, 448), (448, 448)), ((449, 447), (448, 448)), ((1000, 1300), (448, 448)), ((640, 480), (7, 5)),
         ((300, 3), (448, 448)), ((61, 3000), (448, 448))]
TABLE_CASES = [(500, 448), (375, 448), (1, 448), (3000, 7), (449, 448)]
CONTENTS = ("random", "extremes", "white")


def content(kind, h, w, seed):
    """The three contents of every case: random bytes, only {0, 255}, constant 255."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "extremes":
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return np.full((h, w, 3), 255, dtype=np.uint8)


def seeded_shapes(count=100, seed=20):
    """`count` seeded ((h, w), (out_w, out_h)): sides 1..700, outputs 448 x 448 or random 1..600, all with h <= 100 w."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        h, w = int(rng.randint(1, 701)), int(rng.randint(1, 701))
        size = (448, 448) if rng.randint(2) else (int(rng.randint(1, 601)), int(rng.randint(1, 601)))
        if h <= MAX_ASPECT * w:
            out.append(((h, w), size))
    return out
