"""NumPy restatement, in float64, of the 7 x 7 stem convolution's weight gradient (csrc/conv7x7_dw.hip):

    dw[co][ci][ky][kx] = sum over b, oy, ox of dconv[b][co][oy][ox] * x[b][ci][oy s + ky - 3][ox s + kx - 3]

with zero padding 3 and stride s, and beside it the sum of the terms' magnitudes - what a floating-point summation's error is
measured in.  One einsum per tap over the strided window of the padded input: no im2col, no torch."""
import numpy as np

# (B, cin, cout, H, W, stride): the shapes the issue lists ...
SHAPES = [
    (1, 1, 1, 1, 1, 1),
    (1, 3, 4, 7, 9, 1),
    (1, 3, 64, 8, 8, 2),           # even side: the last taps fall into the padding
    (2, 3, 16, 13, 17, 2),
    (2, 4, 64, 31, 45, 1),
    (2, 3, 64, 75, 100, 2),
    # ... and the boundaries of the kernel's tiling (4 x 32 output pixels per tile, 64 output channels per workgroup and 16 per
    # wave, at most 768 splits) that they do not cross:
    (1, 2, 80, 9, 70, 2),          # cout 80: a second 64-channel workgroup row whose last three waves idle; Ho x Wo = 5 x 35: a second row strip and column tile
    (1, 3, 20, 34, 40, 1),         # cout 20: a wave tile of 4 of its 16 rows and two idle waves; stride 1 with a second column tile
    (7, 3, 8, 129, 70, 2),         # Ho x Wo = 65 x 35: 17 x 2 tiles x 7 images = 238 splits of one tile each: splits > 1 at stride 2
    (4, 1, 8, 112, 200, 1),        # 28 x 7 tiles x 4 images = 784 > 768: two tiles per split (392 splits), splits that span a tile-row change
]


def out_size(n, stride):
    return (n - 1) // stride + 1


def terms(shape):
    b, cin, cout, h, w, s = shape
    return b * out_size(h, s) * out_size(w, s)


def dw_and_abs(dconv, x, stride):
    """dconv [B,cout,Ho,Wo], x [B,cin,H,W] (any real dtype) -> (dw, sum |term|), both [cout,cin,7,7] float64."""
    dconv, x = np.asarray(dconv, dtype=np.float64), np.asarray(x, dtype=np.float64)
    b, cout, ho, wo = dconv.shape
    _, cin, h, w = x.shape
    assert (ho, wo) == (out_size(h, stride), out_size(w, stride)) and x.shape[0] == b
    xp = np.zeros((b, cin, (ho - 1) * stride + 7, (wo - 1) * stride + 7))
    hh, ww = min(h, xp.shape[2] - 3), min(w, xp.shape[3] - 3)
    xp[:, :, 3:3 + hh, 3:3 + ww] = x[:, :, :hh, :ww]
    dw, mag = np.zeros((cout, cin, 7, 7)), np.zeros((cout, cin, 7, 7))
    ad, ax = np.abs(dconv), np.abs(xp)
    for ky in range(7):
        for kx in range(7):
            sl = (slice(None), slice(None), slice(ky, ky + (ho - 1) * stride + 1, stride), slice(kx, kx + (wo - 1) * stride + 1, stride))
            dw[:, :, ky, kx] = np.einsum("bohw,bihw->oi", dconv, xp[sl])
            mag[:, :, ky, kx] = np.einsum("bohw,bihw->oi", ad, ax[sl])
    return dw, mag


def seeded(shape, seed, integers=False):
    """(dconv, x) float32 for a shape: standard normal, or integers in -2..2 (every partial sum then is an integer below 2^24)."""
    b, cin, cout, h, w, s = shape
    rs = np.random.RandomState(seed)
    ds, xs = (b, cout, out_size(h, s), out_size(w, s)), (b, cin, h, w)
    if integers:
        return rs.randint(-2, 3, ds).astype(np.float32), rs.randint(-2, 3, xs).astype(np.float32)
    return rs.standard_normal(ds).astype(np.float32), rs.standard_normal(xs).astype(np.float32)
