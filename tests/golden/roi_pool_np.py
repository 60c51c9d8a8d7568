"""NumPy restatement of RoIPool as csrc/roi_pool.hip computes it (include/cim_hip.h) - every operation of the
geometry rounded to np.float32, one at a time:

    b   = int(roi[0])
    rx1 = x1 * s;  ry1 = y1 * s;  rx2 = (x2 + 1) * s;  ry2 = (y2 + 1) * s;  rw = rx2 - rx1;  rh = ry2 - ry1
    rw <= 0 or rh <= 0:  every output of the ROI 0, every argmax -1
    bw = rw / P;  bh = rh / P
    bin (ph, pw):  x in [floor(pw * bw + rx1), ceil((pw + 1) * bw + rx1)),  y likewise, each bound clamped to [0, W] / [0, H]
    empty bin: 0, argmax -1;  else v = -FLT_MAX, idx = -1, then y ascending, x ascending: a pixel > v replaces both

so ties go to the first pixel in row-major order, NaN is never taken, and a bin of -inf / NaN alone yields -FLT_MAX with -1.
Backward: grad_in[b, c, idx] += dy[k, c, ph, pw] for idx != -1, in float64, with the number of terms and the sum of their
magnitudes beside every element - what a float32 summation in any order is measured in.

Arrays are logical NCHW: feat [B,C,H,W], out / argmax [K,C,P,P], cat [K,2C,P,P], masks [K,P,P]; rois [K,5].  No torch; no
program text of any other code base."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
_INT_TOP = f32(2147483520.0)          # the largest float32 below 2^31: a bound is clamped as a float before it becomes an integer


def _clamp(v, size):
    return min(int(np.fmin(np.fmax(v, f32(0.0)), _INT_TOP)), size)


def geometry(roi, scale, P):
    """(b, rx1, ry1, bw, bh, ok) of one ROI; every value np.float32."""
    s = f32(scale)
    x1, y1, x2, y2 = (f32(v) for v in roi[1:5])
    with np.errstate(all="ignore"):
        rx1, ry1 = x1 * s, y1 * s
        rx2, ry2 = (x2 + f32(1.0)) * s, (y2 + f32(1.0)) * s
        rw, rh = rx2 - rx1, ry2 - ry1
        ok = not (rw <= 0 or rh <= 0)
        bw, bh = rw / f32(P), rh / f32(P)
    assert all(v.dtype == np.float32 for v in (rx1, ry1, bw, bh))
    return int(roi[0]), rx1, ry1, bw, bh, ok


def bins(roi, scale, P, H, W):
    """None for a malformed ROI, else four integer arrays of length P: y_lo, y_hi, x_lo, x_hi."""
    _, rx1, ry1, bw, bh, ok = geometry(roi, scale, P)
    if not ok:
        return None
    with np.errstate(all="ignore"):
        ylo = [_clamp(np.floor(f32(p) * bh + ry1), H) for p in range(P)]
        yhi = [_clamp(np.ceil(f32(p + 1) * bh + ry1), H) for p in range(P)]
        xlo = [_clamp(np.floor(f32(p) * bw + rx1), W) for p in range(P)]
        xhi = [_clamp(np.ceil(f32(p + 1) * bw + rx1), W) for p in range(P)]
    return np.array(ylo), np.array(yhi), np.array(xlo), np.array(xhi)


def forward(feat, rois, P, scale):
    """-> (out float32 [K,C,P,P], argmax int32 [K,C,P,P]).  The scan over a bin's pixels is done for all channels at once: the
    strict > from -FLT_MAX leaves the largest non-NaN pixel above -FLT_MAX at its first position in row-major order (or
    -FLT_MAX and -1 where there is none) - tests/test_roi_pool_cpu.py holds this against the scan written out pixel by pixel."""
    feat = np.asarray(feat, np.float32)
    B, C, H, W = feat.shape
    K = len(rois)
    out = np.zeros((K, C, P, P), np.float32)
    arg = np.full((K, C, P, P), -1, np.int32)
    for k in range(K):
        bn = bins(rois[k], scale, P, H, W)
        if bn is None:
            continue
        ylo, yhi, xlo, xhi = bn
        b = int(rois[k][0])
        for ph in range(P):
            for pw in range(P):
                y0, y1, x0, x1 = ylo[ph], yhi[ph], xlo[pw], xhi[pw]
                if y1 <= y0 or x1 <= x0:
                    continue
                win = feat[b, :, y0:y1, x0:x1].reshape(C, -1)
                w = np.where(np.isnan(win), -np.inf, win)
                m = w.max(axis=1)
                pos = np.argmax(w == m[:, None], axis=1)                 # the first maximum
                at = (y0 + pos // (x1 - x0)) * W + x0 + pos % (x1 - x0)
                taken = m > -FLT_MAX
                out[k, :, ph, pw] = np.where(taken, m, -FLT_MAX)
                arg[k, :, ph, pw] = np.where(taken, at, -1)
    return out, arg


def forward_scan(feat, rois, P, scale):
    """The same, written as the contract words it: one comparison per pixel.  Slow; for small cases."""
    feat = np.asarray(feat, np.float32)
    B, C, H, W = feat.shape
    K = len(rois)
    out = np.zeros((K, C, P, P), np.float32)
    arg = np.full((K, C, P, P), -1, np.int32)
    for k in range(K):
        bn = bins(rois[k], scale, P, H, W)
        if bn is None:
            continue
        ylo, yhi, xlo, xhi = bn
        b = int(rois[k][0])
        for c in range(C):
            for ph in range(P):
                for pw in range(P):
                    if yhi[ph] <= ylo[ph] or xhi[pw] <= xlo[pw]:
                        continue
                    v, idx = f32(-FLT_MAX), -1
                    for y in range(ylo[ph], yhi[ph]):
                        for x in range(xlo[pw], xhi[pw]):
                            if feat[b, c, y, x] > v:
                                v, idx = feat[b, c, y, x], y * W + x
                    out[k, c, ph, pw], arg[k, c, ph, pw] = v, idx
    return out, arg


def _scatter(terms, mags, argmax, rois, shape):
    B, C, H, W = shape
    K = argmax.shape[0]
    grad, mag, n = np.zeros((B, C, H * W)), np.zeros((B, C, H * W)), np.zeros((B, C, H * W), np.int64)
    for k in range(K):
        b = int(rois[k][0])
        for c in range(C):
            idx = argmax[k, c].reshape(-1)
            hit = idx >= 0
            np.add.at(grad[b, c], idx[hit], terms[k, c].reshape(-1)[hit])
            np.add.at(mag[b, c], idx[hit], mags[k, c].reshape(-1)[hit])
            np.add.at(n[b, c], idx[hit], 1)
    return grad.reshape(shape), n.reshape(shape), mag.reshape(shape)


def backward(dy, argmax, rois, shape):
    """-> (grad_in float64 [B,C,H,W], number of terms per element, sum of |term| per element)."""
    dy = np.asarray(dy, np.float64)
    return _scatter(dy, np.abs(dy), argmax, rois, shape)


def maskcat_forward(feat, rois, masks, P, scale):
    """-> (cat float32 [K,2C,P,P] = (v, fl(v * mask)), argmax)."""
    out, arg = forward(feat, rois, P, scale)
    with np.errstate(all="ignore"):
        hi = out * np.asarray(masks, np.float32)[:, None]
    return np.concatenate([out, hi.astype(np.float32)], axis=1), arg


def maskcat_backward(dcat, masks, argmax, rois, shape):
    """The terms are d = dcat_lo + mask * dcat_hi in float64; their magnitudes |dcat_lo| + |mask * dcat_hi|."""
    dcat, m = np.asarray(dcat, np.float64), np.asarray(masks, np.float64)[:, None]
    C = shape[1]
    lo, hi = dcat[:, :C], m * dcat[:, C:]
    return _scatter(lo + hi, np.abs(lo) + np.abs(hi), argmax, rois, shape)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# Case A: B 2, a 7 x 9 map
A_SHAPE = (2, 7, 9)         # B, H, W
A_ROIS = np.array([
    [0, 0, 0, 143, 111],                # the whole map and past its edge
    [0, 16, 16, 47, 47],                # bins smaller than a pixel, overlapping
    [0, -40, -24, 20, 30],              # clipped at 0
    [0, 130, 100, 200, 180],            # at the far corner: four bins of the last pixel at 1/16, beyond the map (all empty) at 1/8
    [0, 50, 40, 30, 60],                # malformed: zeros, argmax -1
    [1, 8, 8, 8, 8],                    # a one-pixel box in image 1
    [1, 0, 0, 15, 15],                  # a whole-cell box in image 1
    [1, 37.5, 21.25, 90.75, 77.5],      # fractional coordinates
], np.float32)
A_CHANNELS = (8, 6)                     # the 16-byte and the scalar path
A_VARIANTS = ((7, 1 / 16.0), (1, 1 / 16.0), (14, 1 / 16.0), (7, 1 / 8.0), (7, 1 / 32.0))        # (P, scale)

# Case B: the real map size, bins of up to about 6 x 7 pixels, several ROI groups in the backward
B_SHAPE = (1, 33, 43)
B_CHANNELS = 64
B_P, B_SCALE = 7, 1 / 16.0


def b_rois():
    """24 seeded boxes on the 33 x 43 map at 1/16: the first covers it all, the rest are 2 to 42 cells wide and some hang over."""
    rs = np.random.RandomState(24)
    _, H, W = B_SHAPE
    x1, y1 = rs.uniform(-30, W * 16 * 0.8, 24), rs.uniform(-30, H * 16 * 0.8, 24)
    rois = np.stack([np.zeros(24), x1, y1, x1 + rs.uniform(32, W * 16, 24), y1 + rs.uniform(32, H * 16, 24)], 1).astype(np.float32)
    rois[0] = (0, 0, 0, W * 16 - 1, H * 16 - 1)
    return rois


def census(rois, scale, P, H, W):
    """(malformed ROIs, empty bins among the others, bins among the others, largest bin in pixels)."""
    bad = empty = total = largest = 0
    for roi in rois:
        bn = bins(roi, scale, P, H, W)
        if bn is None:
            bad += 1
            continue
        ylo, yhi, xlo, xhi = bn
        h, w = np.maximum(yhi - ylo, 0), np.maximum(xhi - xlo, 0)
        area = h[:, None] * w[None, :]
        empty += int((area == 0).sum())
        total += P * P
        largest = max(largest, int(area.max()))
    return bad, empty, total, largest


def seeded_feat(shape, seed, kind):
    """[B,C,H,W] float32.  normal: N(0,1);  ints: integers in [-3, 3] (ties everywhere);  special: normal with a block of -inf
    (image 0, rows 1-2, columns 1-2, even channels), one NaN amid numbers (image 0, channel 0, pixel (4, 5)) and - with a second
    image - a NaN alone in a one-pixel bin (image 1, channel 1, pixel (0, 0))."""
    rs = np.random.RandomState(seed)
    if kind == "ints":
        return rs.randint(-3, 4, shape).astype(np.float32)
    x = rs.standard_normal(shape).astype(np.float32)
    if kind == "special":
        x[0, ::2, 1:3, 1:3] = -np.inf
        x[0, 0, 4, 5] = np.nan
        if shape[0] > 1:
            x[1, 1, 0, 0] = np.nan
    return x
