"""NumPy restatement of the PRM peak path (cim_amd/csrc/prm.hip) - the CPU oracle of cim_amd.prm for the maps
no golden covers (the goldens themselves come from running the reference: make_golden_prm.py).

    upsample      bilinear, align_corners = True, every operation rounded to fp32 (the stated arithmetic, not ATen's)
    lower_median  element (n - 1) // 2 of the ascending order (what torch.median returns)
    pair_peaks    3 x 3 peak test with -inf padding (the first maximum of a window wins), value >= median, row-major order;
                  value > threshold, else the first peak holding the largest peak value
    image_points  the pairs of one image in pair order, ascending by score (stable), scaled to image pixels

Written for clarity from those rules; nothing here is used by the product."""
import numpy as np

MAX_PEAKS = 256
STATUS_TOO_MANY, STATUS_NAN, STATUS_NO_PEAK = 1, 2, 4
f32 = np.float32


def scale(n_in, n_out):
    """(n_in - 1) / (n_out - 1) in double, rounded to fp32; 0 when the output side is 1."""
    return f32(np.float64(n_in - 1) / np.float64(n_out - 1)) if n_out > 1 else f32(0.0)


def _taps(n_in, n_out):
    src = scale(n_in, n_out) * np.arange(n_out).astype(f32)                # fp32 product
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    l0 = f32(1.0) - l1
    return i0, i1, l0.astype(f32), l1.astype(f32)


def upsample(crm, pairs, factor, bias=None):
    """crm [B,C,h,w] f32, pairs [(image, class)] -> up [M, factor h, factor w] f32."""
    crm = np.asarray(crm, dtype=f32)
    _, _, h, w = crm.shape
    y0, y1, l0y, l1y = _taps(h, h * factor)
    x0, x1, l0x, l1x = _taps(w, w * factor)
    out = np.empty((len(pairs), h * factor, w * factor), dtype=f32)
    for m, (b, c) in enumerate(pairs):
        src = crm[b, c]
        if bias is not None:
            src = src + f32(bias[c])                                       # added to every tap before interpolating
        v00, v01 = src[y0][:, x0], src[y0][:, x1]
        v10, v11 = src[y1][:, x0], src[y1][:, x1]
        top = (v00 * l0x[None, :]).astype(f32) + (v01 * l1x[None, :]).astype(f32)
        bot = (v10 * l0x[None, :]).astype(f32) + (v11 * l1x[None, :]).astype(f32)
        out[m] = (top.astype(f32) * l0y[:, None]).astype(f32) + (bot.astype(f32) * l1y[:, None]).astype(f32)
    return out


def lower_median(values):
    a = np.sort(np.asarray(values, dtype=f32).reshape(-1), kind="stable")
    med = a[(a.size - 1) // 2]
    if med == 0 and np.any(np.signbit(a[a == 0])):
        # -0.0 == +0.0 for the sort; the device orders bit patterns (-0.0 first).  Only `value >= median` reads the median, a
        # float compare that does not see the sign; this branch keeps the restatement's BITS those of the device.
        below = int(np.sum(a < 0))
        med = f32(-0.0) if (a.size - 1) // 2 < below + int(np.sum(np.signbit(a[a == 0]))) else f32(0.0)
    return med


def pair_peaks(m, threshold):
    """One map [H,W] f32 -> (median, number of peaks, [(y, x, value)] valid peaks in row-major order, flags)."""
    m = np.asarray(m, dtype=f32)
    h, w = m.shape
    if np.isnan(m).any():
        return f32(np.nan), 0, [], STATUS_NAN
    med = lower_median(m)
    pad = np.full((h + 2, w + 2), -np.inf, dtype=f32)
    pad[1:-1, 1:-1] = m
    peaks = []
    for y in range(h):
        for x in range(w):
            v = m[y, x]
            if not v >= med:
                continue
            win = pad[y:y + 3, x:x + 3].reshape(-1)                        # the window in the pool's scan order; index 4 is the pixel
            if np.all(win[:4] < v) and np.all(win[5:] <= v):               # the first maximum wins
                peaks.append((y, x, v))
    thr = f32(threshold)
    valid = [p for p in peaks if p[2] > thr]
    flags = 0
    if not valid:
        if peaks:
            vals = np.array([p[2] for p in peaks], dtype=f32)
            valid = [peaks[int(np.argmax(vals))]]                          # the first of the largest
        else:
            flags = STATUS_NO_PEAK
    return med, len(peaks), valid, flags


def scale_point(y, img_side, grid):
    return (int(y) * int(img_side)) // int(grid)


def image_points(maps, classes, img_h, img_w, threshold):
    """maps [(H,W)] of ONE image in pair order with their classes -> dict(count, status, rows, cols, classes, ys, xs, scores):
    the pairs' valid peaks concatenated, ordered ascending by score (stable)."""
    entries, status = [], 0
    for m, c in zip(maps, classes):
        _, _, valid, flags = pair_peaks(m, threshold)
        status |= flags
        entries += [(c, y, x, v) for y, x, v in valid]
    count = len(entries)
    if count > MAX_PEAKS:
        status |= STATUS_TOO_MANY
    out = {"count": count, "status": status}
    if status:
        return out
    order = np.argsort(np.array([e[3] for e in entries], dtype=f32), kind="stable") if entries else []
    entries = [entries[i] for i in order]
    grid_h, grid_w = np.asarray(maps[0]).shape if len(maps) else (1, 1)
    out["classes"] = np.array([e[0] for e in entries], dtype=np.int64)
    out["ys"] = np.array([e[1] for e in entries], dtype=np.int64)
    out["xs"] = np.array([e[2] for e in entries], dtype=np.int64)
    out["scores"] = np.array([e[3] for e in entries], dtype=f32)
    out["rows"] = np.array([scale_point(e[1], img_h, grid_h) for e in entries], dtype=np.int64)
    out["cols"] = np.array([scale_point(e[2], img_w, grid_w) for e in entries], dtype=np.int64)
    return out
