"""NumPy restatement of the reference's proposal preprocessing - the CPU oracle of cim_amd.proposal_prep for the sizes no
golden covers (the goldens themselves come from running the reference: make_golden_proposal_prep.py).

    boxes_and_small   tools/pre/generate_7_7_voc.py:35-42 == generate_7_7_coco.py:35-42, with pre_tools.imresize(...,
                      interp='nearest') = PIL.Image.resize(size, 0) restated by `nearest_index`
    assign_clusters   tools/pre/point_level_label_assign.py:58-93 == AGPL_label_assign.py:137-180 (the latter indexes
                      [:, x, y] with x the ROW, see cim_amd.proposal_prep.peaks_to_pixels), lib/utils/mask_utils.py:6-18

Written for clarity, statement by statement; nothing here is used by the product."""
import numpy as np

_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def nearest_index(extent, size):
    """Source index of each of `size` outputs over a crop of `extent` pixels, as Pillow's nearest resize walks them
    (ImagingScaleAffine): step = extent / size in fp64, the first coordinate step * 0.5, each next one the previous plus
    step, truncated.  NOT floor((i + 0.5) * extent / size): the two differ at extents 2, 4, 8, 16, 32, ..."""
    step = np.float64(extent) / np.float64(size)
    out = np.empty(size, dtype=np.int64)
    o = step * np.float64(0.5)
    for i in range(size):
        out[i] = int(o)
        o = o + step
    return out


def boxes_and_small(masks, size=7):
    """masks [N,H,W] -> (boxes [N,4] int32 (xmin, ymin, xmax+1, ymax+1), small [N,size,size] bool, area [N] int32).
    An empty mask raises ValueError, as ind_xy[1].min() does in the reference."""
    masks = np.asarray(masks) != 0
    n = masks.shape[0]
    boxes = np.zeros((n, 4), dtype=np.int32)
    small = np.zeros((n, size, size), dtype=bool)
    area = np.zeros(n, dtype=np.int32)
    for i in range(n):
        ys, xs = np.nonzero(masks[i])                                      # generate_7_7_voc.py:36
        if ys.size == 0:
            raise ValueError("proposal %d has no pixel" % i)
        xmin, ymin, xmax, ymax = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1   # :37
        crop = masks[i, ymin:ymax, xmin:xmax]                              # :38
        ry, rx = nearest_index(ymax - ymin, size), nearest_index(xmax - xmin, size)   # :39
        ok = (ry < crop.shape[0])[:, None] & (rx < crop.shape[1])[None, :]             # PIL leaves 0 outside the source
        small[i] = crop[np.minimum(ry, crop.shape[0] - 1)][:, np.minimum(rx, crop.shape[1] - 1)] & ok
        boxes[i] = (xmin, ymin, xmax, ymax)
        area[i] = ys.size
    return boxes, small, area


def covered(cnt, nsel):
    """mean(0) > 0.7 as NumPy evaluates it on a 0 / 1 array: fp64 sum / count against the double 0.7."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(cnt) / np.float64(nsel) > 0.7


def covered_int(cnt, nsel):
    """The same predicate in integers (what the device evaluates)."""
    return 10 * cnt > 7 * nsel


def assign_clusters(masks, rows, cols, classes, num_classes):
    """masks [N,H,W], P points (row, col, class) in the order the reference visits them -> mat [N, C+1] float32."""
    masks = (np.asarray(masks) != 0)
    n = masks.shape[0]
    flat = masks.reshape(n, -1)
    area = flat.sum(1).astype(np.int64)
    bits = np.packbits(flat, axis=1)                                       # only to count intersections 8 pixels at a time
    mat = np.zeros((n, num_classes + 1), dtype=np.float32)                 # point_level_label_assign.py:58
    cluster_idx = 1
    if len(rows) == 0:
        mat[mat.sum(1) == 0, 0] = cluster_idx                              # :60-61
        return mat
    bg_agg = np.zeros(n, dtype=np.float32)                                 # :66
    for j in range(len(rows)):
        sel = masks[:, rows[j], cols[j]]                                   # :75
        cnt = flat[sel].sum(0).astype(np.int64)
        avg = covered(cnt, int(sel.sum()))                                 # :78 (no member: NaN > 0.7 = all False)
        inter = _POPCOUNT[bits & np.packbits(avg)[None]].sum(1, dtype=np.int64)   # mask_utils.py:15: (m_a & m_b).sum()
        union = area + np.int64(avg.sum()) - inter                         # :16
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = (inter / union).astype(np.float32)                       # :17 (int64 / int64 -> f64, stored as f32)
        assign = iou > 0.5                                                 # point_level_label_assign.py:80
        mat[assign, :] = 0                                                 # :82
        mat[assign, classes[j] + 1] = cluster_idx                          # :83
        bg_agg += (iou <= 0.5).astype(np.float32) * (iou != 0).astype(np.float32)   # :85-88
        cluster_idx += 1                                                   # :90
    bg = (bg_agg != 0).astype(np.float32) * (mat.sum(1) == 0).astype(np.float32)   # :92
    mat[bg != 0, 0] = cluster_idx                                          # :93
    return mat


def pack_bits(masks):
    """[N,H,W] bool -> (np.packbits bytes, shape): how the goldens store full-resolution masks."""
    masks = np.asarray(masks) != 0
    return np.packbits(masks.reshape(-1)), np.array(masks.shape, dtype=np.int64)


def unpack_bits(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(tuple(int(s) for s in shape)).astype(bool)
