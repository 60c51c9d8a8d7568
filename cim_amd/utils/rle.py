"""COCO's compressed RLE string <-> run counts, on the host, vectorised in NumPy (pycocotools' rleToString / rleFrString,
as the reference's coco_encode and COCO annotation files use them).

Each count becomes a variable-length run of 5-bit groups, least significant first, each stored as chr(48 + group | 0x20 if
more groups follow); the value is two's complement (the last group's 0x10 bit is its sign), and for index i > 2 the count
two places back is subtracted first (i > 2, not i >= 2: pycocotools' own rule).  Counts are uint32.
"""
import numpy as np

_MAXG = 8                                  # 5-bit groups for any int64 difference of two uint32 values (35 bits signed)


def counts_to_string(counts):
    """uint32 run counts -> the compressed string (str)."""
    c = np.asarray(counts, dtype=np.int64).ravel()
    if c.size == 0:
        return ""
    if c.min() < 0 or c.max() > 0xFFFFFFFF:
        raise ValueError("rle: counts must be uint32")
    x = c.copy()
    x[3:] -= c[1:-2]
    # groups needed: the fewest n with x representable in 5n-bit two's complement
    mag = np.where(x >= 0, x, ~x)
    bits = np.zeros(x.shape, np.int64)
    v = mag.copy()
    while True:
        nz = v > 0
        if not nz.any():
            break
        bits += nz
        v >>= 1
    n = np.maximum(1, (bits + 1 + 4) // 5)
    shifts = 5 * np.arange(_MAXG, dtype=np.int64)
    grp = (x[:, None] >> shifts[None, :]) & 0x1F
    more = np.arange(_MAXG)[None, :] < (n[:, None] - 1)
    ch = (grp | np.where(more, 0x20, 0)) + 48
    keep = np.arange(_MAXG)[None, :] < n[:, None]
    return ch[keep].astype(np.uint8).tobytes().decode("ascii")


def string_to_counts(s):
    """The compressed string (str or bytes) -> uint32 run counts."""
    b = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), dtype=np.uint8).astype(np.int64)
    if b.size == 0:
        return np.zeros(0, np.uint32)
    c = b - 48
    if c.min() < 0 or c.max() > 63:
        raise ValueError("rle: not a COCO compressed RLE string")
    end = (c & 0x20) == 0                                              # the last group of a value
    if not end[-1]:
        raise ValueError("rle: truncated COCO compressed RLE string")
    vid = np.concatenate([[0], np.cumsum(end)[:-1]])                   # value index of every character
    starts = np.flatnonzero(np.concatenate([[True], end[:-1]]))
    k = np.arange(b.size) - starts[vid]                                # group index within the value
    if k.max() >= 13:
        raise ValueError("rle: run count out of range")
    x = np.add.reduceat((c & 0x1F) << (5 * k), starts)
    last = np.flatnonzero(end)
    nk = k[last] + 1
    neg = (c[last] & 0x10) != 0
    x = np.where(neg, x - (np.int64(1) << (5 * nk)), x)                # x |= -1 << 5 k
    # cnts[m] = x[m] + cnts[m - 2] for m > 2: a running sum per parity from index 1 (odd) and index 2 (even)
    out = x.copy()
    if out.size > 3:
        out[3::2] = x[1] + np.cumsum(x[3::2])
    if out.size > 4:
        out[4::2] = x[2] + np.cumsum(x[4::2])
    return (out & 0xFFFFFFFF).astype(np.uint32)


def counts_to_mask(counts, h, w):
    """Run counts -> [h, w] uint8 mask (column-major runs; host-side, for tests and small inputs)."""
    c = np.asarray(counts, dtype=np.int64)
    flat = np.zeros(h * w, np.uint8)
    ends = np.minimum(np.cumsum(c), h * w)
    starts = np.concatenate([[0], ends[:-1]])
    for s, e in zip(starts[1::2], ends[1::2]):
        flat[s:e] = 1
    return flat.reshape(w, h).T.copy()
