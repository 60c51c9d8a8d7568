"""Seeded inputs of the fused loss launch (cim_amd/csrc/losses.hip) at the shapes and values where its jobs take another path,
shared by tests/test_loss_cases_cpu.py and tests/test_gpu_losses_edges.py.  Integer permutations, IEEE divisions and exact
constants only (no libm call): bit-identical on every host.

`loss_case(name)` -> dict(pc, pd, rc[R], ri[R], labels [1,C], pseudo[R] = (pseudo_labels f32 [N,C1], pseudo_iou f16 [N],
loss_weights f32 [N]), valid int32 [R], scales [R], mat [N,C1], N, C1, R, zero = the gradient components the case zeroes on
purpose, fp32 = the case saturates the clamps (its references run in float32), first_max = the case has tied maxima).
Gradient components, in the order of the kernel's `grad` planes: 0 d mil/d pc, 1 d pcl/d pc, 2 d mil/d pd, then per layer i
3+4i d cls/d rc, 4+4i d bag/d rc, 5+4i d iou/d ri, 6+4i d bag/d ri."""
import numpy as np

F32 = np.float32
LO, HI = F32(1e-6), F32(1 - 1e-6)                # the clamp bounds as the kernel and the fp32 reference hold them
UP4 = (0.7, 1.3, 2.0, 0.5)                       # upstream gradients of (bag, pcl, cls, iou)
UP6 = UP4 + (0.9, 1.1)                           # ... and of (3 iou, total) for the with_total outputs


def lds_bytes(n, c1):
    """Dynamic LDS of cim_losses_fwd for [n, c1] scores (the launch raises the kernel's limit above 64 KiB)."""
    g = group_size(c1)
    return 64 + 8 * n + (16 * (1024 // g) * c1 + 16 if g <= 256 else 0) + 256


def group_size(c1):
    """Lanes per row of the column passes: the smallest of 32, 64, 128, 256 that is at least c1, else 1024 (a wave per column)."""
    return next((g for g in (32, 64, 128, 256) if g >= c1), 1024)


def _unit(rs, n, c1, lo=1e-4):
    """A permutation of n*c1 equidistant values in [lo, 1 - lo]: tie-free, nothing near a clamp bound."""
    m = n * c1
    k = rs.permutation(m).astype(np.float64).reshape(n, c1)
    return (lo + k / max(m - 1, 1) * (1 - 2 * lo)).astype(F32)


def _det(rs, n, c1):
    """A permutation divided by its (exact, integer) column sums, each column times a factor in (0.2, 1): like a softmax over
    the proposals, the MIL column sums of cls * det lie well inside the clamp."""
    k = (rs.permutation(n * c1) + 1).reshape(n, c1)
    factor = 0.2 + 0.8 * (rs.permutation(c1) + 1.0) / (c1 + 1)
    return (k / k.sum(axis=0, dtype=np.int64).astype(np.float64) * factor).astype(F32)


def _labels(rs, c1, pos_cols=None):
    """[1, C] image labels with at least three positives; -> (labels, positive COLUMNS of the [N, C1] scores, ascending)."""
    c = c1 - 1
    if pos_cols is None:
        pos_cols = np.sort(rs.permutation(c)[:max(3, c // 4)] + 1)
    labels = np.zeros((1, c), F32)
    labels[0, np.asarray(pos_cols) - 1] = 1
    return labels, [int(x) for x in pos_cols]


def _pseudo(rs, n, c1, fg_cols, with_fg):
    """One layer's mining result: a third of the rows foreground (one-hot in one of fg_cols), a third background (column 0), a
    third unlabelled (all-zero row); with_fg=False turns the foreground rows into background rows (n_fg = 0)."""
    y = np.zeros((n, c1), F32)
    for i, r in enumerate(rs.permutation(n)):
        kind = i % 3                                                     # (n = 1: the one row is labelled)
        if kind == 0:
            y[r, fg_cols[(i // 3) % len(fg_cols)] if with_fg else 0] = 1
        elif kind == 1:
            y[r, 0] = 1
    t16 = ((rs.permutation(n) + 1.0) / (n + 1)).astype(np.float16)
    w = (0.5 + (rs.permutation(n) + 1.0) / (n + 1)).astype(F32)          # distinct: a wrong arg-max row changes the bag loss
    return y, t16, w


def _mat(rs, n, c1):
    """PRM clusters, one non-zero per row: a background cluster (id 3, column 0), ids 1 and 5 in one column, id 2 in another;
    about half of the rows in no cluster."""
    mat = np.zeros((n, c1), F32)
    order = rs.permutation(n)
    a, b = 1 + int(rs.randint(c1 - 1)), 1 + int(rs.randint(c1 - 1))
    if n < 8:
        mat[order[0], a] = 1
        if n > 1:
            mat[order[1], 0] = 3
        return mat
    q = n // 8
    mat[order[:q], 0] = 3
    mat[order[q:2 * q], a] = 1
    mat[order[2 * q:3 * q], b] = 2
    mat[order[3 * q:3 * q + max(q // 2, 1)], a] = 5
    return mat


def _generic(n, c1, r, seed, pos_cols=None):
    """The ingredients every case starts from.  The FIRST positive class has no labelled row in any layer (all f are 0: the
    arg-max is row 0, the gradient gated off); layer 1 has no foreground row."""
    rs = np.random.RandomState(seed)
    labels, pos = _labels(rs, c1, pos_cols)
    case = dict(N=n, C1=c1, R=r, labels=labels, pos_cols=pos, orphan_col=pos[0], zero=set(), fp32=False, first_max=False)
    case["pc"], case["pd"] = _unit(rs, n, c1, 1e-3), _det(rs, n, c1)      # (N = 1: pc * det >= 1e-3 * 0.2, inside the MIL clamp)
    case["rc"] = [_unit(rs, n, c1) for _ in range(r)]
    case["ri"] = [_unit(rs, n, c1) for _ in range(r)]
    case["pseudo"] = [_pseudo(rs, n, c1, pos[1:], with_fg=(i != 1)) for i in range(r)]
    if r > 1:
        case["zero"].add(5 + 4 * 1)
    if n == 1:                                                           # (the one row is foreground or background)
        case["zero"] |= {5 + 4 * i for i in range(r) if not (case["pseudo"][i][0][:, 1:] != 0).any()}
    case["valid"] = np.ones(r, np.int32)
    case["scales"] = [3, 1, 1][:r]
    case["mat"] = _mat(rs, n, c1)
    return case


# ------------------------------------------------------------------------------------------------ ties
def _tied_rows(c, wave):
    """Three rows that share column c's maximum.  Group form (N = 96, 32 groups of 32 lanes, row n in group n % 32): the first
    row lies in a HIGHER group than the second and the third 64 rows on, so the merge in group order meets a later row first.
    Wave form (N = 130, row n in lane n % 64): the same with lanes.  Disjoint between columns in the group form; in the wave
    form for the columns in TIES_POS_COLS and column 0."""
    if wave:
        return [20 + c % 40, 64 + c % 20, 100 + c % 30]
    return [11 + c, 32 + (c + 3) % 21, 69 + c]


TIES_POS_COLS = {21: [3, 7, 12, 15], 257: [3, 7, 12, 15, 205]}           # (3 = the class without a labelled row)


def _ties(c1, seed):
    """Every product rc * ri is exact in fp32 (powers of two and 0.75): ordinary entries give at most 0.125, the three tied
    rows of a column 0.5 * 0.5; a seen column also holds 0.75 * 0.5 in a row that is NOT labelled with it (it must be masked
    out).  Seen columns tie among their labelled rows, unseen columns among all rows, the class without a labelled row among
    all rows at 0.  The tied rows carry different loss_weights."""
    wave = c1 > 256
    n = 130 if wave else 96
    case = _generic(n, c1, 3, seed, TIES_POS_COLS[c1])
    case["first_max"] = True
    rs = np.random.RandomState(seed + 1)
    seen = [0] + case["pos_cols"][1:]
    for i in range(3):
        rc = np.where(rs.randint(2, size=(n, c1)) == 0, F32(0.125), F32(0.25)).astype(F32)
        ri = np.where(rs.randint(2, size=(n, c1)) == 0, F32(0.25), F32(0.5)).astype(F32)
        y = np.zeros((n, c1), F32)
        tied = {x for c in range(c1) for x in _tied_rows(c, wave)}
        for c in range(c1):
            rows = _tied_rows(c, wave)
            rc[rows, c] = ri[rows, c] = 0.5
            if c in seen:
                if c == 0 or i != 1:                                     # (layer 1: no foreground row)
                    y[rows, c] = 1
                trap = 1 + seen.index(c)                                 # rows 1..10 are nobody's tied row and stay unlabelled
                rc[trap, c], ri[trap, c] = 0.75, 0.5
        free = [x for x in range(11, n) if x not in tied]                # rows 0..10 stay unlabelled (row 0, the traps)
        for j, x in enumerate(free):
            if j % 3 == 0:
                y[x, 0] = 1
            elif j % 3 == 1 and i != 1:
                y[x, seen[1 + j % (len(seen) - 1)]] = 1
        case["rc"][i], case["ri"][i] = rc, ri
        case["pseudo"][i] = (y,) + case["pseudo"][i][1:]
    return case


# ------------------------------------------------------------------------------------------------ saturated
def _nx(x, to):
    return np.nextafter(F32(x), F32(to))


SPECIALS = [F32(0), F32(1), LO, HI, _nx(LO, 0), _nx(LO, 1), _nx(HI, 0), _nx(HI, 2), F32(0.3), F32(0.7)]
# (rc, ri) in the hot column of the first labelled rows of each class: every bound from both sides; (1, HI) is the one pair whose
# clamped product (HI * HI) no other reaches, so a class's labelled arg-max is unique
HOT_PAIRS = [(F32(1), HI), (F32(0), _nx(HI, 2)), (LO, F32(1)), (_nx(LO, 0), F32(0)), (_nx(LO, 1), _nx(LO, 1)),
             (_nx(HI, 0), F32(0.3)), (HI, LO), (F32(0.7), _nx(HI, 0))]
# ... and at the arg-max row of an unseen column (all above the (1 - 1e-4)^2 of ordinary entries, all different)
TOP_PAIRS = [(HI, F32(1)), (_nx(HI, 2), _nx(HI, 0)), (_nx(HI, 0), _nx(HI, 0)), (F32(0.99995), HI)]


def _saturated(seed):
    """Exact 0 and 1, both clamp bounds and their fp32 neighbours at every place a clamp and its gradient gate are applied.
    Smooth-L1: |d| = |clamp(ri) - target| <= 1 - 1e-6 for scores and fp16 targets in [0, 1] - the linear branch (|d| >= 1) is
    unreachable; the rows (ri, target) = (0, 1) and (1, 0) come closest (0.999999) and tests/test_loss_cases_cpu.py asserts
    |d| < 1 over all cases.  The bag's `raw` is a product of two clamped scores, at most HI * HI < HI: only its lower gate can
    close (the class without a labelled row, and one unseen column whose rc is 0 in every row)."""
    n, c1 = 96, 21
    case = _generic(n, c1, 3, seed)
    case["fp32"] = True
    unseen = [c for c in range(1, c1) if c not in case["pos_cols"]]
    for i in range(3):
        rc, ri = case["rc"][i], case["ri"][i]
        y, t16, w = case["pseudo"][i]
        t16 = t16.copy()
        for c in range(c1):
            rows = np.nonzero(y[:, c])[0][:len(HOT_PAIRS)]
            for j, r in enumerate(rows):
                k = 1 + (j - 1 + c + i) % (len(HOT_PAIRS) - 1) if j else 0   # (the first labelled row of a class is its arg-max)
                rc[r, c], ri[r, c] = HOT_PAIRS[k]
                if ri[r, c] == 0:
                    t16[r] = 1.0                                         # d = 1e-6 - 1
                elif ri[r, c] == 1:
                    t16[r] = 0.0                                         # d = 1 - 1e-6
        for j, c in enumerate(unseen[1:]):
            rc[(7 * c + i) % n, c], ri[(7 * c + i) % n, c] = TOP_PAIRS[(j + i) % len(TOP_PAIRS)]
        rc[:, unseen[0]] = 0                                             # raw = 1e-6 * max clamp(ri) < 1e-6: the bag's gate closes
        case["pseudo"][i] = (y, t16, w)
    pc, pd, mat = case["pc"], case["pd"], case["mat"]
    for i, r in enumerate(np.nonzero(mat[:, 0])[0]):                     # background-cluster rows: element-wise clamps
        for k, s in enumerate(SPECIALS):
            pc[r, (i + k) % c1] = s
    rows1, rows2 = np.nonzero((mat == 1).any(1))[0], np.nonzero((mat == 2).any(1))[0]
    pc[rows1, 1], pc[rows1, 2] = 1, 0                                    # cluster means exactly 1 and 0 (sums of 0 and 1 are exact)
    pc[rows2, 4], pc[rows2, 5] = 0, 1
    lone = int(np.nonzero(~(mat != 0).any(1))[0][0])                     # a one-row cluster: its mean IS the row, bounds included
    mat[lone, 9] = 7
    pc[lone, :len(SPECIALS)] = SPECIALS
    pd[:, 6] *= F32(16)                                                  # MIL column sums above 1 ...
    pd[:, 7] *= F32(2.0 ** -24)                                          # ... and below 1e-6
    case["mil_out"] = (6, 7)
    return case


# ------------------------------------------------------------------------------------------------ PCL shapes
def _pcl_mat(kind, n, c1, rs):
    mat = np.zeros((n, c1), F32)
    order = rs.permutation(n)
    q = n // 8
    if kind == "no_bg":
        mat[order[:q], 4] = 1
        mat[order[q:2 * q], 9] = 2
    elif kind == "only_bg":
        mat[order[:3 * q], 0] = 2
    elif kind == "one_row":
        mat[order[:q], 0] = 4
        mat[order[q], 6] = 1                                             # a cluster of one row
        mat[order[q + 1:2 * q], 11] = 9
    elif kind == "ids":                                                  # non-consecutive and fractional ids, background in the middle
        for j, (cid, col) in enumerate([(1.5, 3), (7, 0), (1000, 3), (0.25, 17)]):
            mat[order[j * q:(j + 1) * q], col] = cid
    elif kind == "two_cols":                                             # one cluster over two columns
        mat[order[:q], 5] = 2
        mat[order[q:2 * q], 8] = 2
        mat[order[2 * q:3 * q], 0] = 1
    elif kind.startswith("k"):                                           # k clusters of one or two rows; id 100 is the background cluster
        k = int(kind[1:])
        assert k <= n
        for j in range(k):                                               # (a second row while the rows last)
            rows = [order[j]] + ([order[k + j]] if k + j < n else [])
            mat[rows, 0 if j + 1 == 100 else 1 + j % (c1 - 1)] = j + 1
    else:
        assert kind == "none"
    return mat


# ------------------------------------------------------------------------------------------------ the case list
def _plain(n, c1, seed, r=3):
    return lambda: _generic(n, c1, r, seed)


def _with_mat(kind, n, seed):
    def make():
        case = _generic(n, 21, 3, seed)
        case["mat"] = _pcl_mat(kind, n, 21, np.random.RandomState(seed + 7))
        if kind == "none":
            case["zero"].add(1)
        return case
    return make


def _invalid(seed):
    case = _generic(67, 21, 3, seed)
    case["valid"] = np.zeros(3, np.int32)
    case["zero"] |= set(range(3, 15))
    return case


_BUILDERS = {
    "g32_tail": _plain(67, 21, 101),
    "g32_tiny:n3": _plain(3, 21, 102),
    "g32_tiny:n1": _plain(1, 21, 103),
    "g64:c33": _plain(150, 33, 104),
    "g64:c64": _plain(150, 64, 105),
    "g128": _plain(150, 65, 106),
    "g256:c129": _plain(150, 129, 107),
    "g256:c256": _plain(150, 256, 108),
    "wave_col:c257": _plain(130, 257, 109),
    "wave_col:c300": _plain(130, 300, 110),
    "big_n:n7000": _plain(7000, 21, 111),
    "big_n:n15000": _plain(15000, 21, 112),
    "ties": lambda: _ties(21, 113),
    "ties:c257": lambda: _ties(257, 114),
    "saturated": lambda: _saturated(115),
    "pcl_shapes:no_bg": _with_mat("no_bg", 200, 116),
    "pcl_shapes:none": _with_mat("none", 200, 117),
    "pcl_shapes:only_bg": _with_mat("only_bg", 200, 118),
    "pcl_shapes:one_row": _with_mat("one_row", 200, 119),
    "pcl_shapes:ids": _with_mat("ids", 200, 120),
    "pcl_shapes:two_cols": _with_mat("two_cols", 200, 121),
    "pcl_shapes:k256": _with_mat("k256", 512, 122),
    "r_edges:r0": _plain(67, 21, 123, r=0),
    "r_edges:r1": _plain(67, 21, 124, r=1),
    "r_edges:invalid": lambda: _invalid(125),
}
LOSS_CASES = list(_BUILDERS)
_CACHE = {}


def loss_case(name):
    """The named case (built once per process; treat the arrays as read-only)."""
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


def status_mats(rs=None):
    """`mat` [512, 21] variants the PCL plan must flag in the status word: bit -> mat."""
    rs = rs or np.random.RandomState(126)
    two = _pcl_mat("one_row", 512, 21, rs)
    two[np.nonzero(two[:, 0])[0][0], 5] = 2                              # a second non-zero in one row
    bg2 = _pcl_mat("one_row", 512, 21, rs)
    bg2[np.nonzero(bg2[:, 0])[0][0], 0] = 6                              # a second id in column 0
    return {4: two, 8: bg2, 16: _pcl_mat("k257", 512, 21, rs)}
