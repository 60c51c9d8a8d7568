"""NumPy restatement, in float64, of batch-statistics BatchNorm (+ residual) (+ ReLU) (csrc/bn_train.hip):

    mean, var (biased) over the m = N HW values of a channel;  y = relu?(gamma (x - mean) / sqrt(var + eps) + beta (+ res))
    running_mean = (1 - f) running_mean + f mean;  running_var = (1 - f) running_var + f var m / (m - 1);  batches += 1
    dz = dy (y > 0);  S1 = sum dz;  S2 = sum dz (x - mean);  dbeta = S1;  dgamma = rstd S2
    dx = gamma rstd (dz - S1 / m - (x - mean) rstd^2 S2 / m);  dres = dz

and beside every sum the sum of its terms' magnitudes - what a floating-point summation's error is measured in.  Arrays are
[N, C, HW]; no torch."""
import numpy as np

CHUNK = 4096          # csrc/bn_train.hip BT_CHUNK: floats of a chunk at most
WAVE_PLANES = 4       # BT_WAVE_PLANES: a chunk of at least this many whole planes takes one wave per plane

# (N, C, HW): the shapes the issue lists ...
SHAPES = [
    (2, 1, 1),
    (1, 4, 2),
    (3, 5, 49),
    (2, 8, 196),
    (4, 3, 1000),
    (2, 64, 784),
    (16, 4, 3136),
    # ... and the boundaries of the kernel's own chunking that they do not cross.  A plane longer than CHUNK is cut into pieces of
    # CHUNK; shorter planes are gathered CHUNK // HW to a chunk, one wave per plane from WAVE_PLANES planes on, else the whole
    # workgroup plane after plane.  The channel is the grid index of the finishing launches (one wave each): there is no row of
    # channels to cross; C = 130 is here for a channel count above the lanes of that wave.
    (1, 1, 4095),                  # m one below a chunk: one chunk, a 16-byte body with a 3-float tail
    (1, 2, 4096),                  # m = a chunk exactly; the second channel's plane starts a chunk later
    (1, 1, 4097),                  # m one above: a second chunk of ONE value (count 1, M2 0)
    (2, 3, 9000),                  # a plane over three chunks (4096, 4096, 808), N > 1: six chunks per channel
    (3, 2, 2049),                  # CHUNK // HW = 1 below CHUNK: whole planes, one per chunk, odd length
    (5, 2, 1025),                  # three planes per chunk: the workgroup walks them one after another; a last chunk of two
    (9, 2, 1024),                  # four planes per chunk: one wave per plane; a last chunk of one plane (three waves idle)
    (200, 2, 41),                  # 99 planes per chunk, unaligned plane starts: waves take 25, 25, 25, 24 planes; 3 chunks, the last of two planes
    (2, 130, 3),                   # more channels than a wave has lanes
    (70, 1, 4096),                 # 70 chunks: the finishing wave's lanes take runs of two chunks, the last lanes none
]


def chunks(shape):
    """cim_bn_train_chunks of a shape."""
    n, c, hw = shape
    if hw >= CHUNK:
        return n * ((hw + CHUNK - 1) // CHUNK)
    planes = CHUNK // hw
    return n if planes == 1 else (n + planes - 1) // planes


def stats(x):
    """x [N,C,HW] -> (mean, biased var, sum |x|), each [C] float64."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=(0, 2))
    var = ((x - mean[None, :, None]) ** 2).mean(axis=(0, 2))
    return mean, var, np.abs(x).sum(axis=(0, 2))


def forward(x, gamma, beta, eps, res=None, relu=True):
    """-> (y [N,C,HW], mean, var) float64."""
    x = np.asarray(x, dtype=np.float64)
    mean, var, _ = stats(x)
    y = (x - mean[None, :, None]) / np.sqrt(var + eps)[None, :, None] * np.asarray(gamma, np.float64)[None, :, None] \
        + np.asarray(beta, np.float64)[None, :, None]
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64)
    return (np.maximum(y, 0.0) if relu else y), mean, var


def running_update(running_mean, running_var, batches, mean, var, m, momentum):
    """torch's rule for one training-mode call: -> (running_mean, running_var, batches) after it.  momentum None: the cumulative
    average, factor 1 / (the new count)."""
    batches = int(batches) + 1
    f = 1.0 / batches if momentum is None else float(momentum)
    rm = (1.0 - f) * np.asarray(running_mean, np.float64) + f * mean
    rv = (1.0 - f) * np.asarray(running_var, np.float64) + f * var * m / (m - 1.0)
    return rm, rv, batches


def backward(dy, x, y, gamma, mean, var, eps, relu=True):
    """-> dict of float64 arrays: dx, dres [N,C,HW]; dgamma, dbeta, S1, S2 [C] and the sums of the magnitudes of the terms of
    S1 and S2 (mag1, mag2).  y is the forward output (the ReLU mask; ignored without relu)."""
    dy, x = np.asarray(dy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    m = x.shape[0] * x.shape[2]
    dz = dy * (np.asarray(y) > 0) if relu else dy
    xc = x - mean[None, :, None]
    rstd = 1.0 / np.sqrt(var + eps)
    s1, s2 = dz.sum(axis=(0, 2)), (dz * xc).sum(axis=(0, 2))
    g = np.asarray(gamma, np.float64)
    dx = (g * rstd)[None, :, None] * (dz - (s1 / m)[None, :, None] - xc * (rstd * rstd * s2 / m)[None, :, None])
    return {"dx": dx, "dres": dz, "dgamma": rstd * s2, "dbeta": s1, "S1": s1, "S2": s2, "rstd": rstd,
            "mag1": np.abs(dz).sum(axis=(0, 2)), "mag2": np.abs(dz * xc).sum(axis=(0, 2))}


DATA_SETS = ("a", "b", "c", "d")


def seeded(shape, seed, kind):
    """x float32 [N,C,HW] of a data set: (a) standard normal times a per-channel scale in [0.5, 2] plus an offset in [-3, 3];
    (b) offset 1000, scale 1; (c) as (a) with channel 0 constant; (d) integers in -2..2."""
    n, c, hw = shape
    rs = np.random.RandomState(seed)
    if kind == "d":
        return rs.randint(-2, 3, shape).astype(np.float32)
    x = rs.standard_normal(shape)
    if kind == "b":
        return (x + 1000.0).astype(np.float32)
    x = x * rs.uniform(0.5, 2.0, c)[None, :, None] + rs.uniform(-3.0, 3.0, c)[None, :, None]
    if kind == "c":
        x[:, 0, :] = rs.uniform(-3.0, 3.0)
    return x.astype(np.float32)


def seeded_affine(c, seed):
    """(gamma in [0.5, 1.5], beta in [-0.5, 0.5]) float32."""
    rs = np.random.RandomState(seed)
    return rs.uniform(0.5, 1.5, c).astype(np.float32), rs.uniform(-0.5, 0.5, c).astype(np.float32)
