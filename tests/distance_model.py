"""The distance-transform contract of include/volviz.h (vv_distance_volume rules 1-5) and Context.morphology's compositions in numpy, int64.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; a box is ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive, None = the whole
volume.  Nothing here comes from the library and nothing from scipy.  The squared distance is the separable min-plus product written out: along each
axis in turn out[u] = min over j of g[j] + (w (u - j))^2, with the cost of every pair (u, j) in a dense table and numpy's minimum over j -- no lower
envelope, no stack, no intersection of parabolas (the kernels' form).  "No seed" is the int64 value FAR, above every sum the tables can form; it is
turned into the header's 0xFFFFFFFF only at the end.  Results are compared exactly."""
import numpy as np

import hist_model as HM

SEED_BINS, SEED_LABEL, SEED_NONZERO = 0, 1, 2
DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3
NONE = 0xFFFFFFFF                                          # VV_DIST_SQUARED of a box without a seed
MAX_EXTENT = 2048
FAR = np.int64(1) << 40                                    # above (2^32 - 2) + (2^16 - 1)^2, far below what int64 holds after three additions
TABLE = 1 << 22                                            # entries of a cost table times the lines swept at once


def seeds(vol=None, bins=None, labels=None, label=None, invert=False, box=None):
    """Rule 1: the box's seeds, bool [bz, by, bx].  bins = (lo, hi) or one bin: of `vol`; else `labels` (the box's extents) equal to `label`, or not 0."""
    assert (bins is None) != (labels is None)
    if bins is not None:
        lo, hi = (bins, bins) if np.isscalar(bins) else bins
        b = HM.bins(HM.crop(np.asarray(vol), box))
        test = (b >= lo) & (b <= hi)
    else:
        labels = np.asarray(labels, np.uint32)
        test = labels != 0 if label is None else labels == np.uint32(label)
    return test != bool(invert)


def sweep(g, axis, w):
    """out[u] = min over j of g[j] + (w (u - j))^2 along `axis` of an int64 array (FAR: nothing there), by the dense [u, j] table."""
    g = np.moveaxis(np.asarray(g, np.int64), axis, 0)
    n = g.shape[0]
    pos = np.arange(n, dtype=np.int64)
    cost = (np.int64(w) * (pos[:, None] - pos[None, :])) ** 2              # [u, j]
    flat = g.reshape(n, -1)
    out = np.empty_like(flat)
    step = max(1, TABLE // (n * n))
    for k in range(0, flat.shape[1], step):
        out[:, k:k + step] = (cost[:, :, None] + flat[None, :, k:k + step]).min(axis=1)
    return np.moveaxis(out.reshape(g.shape), 0, axis)


def limits_ok(shape, spacing=(1, 1, 1)):
    """Rule 7 for a box of `shape` = (bz, by, bx) and spacing (x, y, z), in Python's integers."""
    bz, by, bx = shape
    far = sum((int(s) * (int(b) - 1)) ** 2 for s, b in zip(spacing, (bx, by, bz)))
    return max(shape) <= MAX_EXTENT and bx * by * bz <= 2 ** 32 - 2 and far <= 0xFFFFFFFE


def squared_i64(seed, spacing=(1, 1, 1)):
    """Rule 4 as int64: D, and FAR or more everywhere if there is no seed."""
    seed = np.asarray(seed, bool)
    assert seed.ndim == 3 and limits_ok(seed.shape, spacing) and min(spacing) >= 1
    g = np.where(seed, np.int64(0), FAR)
    for axis, w in ((2, spacing[0]), (1, spacing[1]), (0, spacing[2])):
        g = sweep(g, axis, w)
    return g


def squared(seed, spacing=(1, 1, 1)):
    """VV_DIST_SQUARED of a seed array: uint32 [bz, by, bx]."""
    g = squared_i64(seed, spacing)
    return np.where(g >= FAR, NONE, g).astype(np.uint32)


def within(seed, r2, spacing=(1, 1, 1)):
    """VV_DIST_WITHIN: 1 where D <= r2, 0 elsewhere (everywhere without a seed)."""
    return (squared_i64(seed, spacing) <= np.int64(r2)).astype(np.uint32)


def distance(vol=None, bins=None, labels=None, label=None, invert=False, spacing=(1, 1, 1), box=None, within_r2=None):
    """vv_distance_volume."""
    s = seeds(vol, bins, labels, label, invert, box)
    return squared(s, spacing) if within_r2 is None else within(s, within_r2, spacing)


def brute(seed, spacing=(1, 1, 1)):
    """Rule 4 as it is written: the minimum over all (voxel, seed) pairs."""
    seed = np.asarray(seed, bool)
    pos = np.argwhere(np.ones(seed.shape, bool)).astype(np.int64)           # (z, y, x)
    s = np.argwhere(seed).astype(np.int64)
    if len(s) == 0:
        return np.full(seed.shape, NONE, np.uint32)
    w = np.array([spacing[2], spacing[1], spacing[0]], np.int64)
    d = (((pos[:, None, :] - s[None, :, :]) * w) ** 2).sum(axis=2).min(axis=1)
    return d.astype(np.uint32).reshape(seed.shape)


def radius2(radius):
    """Context.morphology's r2 = floor(radius^2) in binary64."""
    return int(np.floor(float(radius) * float(radius)))


def morphology(op, seed, radius, spacing=(1, 1, 1)):
    """Context.morphology on a seed array: the 0 / 1 uint32 set.  The box is the world: the complement ends at its faces."""
    seed = np.asarray(seed, bool)
    r2 = radius2(radius)
    dil = lambda s: within(s, r2, spacing).astype(bool)
    ero = lambda s: ~within(~s, r2, spacing).astype(bool)
    out = {DILATE: lambda: dil(seed), ERODE: lambda: ero(seed), OPEN: lambda: dil(ero(seed)), CLOSE: lambda: ero(dil(seed))}[op]()
    return out.astype(np.uint32)


def same(got, want):
    """Exact.  Returns the indices that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return np.argwhere(got != want)
