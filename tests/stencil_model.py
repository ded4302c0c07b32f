"""The neighbourhood-filter contract of include/volviz.h (vv_stencil_volume, rules 1-6; vv_stencil_taps) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; a box is ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive, None = the
whole volume.  Nothing here comes from the library.  A result for a box is computed for the box: every value a stencil reaches is gathered with
np.take at coordinates clipped to the volume (rule 1), so that "the box is the crop of the whole" is something the model can be asked, not
something it assumes.  Every arithmetic step is one vectorised binary32 operation over whole arrays, in the contract's order.  The classification
index and the integer keys of binary32 patterns are hist_model's.  Results are compared exactly (same()): bytes, or uint32 patterns."""
import math

import numpy as np

import hist_model as HM

f32 = np.float32
SEPARABLE, MEDIAN, GRADMAG = 0, 1, 2
BOX, BINOMIAL, GAUSS = 0, 1, 2
U8, F32 = 0, 1
MAX_RADIUS = 4


def _box(vol, box):
    nz, ny, nx = vol.shape
    if box is None:
        return (0, 0, 0), (nx, ny, nz)
    (x0, y0, z0), (x1, y1, z1) = box
    assert 0 <= x0 < x1 <= nx and 0 <= y0 < y1 <= ny and 0 <= z0 < z1 <= nz, box
    return (x0, y0, z0), (x1, y1, z1)


def _gather(a, xs, ys, zs):
    """a at the coordinate lists (any integers), each clipped to the volume: rule 1."""
    nz, ny, nx = a.shape
    a = np.take(a, np.clip(zs, 0, nz - 1), axis=0)
    a = np.take(a, np.clip(ys, 0, ny - 1), axis=1)
    return np.take(a, np.clip(xs, 0, nx - 1), axis=2)


def source(vol):
    """u of rule 1: the voxel in storage units as binary32."""
    vol = np.asarray(vol)
    assert vol.dtype in (np.uint8, np.float32)
    return vol.astype(f32) if vol.dtype == np.uint8 else vol


def radii(radius):
    r = (radius,) * 3 if np.isscalar(radius) else tuple(radius)
    assert len(r) == 3 and all(0 <= int(v) <= MAX_RADIUS for v in r), radius
    return tuple(int(v) for v in r)


def tap_rows(taps):
    """One row of taps for all three axes, or three rows (x, y, z): float32 [3, 5], missing entries 0."""
    t = np.zeros((3, 5), f32)
    if taps is not None:
        a = np.asarray(taps, f32)
        for axis in range(3):
            row = a if a.ndim == 1 else a[axis]
            t[axis, :len(row)] = row[:5]
    return t


def _pass(v, axis, n_out, R, t):
    """One pass of rule 3 along `axis` of v, whose positions along it are the n_out output positions with R more on either side."""
    pick = lambda k: np.take(v, np.arange(R + k, R + k + n_out), axis=axis)
    if R == 0:
        return v.copy()                                         # the identity, bit for bit
    with np.errstate(all="ignore"):
        acc = f32(t[0]) * pick(0)
        for k in range(1, R + 1):
            pair = pick(-k) + pick(k)                           # the pair's sum,
            acc = acc + f32(t[k]) * pair                        # then the product, then the add
        assert acc.dtype == np.float32
    return acc


def separable(vol, box=None, radius=(0, 0, 0), taps=None):
    """Rule 3: r of every voxel of the box, float32 [bz, by, bx] (radius (0, 0, 0) on an f32 volume: the voxels themselves)."""
    vol = np.asarray(vol)
    (x0, y0, z0), (x1, y1, z1) = _box(vol, box)
    rx, ry, rz = radii(radius)
    t = tap_rows(taps)
    # u where P_x is wanted: the box's x with its halo, on the rows and slices the later passes reach.  A coordinate outside the volume brings
    # the clamped voxel, and what a pass makes of clamped voxels is its value at the clamped coordinate: each pass clamps on its own axis.
    u = _gather(source(vol), np.arange(x0 - rx, x1 + rx), np.arange(y0 - ry, y1 + ry), np.arange(z0 - rz, z1 + rz))
    px = _pass(u, 2, x1 - x0, rx, t[0])
    py = _pass(px, 1, y1 - y0, ry, t[1])
    return _pass(py, 0, z1 - z0, rz, t[2])


def _neighbourhood(a, box):
    """The 27 clamped shifts of a over the box, [27, bz, by, bx]."""
    (x0, y0, z0), (x1, y1, z1) = box
    xs, ys, zs = np.arange(x0, x1), np.arange(y0, y1), np.arange(z0, z1)
    return np.stack([_gather(a, xs + dx, ys + dy, zs + dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def median(vol, box=None):
    """Rule 4: the 14th smallest of the 27, a copy of a voxel: uint8, or float32 (look at it as uint32)."""
    vol = np.asarray(vol)
    box = _box(vol, box)
    if vol.dtype == np.uint8:
        return np.sort(_neighbourhood(vol, box), axis=0)[13]
    k = np.sort(_neighbourhood(HM.keys(vol), box), axis=0)[13]
    bits = np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k)       # the key's inverse
    return bits.astype(np.uint32).view(f32)


def gradmag(vol, box=None, gscale=None):
    """Rule 5, float32 [bz, by, bx]."""
    vol = np.asarray(vol)
    (x0, y0, z0), (x1, y1, z1) = _box(vol, box)
    g = (1.0, 1.0, 1.0) if gscale is None or not any(float(v) != 0.0 for v in gscale) else gscale
    u = source(vol)
    xs, ys, zs = np.arange(x0, x1), np.arange(y0, y1), np.arange(z0, z1)
    with np.errstate(all="ignore"):
        gx = (_gather(u, xs + 1, ys, zs) - _gather(u, xs - 1, ys, zs)) * f32(g[0])
        gy = (_gather(u, xs, ys + 1, zs) - _gather(u, xs, ys - 1, zs)) * f32(g[1])
        gz = (_gather(u, xs, ys, zs + 1) - _gather(u, xs, ys, zs - 1)) * f32(g[2])
        r = np.sqrt((gx * gx + gy * gy) + gz * gz)
        assert r.dtype == np.float32
    return r


def finish(r, src_dtype, out_type, kind):
    """Rule 6: r -> the output volume (uint8 or float32)."""
    r = np.asarray(r)
    with np.errstate(all="ignore"):
        if src_dtype == np.float32:
            return r.copy() if out_type == F32 else HM.bins(r)
        if kind == MEDIAN:
            assert r.dtype == np.uint8
            return r.copy() if out_type == U8 else r.astype(f32) / f32(255)
        assert r.dtype == np.float32
        if out_type == F32:
            return r / f32(255)                                 # IEEE division
        s = r + f32(0.5)                                        # one binary32 add,
        out = np.zeros(r.shape, np.uint8)                       # NaN, r < 0.5
        mid = (r >= f32(0.5)) & (r < f32(254.5))
        out[mid] = np.trunc(s[mid]).astype(np.int64).astype(np.uint8)      # then truncation
        out[r >= f32(254.5)] = 255
        return out


def result(vol, kind, box=None, radius=(0, 0, 0), taps=None, gscale=None):
    """r of rules 3-5 for one call."""
    if kind == SEPARABLE:
        return separable(vol, box, radius, taps)
    if kind == MEDIAN:
        return median(vol, box)
    assert kind == GRADMAG
    return gradmag(vol, box, gscale)


def stencil(vol, kind, box=None, out_type=None, radius=(0, 0, 0), taps=None, gscale=None):
    vol = np.asarray(vol)
    if out_type is None:
        out_type = U8 if vol.dtype == np.uint8 else F32
    return finish(result(vol, kind, box, radius, taps, gscale), vol.dtype, out_type, kind)


def taps(shape, radius, sigma=0.0):
    """vv_stencil_taps: float32[5]."""
    R = int(radius)
    assert 0 <= R <= MAX_RADIUS and shape in (BOX, BINOMIAL, GAUSS)
    t = np.zeros(5, f32)
    if shape == BOX:
        t[:R + 1] = f32(1) / f32(2 * R + 1)
    elif shape == BINOMIAL:
        t[:R + 1] = [f32(math.comb(2 * R, R + k)) / f32(4 ** R) for k in range(R + 1)]
    else:
        assert math.isfinite(sigma) and sigma > 0
        s = float(f32(sigma))                                   # the argument is a float
        w = [math.exp(-float(k * k) / (2.0 * s * s)) for k in range(R + 1)]
        total = w[0]
        for k in range(1, R + 1):
            total += 2.0 * w[k]
        t[:R + 1] = [f32(v / total) for v in w]                 # one rounding to binary32
    return t


def same(got, want, nan_free_for_all=False):
    """Exact: bytes, or uint32 patterns; `nan_free_for_all` (arithmetic results): a NaN on both sides is equal whatever its pattern.  Returns
    the indices that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.uint8:
        return np.argwhere(got != want)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = g != w
    if nan_free_for_all:
        bad &= ~(np.isnan(got) & np.isnan(want))
    return np.argwhere(bad)
