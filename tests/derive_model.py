"""The derived-volume contract of include/volviz.h (vv_derive_volume, rules 1-5) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; a box is ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive; a factor
is (fx, fy, fz).  Nothing here comes from the library: the cell is walked offset by offset in the contract's order (at most 512 offsets, each a
vectorised binary32 add over all output voxels), the classification index is hist_model's bin function and the f32 extrema are taken over its
integer keys.  Results are compared exactly (same()): bytes, or uint32 patterns."""
import numpy as np

import hist_model as HM

f32 = np.float32
MEAN, MAX, MIN = 0, 1, 2
U8, F32 = 0, 1
NAN_BITS = np.uint32(0x7FC00000)


def dims(extent, factor):
    """Rule: m_a = ceil((hi_a - lo_a) / f_a), per axis (x, y, z)."""
    return tuple(-(-int(e) // int(f)) for e, f in zip(extent, factor))


def _factor(factor):
    f = (factor,) * 3 if np.isscalar(factor) else tuple(factor)
    return tuple(int(v) if int(v) else 1 for v in f)


def _cells(sub, factor):
    """The box padded to whole cells, and which of its voxels exist: arrays [mz * fz, my * fy, mx * fx]."""
    fx, fy, fz = factor
    bz, by, bx = sub.shape
    mx, my, mz = dims((bx, by, bz), factor)
    pad = np.zeros((mz * fz, my * fy, mx * fx), sub.dtype)
    pad[:bz, :by, :bx] = sub
    valid = np.zeros(pad.shape, bool)
    valid[:bz, :by, :bx] = True
    return pad, valid


def reduce(vol, box=None, factor=1, mode=MEAN):
    """Rules 1 and 2: r of every output voxel, [mz, my, mx]: uint8 for u8 volumes, float32 (look at it as uint32) for f32 volumes."""
    sub = HM.crop(np.asarray(vol), box)
    fx, fy, fz = factor = _factor(factor)
    pad, valid = _cells(sub, factor)
    offsets = [(dz, dy, dx) for dz in range(fz) for dy in range(fy) for dx in range(fx)]          # memory order: x fastest, then y, then z
    pick = lambda a, o: a[o[0]::fz, o[1]::fy, o[2]::fx]
    shape = pick(pad, offsets[0]).shape
    n = np.zeros(shape, np.int64)
    for o in offsets:
        n += pick(valid, o)
    assert n.min() >= 1 and pick(valid, offsets[0]).all()              # every cell has its first voxel
    if sub.dtype == np.uint8:
        if mode == MEAN:
            s = np.zeros(shape, np.int64)
            for o in offsets:
                s += np.where(pick(valid, o), pick(pad, o), 0)
            return ((2 * s + n) // (2 * n)).astype(np.uint8)
        best = pick(pad, offsets[0]).astype(np.int64)
        for o in offsets[1:]:
            v, ok = pick(pad, o).astype(np.int64), pick(valid, o)
            best = np.where(ok & ((v > best) if mode == MAX else (v < best)), v, best)
        return best.astype(np.uint8)
    assert sub.dtype == np.float32
    if mode == MEAN:
        with np.errstate(all="ignore"):
            acc = pick(pad, offsets[0]).copy()                          # starts as the first voxel
            for o in offsets[1:]:
                added = acc + pick(pad, o)                              # one binary32 add
                assert added.dtype == np.float32
                acc = np.where(pick(valid, o), added, acc)
            r = acc / n.astype(f32)                                     # IEEE division, binary32
            assert r.dtype == np.float32
        return np.where(n == 1, acc.view(np.uint32), r.view(np.uint32)).view(f32)      # n == 1: the voxel bit for bit
    key = np.zeros(shape, np.uint32)                                    # 0: no non-NaN voxel yet (no key is 0)
    bits = np.full(shape, NAN_BITS, np.uint32)
    for o in offsets:
        v = np.ascontiguousarray(pick(pad, o))
        k = HM.keys(v).astype(np.uint32)
        if mode == MIN:
            k = ~k                                                      # the least key is the greatest complemented key
        take = pick(valid, o) & ~np.isnan(v) & (k > key)
        key, bits = np.where(take, k, key), np.where(take, v.view(np.uint32), bits)
    return bits.view(f32)


def finish(r, out_type, window=None):
    """Rule 3: stage 1's r -> the output volume (uint8 or float32)."""
    r = np.asarray(r)
    with np.errstate(all="ignore"):
        if window is not None:
            lo, hi = f32(window[0]), f32(window[1])
            u = r.astype(f32)                                           # (float)r of a byte is exact
            w = (u - lo) / (hi - lo)
            assert w.dtype == np.float32
            return w if out_type == F32 else HM.bins(w)
        if r.dtype == np.uint8:
            return r.copy() if out_type == U8 else r.astype(f32) / f32(255)            # correctly rounded: IEEE division
        return r.copy() if out_type == F32 else HM.bins(r)


def window_ok(window):
    """Rule 7: both ends and their binary32 difference finite, the difference > 0."""
    with np.errstate(all="ignore"):
        lo, hi = f32(window[0]), f32(window[1])
        span = f32(hi - lo)
    return bool(np.isfinite(lo) and np.isfinite(hi) and np.isfinite(span) and span > 0)


def derive(vol, box=None, factor=1, mode=MEAN, out_type=None, window=None):
    vol = np.asarray(vol)
    if out_type is None:
        out_type = U8 if vol.dtype == np.uint8 else F32
    return finish(reduce(vol, box, factor, mode), out_type, window)


def same(got, want, nan_free_for_all=False):
    """Exact: bytes, or uint32 patterns; `nan_free_for_all` (results of MEAN on f32 volumes): a NaN on both sides is equal whatever its pattern.
    Returns the indices that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.uint8:
        return np.argwhere(got != want)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = g != w
    if nan_free_for_all:
        bad &= ~(np.isnan(got) & np.isnan(want))
    return np.argwhere(bad)
