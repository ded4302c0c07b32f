"""The resampling contract of include/volviz.h (vv_resample_volume, rules 1-5; vv_resample_matrix) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; an output grid is dims = (mx, my, mz); a box of it is ((x0, y0, z0),
(x1, y1, z1)), lo inclusive, hi exclusive, None = the whole grid.  Nothing here comes from the library.  Coordinates (rule 1) and the inside test
(rule 2) are stated here, one vectorised binary32 operation per step in the contract's order; the trilinear value is witness.filtered (the
texture model's second statement), the classification index is hist_model.bins, the u8 rounding of rule 4 is stated here.  A result for a box
is computed for the box's own voxels, so that "the box is the crop of the whole" is something the model can be asked.  Results are compared
exactly (same()): bytes, or uint32 patterns."""
import math

import numpy as np

import hist_model as HM
import witness as Wt

f32 = np.float32
TEX8, EXACT, NEAREST = 0, 1, 2
U8, F32 = 0, 1
MAX_DIM = 16384
IDENTITY = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _box(dims, box):
    if box is None:
        return (0, 0, 0), tuple(int(v) for v in dims)
    lo, hi = box
    assert all(0 <= l < h <= n for l, h, n in zip(lo, hi, dims)), (box, dims)
    return tuple(lo), tuple(hi)


def axis_q(m_a, lo, hi):
    """Rule 1: q of the grid's voxels lo..hi-1 on an axis of m_a voxels, float32."""
    inv = f32(1) / f32(m_a)                                     # one IEEE division
    return (np.arange(lo, hi).astype(f32) + f32(0.5)) * inv


def positions(dims, matrix=None, box=None):
    """Rule 1: p of every voxel of the box, float32 [bz, by, bx, 3]."""
    m = np.asarray(IDENTITY if matrix is None else matrix, f32).reshape(12)
    lo, hi = _box(dims, box)
    qx = axis_q(dims[0], lo[0], hi[0])[None, None, :]
    qy = axis_q(dims[1], lo[1], hi[1])[None, :, None]
    qz = axis_q(dims[2], lo[2], hi[2])[:, None, None]
    with np.errstate(all="ignore"):
        rows = [((m[4 * r] * qx + m[4 * r + 1] * qy) + m[4 * r + 2] * qz) + m[4 * r + 3] for r in range(3)]
    p = np.stack(np.broadcast_arrays(*rows), axis=-1)
    assert p.dtype == np.float32
    return p


def inside(p):
    """Rule 2: all three coordinates in [0, 1) by comparison; a NaN is outside, -0.0 is inside."""
    with np.errstate(invalid="ignore"):
        return np.all((p >= f32(0)) & (p < f32(1)), axis=-1)


def nearest_index(p_a, n_a):
    """Rule 3, NEAREST: min((uint32_t)(p * (float)n), n - 1) for p in [0, 1)."""
    return np.minimum(np.trunc(p_a * f32(n_a)).astype(np.int64), n_a - 1)


def value(vol, dims, matrix=None, filt=TEX8, fill=0.0, box=None):
    """Rules 1-3: r of every voxel of the box.  TEX8 / EXACT: float32.  NEAREST: (raw, inside) with raw the copied voxels in the volume's own
    dtype (zeros outside) -- no arithmetic touches a copied voxel, so none is made on it here either."""
    vol = np.asarray(vol)
    nz, ny, nx = vol.shape
    p = positions(dims, matrix, box)
    ok = inside(p)
    if filt == NEAREST:
        raw = np.zeros(ok.shape, vol.dtype)
        pi = p[ok]
        raw[ok] = vol[nearest_index(pi[:, 2], nz), nearest_index(pi[:, 1], ny), nearest_index(pi[:, 0], nx)]
        return raw, ok
    r = np.full(ok.shape, f32(fill), f32)
    if ok.any():
        r[ok] = Wt.filtered(vol, p[ok], Wt.FILTER_TEX8 if filt == TEX8 else Wt.FILTER_EXACT)
    return r


def finish(r, src_dtype, out_type):
    """Rule 4 for an arithmetic result r (float32, storage units of the source)."""
    r = np.asarray(r, f32)
    with np.errstate(all="ignore"):
        if src_dtype == np.float32:
            return r.copy() if out_type == F32 else HM.bins(r)
        if out_type == F32:
            return r / f32(255)                                 # IEEE division
        s = r + f32(0.5)                                        # one binary32 add,
        out = np.zeros(r.shape, np.uint8)                       # NaN, r < 0.5
        mid = (r >= f32(0.5)) & (r < f32(254.5))
        out[mid] = np.trunc(s[mid]).astype(np.int64).astype(np.uint8)      # then truncation
        out[r >= f32(254.5)] = 255
        return out


def resample(vol, dims, matrix=None, filt=TEX8, fill=0.0, out_type=None, box=None):
    """One call: the output volume [bz, by, bx], uint8 or float32."""
    vol = np.asarray(vol)
    assert vol.dtype in (np.uint8, np.float32)
    if out_type is None:
        out_type = U8 if vol.dtype == np.uint8 else F32
    if filt != NEAREST:
        return finish(value(vol, dims, matrix, filt, fill, box), vol.dtype, out_type)
    raw, ok = value(vol, dims, matrix, filt, fill, box)
    filled = finish(np.full(1, fill, f32), vol.dtype, out_type)[0]
    with np.errstate(all="ignore"):
        if vol.dtype == np.float32:
            copied = raw if out_type == F32 else HM.bins(raw)   # f32 -> f32: the pattern, bit for bit
        else:
            copied = raw if out_type == U8 else raw.astype(f32) / f32(255)
    out = np.empty(ok.shape, copied.dtype)
    out[...] = filled
    out.view(np.uint32 if out.dtype == np.float32 else np.uint8)[ok] = copied.view(np.uint32 if out.dtype == np.float32 else np.uint8)[ok]
    return out


def matrix(euler=(0.0, 0.0, 0.0), zoom=1.0, centre=(0.5, 0.5, 0.5), scale=None):
    """vv_resample_matrix in binary64 (math.sin / math.cos on the binary32 arguments), each entry rounded once: float32[12]."""
    e = [float(f32(v)) for v in euler]
    z = float(f32(zoom))
    c = [float(f32(v)) for v in centre]
    s = [1.0, 1.0, 1.0] if scale is None or not any(float(v) != 0.0 for v in scale) else [float(f32(v)) for v in scale]

    def R(axis, a):
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]                   # the plane the axis turns: Rx (y, z), Ry (z, x), Rz (x, y)
        m[i, i] = m[j, j] = math.cos(a)
        m[i, j], m[j, i] = -math.sin(a), math.sin(a)
        return m

    Rm = R(2, e[2]) @ R(1, e[1]) @ R(0, e[0])
    A = np.array([[Rm[r, k] * (s[k] / s[r]) / z for k in range(3)] for r in range(3)])
    t = np.array(c) - A @ np.array([0.5, 0.5, 0.5])
    return np.concatenate([A, t[:, None]], axis=1).reshape(12).astype(f32)


def same(got, want):
    """Exact: bytes, or uint32 patterns, except that a NaN on both sides is equal whatever its pattern where `got` is an arithmetic result (the
    caller compares copies with tobytes()).  Returns the indices that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.uint8:
        return np.argwhere(got != want)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    return np.argwhere((g != w) & ~(np.isnan(got) & np.isnan(want)))
