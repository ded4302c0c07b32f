"""The thick-slab slice contract (include/volviz.h: vv_slice_slab / vv_slice_advanced_slab) in numpy, on top of the witness's slice sampler.

A slab is K layers -- per sample k a plane of values and a mask of the pixels whose sample is executed -- and one reduction over them.
Every operation is one IEEE binary32 operation on float32 arrays (witness.py); the reductions walk the layers in order of k.
Volumes are [nz, ny, nx] uint8 or float32; results are the flat buffers the C call fills: float32 values and int32 aux, with `fill` /
`aux_fill` where the kernel stores nothing."""
from __future__ import annotations

import numpy as np

import witness as Wt

f32 = np.float32
SLAB_MAX, SLAB_MIN, SLAB_MEAN = 0, 1, 2
MODES = (SLAB_MAX, SLAB_MIN, SLAB_MEAN)
AXIS_OF = {Wt.SAGITTAL: 2, Wt.HORIZONTAL: 1, Wt.CORONAL: 0}      # the coordinate the orientation switch leaves at 0


def offsets(samples, thickness):
    """o_k = ((float)k - 0.5f * (float)(K - 1)) * (thickness / (float)K), k = 0 .. K - 1, as [K, 1, 1]."""
    spacing = f32(thickness) / f32(samples)
    half = f32(0.5) * f32(samples - 1)
    return ((np.arange(samples, dtype=f32) - half) * spacing).reshape(samples, 1, 1)


def _grid(height, width):
    u = (np.arange(width, dtype=f32) / f32(width))[None, :] + np.zeros((height, 1), f32)
    w = (np.arange(height, dtype=f32) / f32(height))[:, None] + np.zeros((1, width), f32)
    return u, w


def _layer(vol, p, filt):
    ok = Wt._in_bounds(p)
    return np.where(ok, Wt.tex3d(vol, p, filt), f32(0)).astype(f32), ok


def layers_canonical(vol, height, width, dx, dy, dz, orientation, samples, thickness, scale=(1, 1, 1), filt=Wt.FILTER_TEX8):
    """(values [K, height, width], executed [K, height, width]): witness.slice_canonical with the slab axis' displacement d_a + o_k."""
    u, w = _grid(height, width)
    zero = np.zeros((height, width), f32)
    pos = {Wt.SAGITTAL: [u, w, zero], Wt.HORIZONTAL: [w, zero, u], Wt.CORONAL: [zero, w, u]}[orientation]
    a = AXIS_OF[orientation]
    d = [f32(dx), f32(dy), f32(dz)]
    d[a] = d[a] + offsets(samples, thickness)                   # the one add, before anything else
    shape = (samples, height, width)
    p = np.stack([np.broadcast_to(pos[c] + d[c], shape) for c in range(3)], axis=-1)
    return _layer(vol, Wt._to_tex(p, Wt._inv_scale(scale)), filt)


def layers_advanced(vol, height, width, trans, samples, thickness, scale=(1, 1, 1), filt=Wt.FILTER_TEX8):
    """The same for witness.slice_advanced with rz = 0.5f + o_k."""
    t = np.asarray(trans, f32).reshape(16)
    rx, ry = _grid(height, width)
    inv = Wt._inv_scale(scale)
    with np.errstate(all="ignore"):
        rz, rw = f32(0.5) + offsets(samples, thickness), f32(1)
        rows = [t[4 * r] * rx + t[4 * r + 1] * ry + t[4 * r + 2] * rz + t[4 * r + 3] * rw for r in range(3)]
        p = Wt._to_tex(np.stack(rows, axis=-1) * inv, inv)
    return _layer(vol, p, filt)


def reduce(vals, oks, mode):
    """(value [height, width] float32, aux [height, width] int32) of one mode over the layers, in order of k."""
    best = np.zeros(vals.shape[1:], f32)
    arg = np.full(vals.shape[1:], -1, np.int32)
    n = np.zeros(vals.shape[1:], np.int32)
    with np.errstate(all="ignore"):
        for k in range(len(vals)):
            s, ok = vals[k], oks[k]
            if mode == SLAB_MEAN:
                best = np.where(ok, np.where(n == 0, s, best + s), best).astype(f32)
            else:
                take = ok & ((n == 0) | ((s > best) if mode == SLAB_MAX else (s < best)))
                best = np.where(take, s, best).astype(f32)
                arg = np.where(take, np.int32(k), arg)
            n = n + ok.astype(np.int32)
        if mode == SLAB_MEAN:
            return np.where(n > 0, best / np.maximum(n, 1).astype(f32), f32(0)).astype(f32), n
    return best, arg


def store(height, width, value, aux, fill=-3.0, aux_fill=-7):
    """The two buffers as the kernel leaves them (witness._slice_store: stride `height`, later rows win, the tail is skipped)."""
    return (Wt._slice_store(np.full(height * width, fill, f32), height, width, value),
            Wt._slice_store(np.full(height * width, aux_fill, np.int32), height, width, aux))


def slab_canonical(vol, height, width, dx, dy, dz, orientation, mode, samples, thickness, scale=(1, 1, 1), filt=Wt.FILTER_TEX8,
                   fill=-3.0, aux_fill=-7):
    v, a = reduce(*layers_canonical(vol, height, width, dx, dy, dz, orientation, samples, thickness, scale, filt), mode)
    return store(height, width, v, a, fill, aux_fill)


def slab_advanced(vol, height, width, trans, mode, samples, thickness, scale=(1, 1, 1), filt=Wt.FILTER_TEX8, fill=-3.0, aux_fill=-7):
    v, a = reduce(*layers_advanced(vol, height, width, trans, samples, thickness, scale, filt), mode)
    return store(height, width, v, a, fill, aux_fill)
