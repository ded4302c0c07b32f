"""The isosurface frame of include/volviz.h (vv_render_iso) as plain numpy over whole frames (test infrastructure only).

Built from the witness's ray list, end points, ray set-up, texture-coordinate mapping and classification (tests/witness.py,
imported and unchanged); what this file adds is the contract's own text: the first executed sample, in march order, whose
8-bit index reaches the level; the march's accumulated position and the ordinal of that sample; six more samples around it
and the headlight shade.  Every operation is one IEEE binary32 operation on numpy float32 arrays, in the order the contract
writes it.  No kernel of the product appears here."""
from __future__ import annotations

import numpy as np

from witness import (SLICE_NONE, SLICE_PLANE, FILTER_TEX8, _dot, _to_tex, analytic_endpoints, classify, f32, frame_rays,
                     image_endpoints, setup)

SAMPLES = 30                                    # kernel.cu:25: samples per chunk


def pack(v):
    """pack_rgba's conversion of one channel: (uint8)(fmaxf(0, fminf(v, 1)) * 255), truncating."""
    with np.errstate(invalid="ignore"):
        return (np.fmax(f32(0), np.fmin(np.asarray(v, f32), f32(1))) * f32(255)).astype(np.int32).astype(np.uint8)


def shade_of(g, inv_scale, dims, direction):
    """shade [n] float32 from the index differences g [n, 3] (integers), 1 / scale [3], the volume's dimensions (nx, ny, nz)
    and the rays' directions [n, 3]: G_a = ((float)g_a * inv_scale[a]) * (float)n_a, diffuse = |G . dir| / |G| clamped to 1
    (0 where |G| = 0), shade = 0.3 + 0.7 * diffuse."""
    inv_scale = np.asarray(inv_scale, f32); nf = np.asarray(dims, np.int64).astype(f32)
    with np.errstate(all="ignore"):
        G = (np.asarray(g).astype(f32) * inv_scale[None, :]) * nf[None, :]
        dp = _dot(G, np.asarray(direction, f32))
        ln = np.sqrt(_dot(G, G))
        diffuse = np.where(ln > 0, np.fmin(np.abs(dp) / ln, f32(1)), f32(0)).astype(f32)
        return (f32(0.3) + f32(0.7) * diffuse).astype(f32)


def gradient(vol, t, filt=FILTER_TEX8):
    """g [n, 3] int32: k(t + h_a e_a) - k(t - h_a e_a) with h_a = 1.0f / (float)n_a, through the march's classification
    (0 outside [0, 1)^3)."""
    nz, ny, nx = vol.shape
    g = np.zeros((len(t), 3), np.int32)
    for a, n in enumerate((nx, ny, nz)):
        h = f32(1) / f32(n)
        hi = t.copy(); hi[:, a] = t[:, a] + h
        lo = t.copy(); lo[:, a] = t[:, a] - h
        g[:, a] = classify(vol, hi, filt).astype(np.int32) - classify(vol, lo, filt).astype(np.int32)
    return g


def render(vol, tf, W, H, level, *, cam_origin, look=None, up=(0, 1, 0), fov_y=45.0, scale=(1, 1, 1), aspect=0.0, quantize8=False,
           images=None, slice_type=SLICE_NONE, plane=(.5, .5, .5, 0, 0, 1), step=None, filt=FILTER_TEX8, slab_rows=(0, 0), shard=None,
           fill=0):
    """One isosurface frame.  Returns a dict: rgba [H, W, 4] uint8, index [H, W] uint8 and hit [H, W, 4] float32, each over
    `fill` bytes; written [H, W] bool; count, the samples executed; and, for the tests' own conditions, shade [H, W] float32
    (NaN where there is no hit) and g [H, W, 3] int32."""
    assert 1 <= level <= 255
    nz, ny, nx = vol.shape
    table = np.ascontiguousarray(tf, f32).reshape(256, 4)
    if step is None or not np.any(np.asarray(step, f32) != 0):
        step = f32(1) / np.array([nx, ny, nz], f32)
    else:
        step = np.asarray([step] * 3 if np.isscalar(step) else step, f32)
    if slice_type == SLICE_PLANE:
        slice_type = SLICE_NONE
    out = dict(rgba=np.full((H, W, 4), fill, np.uint8), index=np.full((H, W), fill, np.uint8),
               hit=np.full((H, W, 16), fill, np.uint8).view(f32), written=np.zeros((H, W), bool), count=0,
               shade=np.full((H, W), np.nan, f32), g=np.zeros((H, W, 3), np.int32))
    R = frame_rays(W, H, slab_rows, shard)
    if len(R["x"]) == 0:
        return out
    if images is not None:
        front, back = image_endpoints(W, H, R["x"], R["y"], images[0], images[1])
    else:
        if look is None:
            look = -np.asarray(cam_origin, f32)
        front, back = analytic_endpoints(W, H, R["x"], R["y"], cam_origin, look, up, fov_y, scale, aspect, quantize8)
    setup(R, front, back, cam_origin, step, slice_type, plane)
    inv_scale = f32(1) / np.asarray(scale, f32)
    own = R["owned"]
    R = {k: v[own] for k, v in R.items()}                      # the radius is the slab's (set-up saw every ray); only owned rays march
    n = len(R["x"])
    found = np.zeros(n, bool)
    k_hit = np.zeros(n, np.uint8)
    ordinal = np.zeros(n, np.int64)                             # samples executed so far; at the end: up to and including the hit
    pos_hit = np.zeros((n, 3), f32)
    dist = R["dist0"].copy()
    alive = ~R["dead"] & ~R["cut"]
    with np.errstate(all="ignore"):
        while True:
            act = np.flatnonzero(alive & ~found & (dist < R["upper"]))          # `while (dist < upper)`
            if len(act) == 0:
                break
            d = dist[act]; sstep = R["sstep"][act]; upper = R["upper"][act]; sdir = R["sdir"][act]
            p = R["origin"][act] + R["dir"][act] * d[:, None]
            pos = np.empty((len(act), SAMPLES, 3), f32)
            for i in range(SAMPLES):                            # the position accumulates one step per sample
                p = p + sdir
                pos[:, i] = p
            i1 = np.arange(1, SAMPLES + 1, dtype=f32)[None, :]
            stop = (i1 * sstep[:, None] + d[:, None]) > upper[:, None]           # the sample is executed unless this, or an earlier one, holds
            runs = np.cumsum(stop, axis=1) == 0
            k = classify(vol, _to_tex(pos, inv_scale), filt)
            is_hit = runs & (k >= level)
            has = is_hit.any(axis=1)
            first = np.argmax(is_hit, axis=1)
            executed = np.where(has, first + 1, runs.sum(axis=1))
            ordinal[act] += executed
            rows = np.flatnonzero(has)
            found[act[rows]] = True
            k_hit[act[rows]] = k[rows, first[rows]]
            pos_hit[act[rows]] = pos[rows, first[rows]]
            dist[act] = d + sstep * f32(SAMPLES)
        out["count"] = int(ordinal.sum())
        hit = np.zeros((n, 4), f32)
        hit[found, :3] = pos_hit[found]
        hit[found, 3] = ordinal[found].astype(f32)
        rgba = np.zeros((n, 4), np.uint8)
        shade = np.full(n, np.nan, f32)
        g = np.zeros((n, 3), np.int32)
        if found.any():
            g[found] = gradient(vol, _to_tex(pos_hit[found], inv_scale), filt)
            shade[found] = shade_of(g[found], inv_scale, (nx, ny, nz), R["dir"][found])
            e = table[k_hit[found]]
            rgba[found, :3] = pack(e[:, :3] * shade[found][:, None])
            rgba[found, 3] = pack(f32(1))
    y, x = R["y"], R["x"]
    out["written"][y, x] = True
    out["index"][y, x] = k_hit
    out["hit"][y, x] = hit
    out["rgba"][y, x] = rgba
    out["shade"][y, x] = shade
    out["g"][y, x] = g
    return out


def render_cam(vol, tf, W, H, cam, level, *, slice_type=SLICE_NONE, plane=(.5, .5, .5, 0, 0, 1), **kw):
    """render() for a camera object with origin, look(), up, fov_y and scale (the binding's Camera)."""
    return render(vol, tf, W, H, level, cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y, scale=cam.scale,
                  slice_type=slice_type, plane=plane, **kw)
