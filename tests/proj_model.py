"""The projection frame of include/volviz.h (vv_render_projection) as plain numpy over whole frames (test infrastructure only).

Built, like tests/iso_model.py, from the witness's ray list, end points, ray set-up, texture-coordinate mapping, bounds test and
classification (tests/witness.py, imported and unchanged).  What this file adds is the contract's own text: which executed
samples are counted (those whose texture coordinates lie in [0, 1)^3), the maximum / minimum of their indices with the ordinal
of the first sample that attains it, their sum with the mean rounded half up, and the three images.  Integers throughout.
No kernel of the product appears here."""
from __future__ import annotations

import numpy as np

from witness import (SLICE_NONE, SLICE_PLANE, FILTER_TEX8, _in_bounds, _to_tex, analytic_endpoints, classify, f32, frame_rays,
                     image_endpoints, setup)

SAMPLES = 30                                    # kernel.cu:25: samples per chunk
PROJ_MAX, PROJ_MIN, PROJ_MEAN = 0, 1, 2         # include/volviz.h: vv_proj_mode


def rgba_of(tf, v):
    """vv_render_mip's conversion of tf[v]: channel c = (uint8)(clamp(tf[v][c], 0, 1) * 255) in binary32, truncating."""
    t = np.ascontiguousarray(tf, f32).reshape(256, 4)
    with np.errstate(invalid="ignore"):
        lut = (np.fmax(f32(0), np.fmin(t, f32(1))) * f32(255)).astype(np.int32).astype(np.uint8)
    return lut[v]


def mean_half_up(s, n):
    """(2 s + n) / (2 n) in 64-bit integers, truncating; 0 where n == 0."""
    s = np.asarray(s, np.int64); n = np.asarray(n, np.int64)
    return np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), 0)


def owned_rays(dims, W, H, *, cam_origin, look=None, up=(0, 1, 0), fov_y=45.0, scale=(1, 1, 1), aspect=0.0, quantize8=False, images=None,
               slice_type=SLICE_NONE, plane=(.5, .5, .5, 0, 0, 1), step=None, slab_rows=(0, 0), shard=None):
    """The rays of a reducer frame over a volume of dims (nx, ny, nz) that march -- those whose slab writes their pixel -- after the witness's
    set-up, and 1 / scale; (None, None) for a frame without rays.  A highlighted plane (SLICE_PLANE) is ignored, as the reducer frames do."""
    nx, ny, nz = dims
    if step is None or not np.any(np.asarray(step, f32) != 0):
        step = f32(1) / np.array([nx, ny, nz], f32)
    else:
        step = np.asarray([step] * 3 if np.isscalar(step) else step, f32)
    if slice_type == SLICE_PLANE:
        slice_type = SLICE_NONE
    R = frame_rays(W, H, slab_rows, shard)
    if len(R["x"]) == 0:
        return None, None
    if images is not None:
        front, back = image_endpoints(W, H, R["x"], R["y"], images[0], images[1])
    else:
        if look is None:
            look = -np.asarray(cam_origin, f32)
        front, back = analytic_endpoints(W, H, R["x"], R["y"], cam_origin, look, up, fov_y, scale, aspect, quantize8)
    setup(R, front, back, cam_origin, step, slice_type, plane)
    own = R["owned"]
    return {k: v[own] for k, v in R.items()}, f32(1) / np.asarray(scale, f32)      # the radius is the slab's (set-up saw every ray); only owned rays march


def march(R, inv_scale):
    """The march loop of a reducer frame over the rays R, chunk by chunk: yields (act, t, runs) -- the indices of the rays that start the chunk, the
    texture coordinates [len(act), 30, 3] of its samples and which of them are executed [len(act), 30] (a prefix of the chunk).  No ray ends early."""
    dist = R["dist0"].copy()
    alive = ~R["dead"] & ~R["cut"]
    with np.errstate(all="ignore"):
        while True:
            act = np.flatnonzero(alive & (dist < R["upper"]))                   # `while (dist < upper)`
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
            yield act, _to_tex(pos, inv_scale), runs
            dist[act] = d + sstep * f32(SAMPLES)


def render(vol, tf, W, H, mode, *, cam_origin, look=None, up=(0, 1, 0), fov_y=45.0, scale=(1, 1, 1), aspect=0.0, quantize8=False,
           images=None, slice_type=SLICE_NONE, plane=(.5, .5, .5, 0, 0, 1), step=None, filt=FILTER_TEX8, slab_rows=(0, 0), shard=None,
           fill=0):
    """One projection frame.  Returns a dict: rgba [H, W, 4] uint8, index [H, W] uint8 and stat [H, W, 2] uint32, each over `fill`
    bytes; written [H, W] bool; count, the samples executed; and, for the tests' own conditions, e and n [H, W] int64 (executed
    and counted samples per pixel) and ties [H, W] int64 (MAX / MIN: how many counted samples attain the extremum)."""
    assert mode in (PROJ_MAX, PROJ_MIN, PROJ_MEAN)
    nz, ny, nx = vol.shape
    out = dict(rgba=np.full((H, W, 4), fill, np.uint8), index=np.full((H, W), fill, np.uint8),
               stat=np.full((H, W, 8), fill, np.uint8).view(np.uint32), written=np.zeros((H, W), bool), count=0,
               e=np.zeros((H, W), np.int64), n=np.zeros((H, W), np.int64), ties=np.zeros((H, W), np.int64))
    R, inv_scale = owned_rays((nx, ny, nz), W, H, cam_origin=cam_origin, look=look, up=up, fov_y=fov_y, scale=scale, aspect=aspect, quantize8=quantize8,
                              images=images, slice_type=slice_type, plane=plane, step=step, slab_rows=slab_rows, shard=shard)
    if R is None:
        return out
    rays = len(R["x"])
    e = np.zeros(rays, np.int64)                                # executed samples so far
    n = np.zeros(rays, np.int64)                                # counted samples so far
    s = np.zeros(rays, np.int64)                                # MEAN: their sum
    ext = np.zeros(rays, np.int64)                              # MAX / MIN: the extremum so far (meaningful where n > 0),
    ordinal = np.zeros(rays, np.int64)                          # the ordinal of the first sample that attained it,
    ties = np.zeros(rays, np.int64)                             # and how many counted samples equal it
    with np.errstate(all="ignore"):
        for act, t, runs in march(R, inv_scale):
            k = classify(vol, t, filt).astype(np.int64)
            counted = runs & _in_bounds(t)
            for i in range(SAMPLES):                            # march order: a later sample replaces only if strictly better
                c = counted[:, i]; ki = k[:, i]; a = act
                if mode == PROJ_MEAN:
                    s[a] += np.where(c, ki, 0)
                else:
                    first = c & (n[a] == 0)
                    better = c & ~first & ((ki > ext[a]) if mode == PROJ_MAX else (ki < ext[a]))
                    new = first | better
                    same = c & ~new & (ki == ext[a])
                    ext[a] = np.where(new, ki, ext[a])
                    ordinal[a] = np.where(new, e[a] + i + 1, ordinal[a])         # (runs is a prefix: sample i is the (i + 1)-th of the chunk)
                    ties[a] = np.where(new, 1, ties[a] + same)
                n[a] += c
            e[act] += runs.sum(axis=1)
    if mode == PROJ_MEAN:
        v = mean_half_up(s, n)
        first_word = np.where(n > 0, s, 0)
    else:
        v = np.where(n > 0, ext, 0)
        first_word = np.where(n > 0, ordinal, 0)
    assert ((v >= 0) & (v <= 255)).all() and (first_word < 2 ** 32).all()
    y, x = R["y"], R["x"]
    out["count"] = int(e.sum())
    out["written"][y, x] = True
    out["index"][y, x] = v.astype(np.uint8)
    out["stat"][y, x, 0] = first_word.astype(np.uint32)
    out["stat"][y, x, 1] = n.astype(np.uint32)
    out["rgba"][y, x] = rgba_of(tf, v)
    out["e"][y, x] = e
    out["n"][y, x] = n
    out["ties"][y, x] = np.where(n > 0, ties, 0)
    return out


def render_cam(vol, tf, W, H, cam, mode, *, slice_type=SLICE_NONE, plane=(.5, .5, .5, 0, 0, 1), **kw):
    """render() for a camera object with origin, look(), up, fov_y and scale (the binding's Camera)."""
    return render(vol, tf, W, H, mode, cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y, scale=cam.scale,
                  slice_type=slice_type, plane=plane, **kw)
