"""A second, independent statement of the ray march, the MIP frame and the slice sampler: plain numpy over whole frames.

Written from the reference's kernel.cu / implicit.cu / slicekernel.cu / firstpass.vert, DESIGN.md sections 3 and 4c and
include/volviz.h.  Where the oracle works block by block with 32-deep caches, this model lists every ray of the frame once --
one entry per (slab, footprint pixel) -- and holds everything as flat arrays indexed by (ray, chunk, sample); there are no
caches: a Phong neighbour is another entry of the same list.

Arithmetic is binary32: every operation below is one IEEE operation on numpy float32 arrays.  The fused multiply-add numpy
lacks is `fma`: exact product in binary64, TwoSum with the addend, rounding to odd, one narrowing.

Plain numpy arrays and Python numbers in and out.  Volumes are [nz, ny, nx] uint8 or float32, tables float32[1024],
frames uint8 [H, W, 4] with row 0 at the bottom."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
SLICE_NONE, SLICE_PLANE, SLICE_PLANE_CUT = -1, 0, 1
HORIZONTAL, SAGITTAL, CORONAL, FREE_FORM = 0, 1, 2, 4
FILTER_TEX8, FILTER_EXACT = 0, 1
ERT_REFERENCE, ERT_TRUE = 0, 1
SLAB = 14                                   # kernel.cu:418: 16 x 16 threads, the inner 14 x 14 own pixels
CHUNK = 32                                  # kernel.cu:24
SQRT_3 = f32(1.73205081)


# ---------------------------------------------------------------------------------------------------------------------
# binary32 helpers
# ---------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: a * b is exact in binary64 (two 24-bit factors), TwoSum gives the sum and
    its error, and a sum whose last bit is even moves one ulp towards a non-zero error (rounding to odd: the binary64
    result then narrows to binary32 as the exact value would)."""
    a = np.asarray(a, f32); b = np.asarray(b, f32); c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        s = np.array(s, np.float64, ndmin=1)
        e = np.broadcast_to(e, s.shape)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        r = s.astype(f32)
    return r.reshape(np.broadcast(a, b, c).shape)


def _vlen(v):
    """kernel.cu:53-57."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.sqrt(x * x + y * y + z * z)


def _dot(a, b):
    """helper_math.h dot: left to right."""
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _clamp(v, lo, hi):
    """helper_math.h clamp = fmaxf(lo, fminf(v, hi))."""
    return np.fmax(f32(lo), np.fmin(v, f32(hi)))


def _in_bounds(p):
    """kernel.cu:65-71; false for NaN."""
    with np.errstate(invalid="ignore"):
        return np.all((p < f32(1)) & (p >= f32(0)), axis=-1)


def _sat_u8(v):
    """float -> unsigned char: truncation, saturation to [0, 255], NaN -> 0."""
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, np.fmin(v, f32(255)), f32(0))
    return v.astype(np.int32).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 1. texture model (pin 2)
# ---------------------------------------------------------------------------------------------------------------------
def _axis(x, n, filt):
    """lower texel, upper texel (both clamped), weight; and the weight as an integer 0..256 (TEX8 only)."""
    xb = fma(x, f32(n), f32(-0.5))
    fl = np.floor(xb)
    w = xb - fl
    k = None
    if filt == FILTER_TEX8:
        r = np.rint(w * f32(256))                               # ties to even
        k = r.astype(np.int64)
        w = r * f32(1.0 / 256.0)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), w, k


def _corners(vol, ax, ay, az):
    (x0, x1, _, _), (y0, y1, _, _), (z0, z1, _, _) = ax, ay, az
    return [[[vol[z, y, x] for x in (x0, x1)] for y in (y0, y1)] for z in (z0, z1)]     # [z][y][x]


def filtered(vol, p, filt=FILTER_TEX8):
    """The trilinear value at normalised coordinates p [..., 3] in storage units (0..255 for u8 volumes), binary32:
    lerps in x, then y, then z, each fma(w, b - a, a)."""
    nz, ny, nx = vol.shape
    with np.errstate(invalid="ignore"):
        p = np.where(np.isfinite(p), p, f32(0)).astype(f32)
    ax, ay, az = _axis(p[..., 0], nx, filt), _axis(p[..., 1], ny, filt), _axis(p[..., 2], nz, filt)
    c = _corners(vol, ax, ay, az)
    c = [[[v.astype(f32) for v in row] for row in pl] for pl in c]
    wx, wy, wz = ax[2], ay[2], az[2]
    lx = [[fma(wx, c[z][y][1] - c[z][y][0], c[z][y][0]) for y in (0, 1)] for z in (0, 1)]
    ly = [fma(wy, lx[z][1] - lx[z][0], lx[z][0]) for z in (0, 1)]
    return fma(wz, ly[1] - ly[0], ly[0])


def tex3d(vol, p, filt=FILTER_TEX8):
    """tex3D as the slice kernels read it: u8 volumes are normalised after filtering (L / 255)."""
    L = filtered(vol, p, filt)
    return L / f32(255) if vol.dtype == np.uint8 else L


def index_int(vol, p):
    """u8 volumes under TEX8, integers only: weights 0..256, the trilinear value as an exact numerator over 2^24, one
    round-to-nearest-even to 24 significant bits, truncation.  (The first two lerp stages need 16 and 24 bits and are
    exact in binary32; only the last one rounds.)"""
    assert vol.dtype == np.uint8
    nz, ny, nx = vol.shape
    with np.errstate(invalid="ignore"):
        p = np.where(np.isfinite(p), p, f32(0)).astype(f32)
    ax, ay, az = _axis(p[..., 0], nx, FILTER_TEX8), _axis(p[..., 1], ny, FILTER_TEX8), _axis(p[..., 2], nz, FILTER_TEX8)
    c = _corners(vol, ax, ay, az)
    kx, ky, kz = ax[3], ay[3], az[3]
    num = np.zeros(kx.shape, np.int64)
    for z in (0, 1):
        for y in (0, 1):
            for x in (0, 1):
                wgt = (kx if x else 256 - kx) * (ky if y else 256 - ky) * (kz if z else 256 - kz)
                num += c[z][y][x].astype(np.int64) * wgt
    shift = np.zeros(num.shape, np.int64)                       # bits beyond 24 significant ones (num < 2^32)
    for k in range(8):
        shift += num >= (1 << (24 + k))
    q = num >> shift
    rem = num - (q << shift)
    half = np.where(shift > 0, np.int64(1) << np.maximum(shift - 1, 0), np.int64(0))
    up = (shift > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    val = (q + up) << shift
    return (val >> 24).astype(np.uint8)


def classify(vol, p, filt=FILTER_TEX8):
    """kernel.cu:99-105 sample(): the 8-bit index at texture coordinates p, 0 outside [0, 1)^3."""
    L = filtered(vol, p, filt)
    idx = _sat_u8(L if vol.dtype == np.uint8 else f32(255) * L)
    return np.where(_in_bounds(p), idx, np.uint8(0))


def _to_tex(pos, inv_scale):
    """(pos - .5) / scale + .5 in its reciprocal form (pin 3)."""
    return fma(pos - f32(0.5), inv_scale, f32(0.5))


def _inv_scale(scale):
    return f32(1) / np.asarray(scale, f32)


# ---------------------------------------------------------------------------------------------------------------------
# 2. slice sampler
# ---------------------------------------------------------------------------------------------------------------------
def _slice_store(buf, height, width, values):
    j, i = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    off = j * height + i                                        # `height` is the row stride (pin 9)
    ok = off < height * width                                   # elements past the buffer are skipped
    buf[off[ok]] = values[ok]                                   # rows overlap when width > height: the later row wins
    return buf


def slice_canonical(vol, height, width, dx=0.0, dy=0.0, dz=0.0, orientation=SAGITTAL, scale=(1, 1, 1), legacy=False,
                    filt=FILTER_TEX8, fill=0.0):
    """kernel.cu:543-597; legacy = the 4-argument slicekernel.cu:51-82 (no orientation, scale or bounds check)."""
    u = (np.arange(width, dtype=f32) / f32(width))[None, :] + np.zeros((height, 1), f32)
    w = (np.arange(height, dtype=f32) / f32(height))[:, None] + np.zeros((1, width), f32)
    zero = np.zeros((height, width), f32)
    if legacy or orientation == SAGITTAL:
        pos = [u, w, zero]
    elif orientation == HORIZONTAL:
        pos = [w, zero, u]
    elif orientation == CORONAL:
        pos = [zero, w, u]
    else:                                                       # FREE_FORM: no case of the switch
        pos = [zero, zero, zero]
    pos = np.stack([pos[0] + f32(dx), pos[1] + f32(dy), pos[2] + f32(dz)], axis=-1)
    if legacy:
        val = tex3d(vol, pos, filt)
    else:
        p = _to_tex(pos, _inv_scale(scale))
        val = np.where(_in_bounds(p), tex3d(vol, p, filt), f32(0))
    return _slice_store(np.full(height * width, fill, f32), height, width, val)


def slice_advanced(vol, height, width, trans, scale=(1, 1, 1), filt=FILTER_TEX8, fill=0.0):
    """kernel.cu:599-644: the row-major 4 x 4 transform of (i / width, j / height, .5, 1), divided by the scale twice."""
    t = np.asarray(trans, f32).reshape(16)
    rx = (np.arange(width, dtype=f32) / f32(width))[None, :] + np.zeros((height, 1), f32)
    ry = (np.arange(height, dtype=f32) / f32(height))[:, None] + np.zeros((1, width), f32)
    rz, rw = f32(0.5), f32(1)
    inv = _inv_scale(scale)
    rows = [t[4 * r] * rx + t[4 * r + 1] * ry + t[4 * r + 2] * rz + t[4 * r + 3] * rw for r in range(3)]
    pos = np.stack(rows, axis=-1) * inv
    p = _to_tex(pos, inv)
    val = np.where(_in_bounds(p), tex3d(vol, p, filt), f32(0))
    return _slice_store(np.full(height * width, fill, f32), height, width, val)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ray set-up
# ---------------------------------------------------------------------------------------------------------------------
def _norm3(v):
    return v / _vlen(v)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def analytic_endpoints(W, H, x, y, origin, look, up, fov_y, scale, aspect=0.0, quantize8=False):
    """The analytic first pass (a project definition: the reference rasterises the cube with GL, firstpass.vert:6): the ray
    through the centre of pixel (x, y) under perspective(fovY, aspect) and the look-at basis, cut with the box
    [-scale, scale], in cube space world / 2 + .5; (0, 0, 0) where the face is not visible."""
    look = _norm3(np.asarray(look, f32)); up0 = np.asarray(up, f32)
    side = _norm3(_cross(look, up0))
    upv = _norm3(_cross(side, look))
    asp = f32(aspect) if aspect > 0 else f32(W) / f32(H)
    th = f32(math.tan(float(f32(fov_y)) * math.pi / 360.0))
    ndx = (f32(2) * (x.astype(f32) + f32(0.5))) / f32(W) - f32(1)
    ndy = (f32(2) * (y.astype(f32) + f32(0.5))) / f32(H) - f32(1)
    sx = ndx * (th * asp); sy = ndy * th
    d = (side[None, :] * sx[:, None] + upv[None, :] * sy[:, None]) + look[None, :]
    o = np.asarray(origin, f32); sc = np.asarray(scale, f32)
    tmin = np.full(x.shape, -np.inf, f32); tmax = np.full(x.shape, np.inf, f32)
    miss = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            da = d[:, a]
            t1 = (-sc[a] - o[a]) / da; t2 = (sc[a] - o[a]) / da
            nz = da != 0
            tmin = np.where(nz, np.fmax(tmin, np.fmin(t1, t2)), tmin)
            tmax = np.where(nz, np.fmin(tmax, np.fmax(t1, t2)), tmax)
            miss |= ~nz & ((o[a] < -sc[a]) | (o[a] > sc[a]))
        hit_b = ~miss & (tmin <= tmax) & (tmax > 0)
        hit_f = hit_b & (tmin > 0)
        pb = (o[None, :] + d * tmax[:, None]) * f32(0.5) + f32(0.5)
        pf = (o[None, :] + d * tmin[:, None]) * f32(0.5) + f32(0.5)
    back = np.where(hit_b[:, None], pb, f32(0)).astype(f32)
    front = np.where(hit_f[:, None], pf, f32(0)).astype(f32)
    if quantize8:                                               # GL float -> UNORM8, then kernel.cu:320-321
        front = np.floor(_clamp(front, 0, 1) * f32(255) + f32(0.5)) / f32(255)
        back = np.floor(_clamp(back, 0, 1) * f32(255) + f32(0.5)) / f32(255)
    return front, back


def image_endpoints(W, H, x, y, front_img, back_img):
    """kernel.cu:317-321: point sampling at (x / W, y / H), bytes / 255."""
    ih, iw = front_img.shape[:2]
    tx = np.clip(np.floor((x.astype(f32) / f32(W)) * f32(iw)).astype(np.int64), 0, iw - 1)
    ty = np.clip(np.floor((y.astype(f32) / f32(H)) * f32(ih)).astype(np.int64), 0, ih - 1)
    return (front_img[ty, tx, :3].astype(f32) / f32(255)), (back_img[ty, tx, :3].astype(f32) / f32(255))


def frame_rays(W, H, slab_rows=(0, 0), shard=None):
    """Every ray of the frame, one per (slab, footprint pixel), slabs in launch order (kernel.cu:294-315).  Returns a dict
    of flat arrays: slab (by * nbx + bx), x, y, sx, sy (position inside the footprint), fw, fh (footprint size), lone (an
    empty footprint, W or H = 1: blockMin's loop is empty and the radius is the ray's own), owned (the slab writes the
    pixel: a non-border thread lands on it, no higher slab does (pin 10), and its row passes the slab-row predicates of
    include/volviz.h, which go by the pixel row's slab row y / 14)."""
    nbx, nby = -(-W // SLAB), -(-H // SLAB)
    keys = ("slab", "x", "y", "sx", "sy", "fw", "fh", "lone", "owned")
    out = {k: [] for k in keys}
    begin, end = slab_rows
    top = {}                                                    # pixel -> the highest slab that lands a non-border thread on it
    blocks = []
    t = np.arange(16)
    inner = (t >= 1) & (t <= 14)
    for by in range(nby):
        for bx in range(nbx):
            lox, loy = max(bx * SLAB - 1, 0), max(by * SLAB - 1, 0)
            upx, upy = min((bx + 1) * SLAB + 1, W - 1), min((by + 1) * SLAB + 1, H - 1)
            tx = np.maximum(lox, np.minimum(bx * SLAB + t - 1, upx - 1))       # clamp(x, slabLower, slabUpper - 1) = max(lo, min(x, hi))
            ty = np.maximum(loy, np.minimum(by * SLAB + t - 1, upy - 1))
            lone = upx - lox <= 0 or upy - loy <= 0
            xr = np.unique(tx); yr = np.unique(ty)              # the footprint = what the 16 x 16 threads land on
            ys, xs = np.meshgrid(yr, xr, indexing="ij")
            hit = np.isin(ys, ty[inner]) & np.isin(xs, tx[inner])
            for y, x in zip(ys[hit].tolist(), xs[hit].tolist()):
                top[(y, x)] = by * nbx + bx
            blocks.append((by * nbx + bx, xs, ys, hit, lone))
    for slab, xs, ys, hit, lone in blocks:
        r = ys // SLAB
        own = hit & np.array([[top.get((y, x)) == slab for y, x in zip(ry, rx)] for ry, rx in zip(ys.tolist(), xs.tolist())], bool).reshape(hit.shape)
        if not (begin == 0 and end == 0):
            own &= (r >= begin) & (r < end)
        if shard is not None and shard[1] > 1:
            own &= (r // shard[0]) % shard[1] == shard[2]
        if not own.any():
            continue
        n = xs.size
        fh, fw = xs.shape
        out["slab"].append(np.full(n, slab)); out["x"].append(xs.ravel()); out["y"].append(ys.ravel())
        out["sx"].append((xs - xs.min()).ravel()); out["sy"].append((ys - ys.min()).ravel())
        out["fw"].append(np.full(n, fw)); out["fh"].append(np.full(n, fh)); out["lone"].append(np.full(n, lone)); out["owned"].append(own.ravel())
    return {k: (np.concatenate(v) if v else np.zeros(0, bool if k in ("owned", "lone") else np.int64)) for k, v in out.items()}


def setup(R, front, back, cam_origin, step, slice_type, plane):
    """kernel.cu:320-357 and the head of mainLoop (:218-246) for every ray of R.  Adds origin, dir, sdir, sstep, upper,
    dist0, dead (zero-length interior ray: the pixel is (0,0,0,0)), cut (the cut plane's early return)."""
    cam = np.asarray(cam_origin, f32)
    with np.errstate(all="ignore"):
        cam_len = _vlen(front - cam[None, :])
        rad = np.full(int(R["slab"].max()) + 1 if len(cam_len) else 0, np.inf, f32)
        np.minimum.at(rad, R["slab"], cam_len)                  # blockMin over the slab's clamped apron footprint
        rad = np.where(R["lone"], cam_len, rad[R["slab"]])
        d = back - front
        length = _vlen(d)
        ray = d / length[:, None]
        l0p0 = front - cam[None, :]                             # implicit.cu:19-35 with l = -ray
        b = _dot(-ray, l0p0)
        c = _dot(l0p0, l0p0) - rad * rad
        disc = b * b - c
        t = b * f32(-1) - np.sqrt(disc)
        ok = (disc >= 0) & (t.astype(np.float64) > -1e-6)
        pos = np.where(ok[:, None], front - ray * t[:, None], front)
        upper = np.fmin(SQRT_3, _vlen(back - pos))
        sdir = ray * np.asarray(step, f32)[None, :]
        sstep = _vlen(sdir)
        dist0 = np.zeros(len(upper), f32)
        cut = np.zeros(len(upper), bool)
        if slice_type == SLICE_PLANE_CUT:
            p0 = np.asarray(plane[:3], f32)[None, :]; n = np.asarray(plane[3:], f32)[None, :]
            bk = pos + ray * upper[:, None]
            cut = (_dot(n, pos - p0).astype(np.float64) < 1e-6) & (_dot(n, bk - p0).astype(np.float64) < 1e-6)
            den = _dot(n, ray)
            t1 = _dot(p0 - pos, n) / den
            hit1 = (den.astype(np.float64) > 1e-6) & (t1 >= 0)
            nray = ray * f32(-1)
            den2 = _dot(n, nray)
            t2 = _dot(p0 - bk, n) / den2
            hit2 = ~hit1 & (den2.astype(np.float64) > 1e-6) & (t2 >= 0)
            dist0 = np.where(hit1 & ~cut, t1, dist0).astype(f32)
            upper = np.where(hit2 & ~cut, upper - t2, upper).astype(f32)
        dead = length < f32(0.001)
    R.update(origin=pos.astype(f32), dir=ray.astype(f32), sdir=sdir.astype(f32), sstep=sstep.astype(f32),
             upper=upper.astype(f32), dist0=dist0, dead=dead, cut=cut)
    return R


# ---------------------------------------------------------------------------------------------------------------------
# 4.-6. the march
# ---------------------------------------------------------------------------------------------------------------------
def _chunk_indices(vol, R, dist, inv_scale, filt, both_paths, visit=None):
    """The 32 classification indices of every ray's chunk starting at `dist` (kernel.cu:126-145: the position accumulates
    one step at a time); [rays, 32].  `visit`, if given, is called with the chunk's texture coordinates [rays, 32, 3]."""
    n = len(dist)
    pos = np.empty((n, CHUNK, 3), f32)
    with np.errstate(all="ignore"):
        p = R["origin"] + R["dir"] * dist[:, None]
        for i in range(CHUNK):
            pos[:, i] = p
            p = p + R["sdir"]
        tp = _to_tex(pos, inv_scale)
    if visit is not None:
        visit(tp)
    idx = classify(vol, tp, filt)
    if both_paths is not None and vol.dtype == np.uint8 and filt == FILTER_TEX8:
        alt = np.where(_in_bounds(tp), index_int(vol, tp), np.uint8(0))
        both_paths["samples"] += idx.size
        both_paths["differ"] += int((alt != idx).sum())
    return idx                                                  # a zero-length ray has a NaN direction: out of bounds, 0 (pin 7)


def render(vol, tf, W, H, *, cam_origin, look=None, up=(0, 1, 0), fov_y=45.0, fov_x=None, scale=(1, 1, 1), aspect=0.0, quantize8=False,
           images=None, slice_type=SLICE_NONE, plane=(.5, .5, .5, 0, 0, 1), phong=False, step=None, ert_threshold=0.0,
           filt=FILTER_TEX8, ert_mode=ERT_REFERENCE, slab_rows=(0, 0), shard=None, fill=0, mip=False, both_paths=None, visit=None):
    """One frame.  Compositing: (rgba [H, W, 4] uint8 over `fill`, executed samples).  mip=True: (rgba, index [H, W] uint8,
    executed samples) of the maximum-intensity projection.  `both_paths`: a dict with "samples" and "differ"
    that receives the comparison of the fma path with the integer path on every u8 / TEX8 sample.  `visit`: called once per
    chunk with (texture coordinates [rays, 32, 3] of the rays that march, executed [rays, 32] bool: the samples of the chunk
    that ran, started [rays] bool: the rays that began the chunk); nothing the frame returns depends on it."""
    nz, ny, nx = vol.shape
    table = np.ascontiguousarray(tf, f32).reshape(256, 4)
    if step is None or not np.any(np.asarray(step, f32) != 0):
        step = f32(1) / np.array([nx, ny, nz], f32)              # kernel.cu:415
    else:
        step = np.asarray([step] * 3 if np.isscalar(step) else step, f32)
    thr = f32(ert_threshold) if ert_threshold != 0 else f32(0.95)
    if mip and slice_type == SLICE_PLANE:
        slice_type = SLICE_NONE
    rgba = np.full((H, W, 4), fill, np.uint8)
    index_img = np.full((H, W), fill, np.uint8)
    R = frame_rays(W, H, slab_rows, shard)
    if len(R["x"]) == 0:
        return (rgba, index_img, 0) if mip else (rgba, 0)
    if images is not None:
        front, back = image_endpoints(W, H, R["x"], R["y"], images[0], images[1])
    else:
        if look is None:
            look = -np.asarray(cam_origin, f32)
        front, back = analytic_endpoints(W, H, R["x"], R["y"], cam_origin, look, up, fov_y, scale, aspect, quantize8)
    setup(R, front, back, cam_origin, step, slice_type, plane)
    inv_scale = _inv_scale(scale)
    n = len(R["x"])
    live = ~R["dead"] & ~R["cut"] & R["owned"]                  # rays that composite
    march = np.ones(n, bool) if phong else R["owned"]           # rays whose samples anybody reads
    sub = {k: v[march] for k, v in R.items()}
    pos_of = np.full(n, -1); pos_of[march] = np.arange(int(march.sum()))
    res = np.zeros((n, 4), f32)
    best = np.zeros(n, np.int32)
    count = 0
    dist = R["dist0"].copy()
    stopped = np.zeros(n, bool)                                 # ERT_TRUE
    p0 = np.asarray(plane[:3], f32)[None, :]; pn = np.asarray(plane[3:], f32)[None, :]
    if phong:
        fov_x = f32(fov_y) * (f32(W) / f32(H)) if fov_x is None else f32(fov_x)         # glwidget.cpp:341
        tan_x = f32(math.tan(float(fov_x) * math.pi / float(f32(180) * f32(W))))           # kernel.cu:221-222, in double
        tan_y = f32(math.tan(float(f32(fov_y)) * math.pi / float(f32(180) * f32(H))))
        # neighbours inside the same slab's footprint, +-1 clamped to it (pin 6); rays of a slab are contiguous, row-major
        base = np.arange(n) - (R["sy"] * R["fw"] + R["sx"])
        def nb(dx, dy):
            sx = np.clip(R["sx"] + dx, 0, R["fw"] - 1); sy = np.clip(R["sy"] + dy, 0, R["fh"] - 1)
            return base + sy * R["fw"] + sx
        n_l, n_r, n_t, n_b = nb(-1, 0), nb(1, 0), nb(0, 1), nb(0, -1)
    with np.errstate(all="ignore"):
        while True:
            active = live & ~stopped & (dist < R["upper"])      # `while (dist < upper)`
            if not active.any():
                break
            idx = np.zeros((n, CHUNK), np.uint8)
            seen = []                                           # visit: the chunk's texture coordinates and which of its samples ran
            idx[march] = _chunk_indices(vol, sub, dist[march], inv_scale, filt, both_paths, seen.append if visit is not None else None)
            ran = np.zeros((n, CHUNK), bool) if visit is not None else None
            running = active.copy()                             # inside the 30-sample loop of this chunk
            for i in range(1, CHUNK - 1):
                vd = f32(i) * R["sstep"] + dist
                running &= ~(vd > R["upper"])
                if not running.any():
                    break
                count += int(running.sum())
                if ran is not None:
                    ran[:, i] = running
                if mip:
                    best = np.where(running, np.maximum(best, idx[:, i]), best)
                    continue
                val = table[idx[:, i]].copy()
                if phong:
                    lit = running & (val[:, 3].astype(np.float64) > 1e-6)
                    f_ = idx[:, i - 1].astype(f32) / f32(255); a_ = idx[:, i + 1].astype(f32) / f32(255)
                    l_ = idx[n_l, i].astype(f32) / f32(255); r_ = idx[n_r, i].astype(f32) / f32(255)
                    t_ = idx[n_t, i].astype(f32) / f32(255); b_ = idx[n_b, i].astype(f32) / f32(255)
                    g = np.stack([(r_ - l_) / (tan_x * vd), (t_ - b_) / (tan_y * vd), (a_ - f_) / (R["sstep"] * f32(2))], axis=-1)
                    nzero = np.all(g != 0, axis=-1)
                    inv_len = f32(1) / np.sqrt(_dot(g, g))
                    g = np.where(nzero[:, None], g * inv_len[:, None], g)
                    direct = _clamp((g[:, 0] * f32(-1) + g[:, 1] * f32(-1) + g[:, 2] * f32(1)) * f32(0.3), 0, 0.3)
                    shaded = val.copy()
                    shaded[:, :3] = val[:, :3] * f32(0.7) + direct[:, None]
                    val = np.where(lit[:, None], shaded, val)
                if slice_type == SLICE_PLANE:
                    vp = R["origin"] + R["dir"] * vd[:, None]
                    pd = np.abs(_dot(pn, vp - p0))
                    hl = _clamp(val[:, 0] + (f32(0.01) - pd) * f32(100), 0, 1)
                    val[:, 0] = np.where(pd < f32(0.01), hl, val[:, 0])
                do = running & (val[:, 3].astype(np.float64) > 1e-6)
                bf = val[:, 3] * (f32(1) - res[:, 3])
                new = np.concatenate([res[:, :3] + val[:, :3] * bf[:, None], (res[:, 3] + bf)[:, None]], axis=1)
                res = np.where(do[:, None], new, res)
                over = running & (res[:, 3] > thr)
                running &= ~over                                # `break` leaves the inner loop only (pin 4)
                if ert_mode == ERT_TRUE:
                    stopped |= over
            if visit is not None:
                visit(seen[0], ran[march], active[march])
            dist = dist + R["sstep"] * f32(30)
    own = R["owned"]
    px, py = R["x"][own], R["y"][own]
    if mip:
        lut = (np.clip(table, f32(0), f32(1)) * f32(255)).astype(np.uint8)
        index_img[py, px] = best[own].astype(np.uint8)          # slabs in launch order: the higher one wins (pin 10)
        rgba[py, px] = lut[best[own]]
        return rgba, index_img, count
    out = _sat_u8(_clamp(res, 0, 1) * f32(255))
    rgba[py, px] = out[own]
    return rgba, count
