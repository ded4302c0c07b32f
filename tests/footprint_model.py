"""The memory footprint of a frame as plain numpy (test infrastructure only): what the layouts of a volume hold byte for byte, which bytes
one sample loads from each, and from these the three instruments of an instrumented frame that the roofline's denominators are read from
(vv_render_options: touched_bricks, touched_lines, touched_block_lines).

Written from the text of the layout contracts -- the VolumeView comments of csrc/vv_device.h, "optional second layouts" in include/volviz.h,
DESIGN.md sections 2 and 4i -- and from nothing else of the product: no kernel, no builder and no instrument appears here.  The base texel of
a sample is the witness's (`witness._axis`, the fetch's own index); the executed samples of a frame come from the march loop of
tests/proj_model.py (reducer frames), from the witness's own march through its `visit` callback (composite frames, which end rays early) and
from tests/iso_model.py's ordinals (isosurface frames).

Layouts (the names used throughout): "linear" (also what the 64-bit build samples, and with other strides the padded pitch), "bricked",
"zpair", "xpair", "zfast".  A geometry is a dict: row and slice (the two strides of the layout in bytes -- bytes per row of bricks and per
layer of bricks for the bricked copy) and alloc (bytes of the allocation, the zeroed bytes behind the layout included).

What is modelled and what is not.  `lines()` is the compulsory set: the 128-byte lines under the loads of the executed samples that lie in
the volume (touched_lines_all = 0).  The issued set (touched_lines_all = 1, and the (block, line) pairs of touched_block_lines) also holds
the loads of idle lanes and of samples outside the volume; it depends on the samples per loop trip and the wave tiles of the launch and is
not modelled: the tests hold it to containment only.  The experiment geometries of the bricked copy (VV_BRICK_X7, VV_BRICK_HALO=0,
VV_BRICK_XLOG2, VV_BRICK_ZLOG2, VV_BRICK_EXTRA) are not modelled either: this file states the 4 x 4 x 4 bricks with an x halo that are built."""
from __future__ import annotations

import numpy as np

from witness import FILTER_TEX8, _axis, _in_bounds

LAYOUTS = ("linear", "bricked", "zpair", "xpair", "zfast")
LINE = 128                                      # bytes of a cache line
BRICK_ROW = {4: 20, 1: 8}                       # bytes of a brick row: f32 4 voxels + 1 halo voxel; u8 the same 5 bytes padded to 8
BRICK_BYTES = {4: 320, 1: 128}                  # 16 rows


def _vsz(vtype):
    return np.dtype(vtype).itemsize


# ---------------------------------------------------------------------------------------------------------------------
# a. layouts
# ---------------------------------------------------------------------------------------------------------------------
def pitched_linear(vtype, dims, pad, force, rows_knob=None):
    """(row, slice) of the linear layout as finalize_layout documents them for VV_PITCH_PAD=pad, VV_PITCH_FORCE (set or not) and
    VV_PITCH_ROWS=rows_knob: rows of a multiple of 1 KiB (any multiple of 16 bytes when forced) get `pad` bytes more; a slice that would then
    be a multiple of 4 KiB gets one more row, or rows_knob more rows whatever its size."""
    nx, ny, nz = dims
    dense = nx * _vsz(vtype)
    if pad == 0 or (dense % 1024 != 0 and not force) or dense % 16 != 0:
        return dense, dense * ny
    row = dense + pad
    rows = ny + (1 if (ny * row) % 4096 == 0 else 0)
    if rows_knob is not None and 0 <= rows_knob <= 64:
        rows = ny + rows_knob
    return row, rows * row


def dense_geom(layout, vtype, dims, row=None, slice=None):
    """The geometry of `layout` for a volume of dims (nx, ny, nz) as the contracts give it.  row / slice: the strides of a linear layout with
    padded pitch (pitched_linear); every other stride follows from the dimensions."""
    nx, ny, nz = dims
    v = _vsz(vtype)
    if layout == "linear":
        row = nx * v if row is None else row
        slice = row * ny if slice is None else slice
        # behind the voxels: one slice, two rows and 4096 bytes of zeros (weight-0 corners of edge samples land there)
        return dict(row=row, slice=slice, alloc=slice * nz + slice + 2 * row + 4096)
    assert row is None and slice is None
    if layout == "zfast":
        # rows of nz voxels, ny rows per slice, nx slices: padded like the linear layout's rows (1 KiB multiples: + 32 bytes, then one more row if the slice
        # is still a multiple of 4 KiB); u8 rows are multiples of 4 bytes; one slice, one row and 16 bytes of zeros behind the nx slices
        row = nz * v
        if row % 1024 == 0:
            row += 32
        elif v == 1:
            row = (row + 3) & ~3
        rows = ny + (1 if row % 1024 == 32 and (ny * row) % 4096 == 0 else 0)
        return dict(row=row, slice=rows * row, alloc=rows * row * (nx + 1) + row + 16)
    if layout in ("zpair", "xpair"):
        # records of two voxels, rows of n_fast + 1 records (u8 rows rounded up to 4 bytes), slabs of ny + 1 rows, one slab per index of the slow axis; 32 zero bytes behind
        n_fast, n_slow = (nx, nz) if layout == "zpair" else (nz, nx)
        row = ((n_fast + 1) * 2 * v + 3) & ~3
        return dict(row=row, slice=(ny + 1) * row, alloc=(ny + 1) * row * n_slow + 32)
    assert layout == "bricked"
    # bricks x fastest; one extra layer in y and z when the last voxel's neighbour would not exist otherwise, i.e. when the dimension is a multiple of 4;
    # f32: a row of bricks that is a multiple of 4 KiB gets 64 bytes more; 16 zero bytes behind
    nbx, nby, nbz = (nx + 3) // 4, ny // 4 + 1, nz // 4 + 1
    row = nbx * BRICK_BYTES[v]
    if v == 4 and row % 4096 == 0:
        row += 64
    return dict(row=row, slice=nby * row, alloc=nbz * nby * row + 16)


def _rows_into(buf, geom, block):
    """block [slices, rows, bytes] uint8 -> buf at slice / row strides."""
    s, r, b = block.shape
    assert geom["slice"] % geom["row"] == 0 and r * geom["row"] <= geom["slice"] and b <= geom["row"] and s * geom["slice"] <= len(buf)
    buf[:s * geom["slice"]].reshape(s, -1, geom["row"])[:, :r, :b] = block


def _pair_copy(vol, geom):
    """records (f, y, s) = {v(f, y, s), v(f, y, s + 1)} of a volume indexed [s, y, f]; indices beyond the volume clamp"""
    ns, ny, nf = vol.shape
    f = np.minimum(np.arange(nf + 1), nf - 1); y = np.minimum(np.arange(ny + 1), ny - 1); s1 = np.minimum(np.arange(ns) + 1, ns - 1)
    a = vol[:, y][:, :, f]
    b = vol[s1][:, y][:, :, f]
    rec = np.ascontiguousarray(np.stack([a, b], axis=-1))
    buf = np.zeros(geom["alloc"], np.uint8)
    _rows_into(buf, geom, rec.view(np.uint8).reshape(ns, ny + 1, -1))
    return buf


def pack(vol, layout, geom):
    """The whole allocation of `layout` for vol [nz, ny, nx] (uint8 or float32) as uint8 [geom["alloc"]].  The padding record that ends the rows of a
    u8 pair copy with an even dimension is written as zeros here; its content is unspecified (pair_padding)."""
    nz, ny, nx = vol.shape
    v = vol.dtype.itemsize
    if layout == "linear":
        buf = np.zeros(geom["alloc"], np.uint8)
        _rows_into(buf, geom, np.ascontiguousarray(vol).view(np.uint8).reshape(nz, ny, nx * v))
        return buf
    if layout == "zfast":                                      # voxel (x, y, z) at x * slice + y * row + z * voxel bytes
        buf = np.zeros(geom["alloc"], np.uint8)
        _rows_into(buf, geom, np.ascontiguousarray(vol.transpose(2, 1, 0)).view(np.uint8).reshape(nx, ny, nz * v))
        return buf
    if layout == "zpair":
        return _pair_copy(vol, geom)
    if layout == "xpair":                                      # the z-pair copy with x and z in each other's roles
        return _pair_copy(np.ascontiguousarray(vol.transpose(2, 1, 0)), geom)
    assert layout == "bricked"
    nbx, nby, nbz = (nx + 3) // 4, ny // 4 + 1, nz // 4 + 1
    e = BRICK_ROW[v] // v                                       # stored elements per brick row: 5 (f32), 8 (u8: the last three are zero padding)
    x = np.minimum(np.arange(nbx)[:, None] * 4 + np.arange(e)[None, :], nx - 1)      # [brick, element]: 4 voxels, then the halo = the next voxel in x, clamped
    y = np.minimum(np.arange(nby * 4), ny - 1).reshape(nby, 4)
    z = np.minimum(np.arange(nbz * 4), nz - 1).reshape(nbz, 4)
    # [bz, by, bx, z in brick, y in brick, element]: rows of a brick are y fastest, then z
    b = vol[z[:, None, None, :, None, None], y[None, :, None, None, :, None], x[None, None, :, None, None, :]]
    b = np.where(np.arange(e) <= 4, b, np.zeros((), vol.dtype))
    b = np.ascontiguousarray(b).view(np.uint8).reshape(nbz, nby, nbx * BRICK_BYTES[v])
    buf = np.zeros(geom["alloc"], np.uint8)
    _rows_into(buf, geom, b)
    return buf


def pair_padding(layout, vtype, dims, geom):
    """The byte ranges [(begin, end)] of a pair copy that the contract leaves unspecified: u8 rows are rounded up to 4 bytes, which appends one record
    of padding to the n_fast + 1 records of a row when n_fast is even.  No gather reads it: the last one starts at record n_fast - 1 and is 4 bytes long.
    By formula: row r of the copy, bytes [(n_fast + 1) * 2, row stride)."""
    nx, ny, nz = dims
    if layout not in ("zpair", "xpair") or _vsz(vtype) != 1:
        return []
    n_fast, n_slow = (nx, nz) if layout == "zpair" else (nz, nx)
    used = (n_fast + 1) * 2
    if used == geom["row"]:
        return []
    return [(r * geom["row"] + used, (r + 1) * geom["row"]) for r in range((ny + 1) * n_slow)]


def gathers(layout, vtype, geom, ix, iy, iz):
    """The loads one sample with base texel (ix, iy, iz) issues on `layout`: [(byte offsets from the layout's base, length)], offsets as int64 arrays of the
    indices' shape.  Order: the rows (y, z), (y + 1, z), (y, z + 1), (y + 1, z + 1) where there are four -- on the z-fastest copy, with z in the role of x,
    the rows (x, y), (x, y + 1), (x + 1, y), (x + 1, y + 1) --, the rows y, y + 1 of a pair copy.  The upper rows are not clamped: every layout holds them."""
    v = _vsz(vtype)
    ix = np.asarray(ix, np.int64); iy = np.asarray(iy, np.int64); iz = np.asarray(iz, np.int64)
    row, sl = geom["row"], geom["slice"]
    if layout in ("linear", "zfast"):
        fast, slow = (ix, iz) if layout == "linear" else (iz, ix)
        # f32: the pair (fast, fast + 1) in one 8-byte load; u8: the aligned pair of dwords that holds it, from fast & ~3
        o = slow * sl + iy * row + (fast * 4 if v == 4 else (fast & ~3))
        return [(o, 8), (o + row, 8), (o + sl, 8), (o + sl + row, 8)]
    if layout in ("zpair", "xpair"):
        fast, slow = (ix, iz) if layout == "zpair" else (iz, ix)
        o = slow * sl + iy * row + fast * 2 * v                # two neighbouring records: 16 bytes (f32), 4 bytes (u8)
        return [(o, 4 * v), (o + row, 4 * v)]
    assert layout == "bricked"

    def row_of(y, z):                                          # where the brick row that holds voxels (4 (x >> 2) .., y, z) begins
        return (z >> 2) * sl + (y >> 2) * row + (ix >> 2) * BRICK_BYTES[v] + ((z & 3) * 4 + (y & 3)) * BRICK_ROW[v]
    x_in = (ix & 3) * 4 if v == 4 else 0                       # f32: the pair from voxel x on (the halo makes it whole); u8: the whole 8-byte row
    return [(row_of(iy + dy, iz + dz) + x_in, 8) for dz in (0, 1) for dy in (0, 1)]


def corners(buf, layout, vtype, geom, ix, iy, iz):
    """The eight corner values [..., z, y, x] that the loads of gathers() deliver, taken out of `buf` (a pack() or a read-out) the way the contracts
    place them in each load."""
    v = _vsz(vtype)
    ix = np.asarray(ix, np.int64)
    loads = []
    for off, length in gathers(layout, vtype, geom, ix, iy, iz):
        raw = buf[off[..., None] + np.arange(length)]
        loads.append(np.ascontiguousarray(raw).view(vtype))    # [..., elements of the load]
    out = np.empty(ix.shape + (2, 2, 2), vtype)
    if layout in ("linear", "bricked", "zfast"):
        fast = ix if layout != "zfast" else np.asarray(iz, np.int64)
        first = np.zeros_like(fast) if v == 4 else (fast & 3)  # u8: voxel `fast` is byte fast & 3 of the 8 loaded
        for k, ld in enumerate(loads):
            lo = np.take_along_axis(ld, first[..., None], axis=-1)[..., 0]
            hi = np.take_along_axis(ld, first[..., None] + 1, axis=-1)[..., 0]
            if layout == "zfast":                               # load k = row (x + (k >> 1), y + (k & 1)), elements z, z + 1
                out[..., 0, k & 1, k >> 1] = lo; out[..., 1, k & 1, k >> 1] = hi
            else:                                               # load k = row (y + (k & 1), z + (k >> 1)), elements x, x + 1
                out[..., k >> 1, k & 1, 0] = lo; out[..., k >> 1, k & 1, 1] = hi
    else:
        for k, ld in enumerate(loads):                          # load k = row y + k: record (fast), record (fast + 1), each {slow, slow + 1}
            for f in (0, 1):
                for s in (0, 1):
                    if layout == "zpair":
                        out[..., s, k, f] = ld[..., 2 * f + s]
                    else:
                        out[..., f, k, s] = ld[..., 2 * f + s]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# b. samples
# ---------------------------------------------------------------------------------------------------------------------
def base_texels(tex, dims):
    """(ix, iy, iz) of texture coordinates tex [n, 3]: the witness's lower texel, the index the fetch computes."""
    nx, ny, nz = dims
    return tuple(_axis(tex[:, a], n, FILTER_TEX8)[0] for a, n in enumerate((nx, ny, nz)))


def in_volume(tex):
    return _in_bounds(tex)


def reducer_samples(R, inv_scale, march, ordinal_limit=None):
    """The executed samples of a reducer frame (MIP, projection; isosurface with ordinal_limit): tex [n, 3] float32 of every executed sample, inside the
    volume or not, and ray [n], the index into R of the ray that took it.  `march`: proj_model.march.  ordinal_limit [rays]: a ray's samples beyond this
    ordinal (1-based, in march order) are not executed -- the hit of an isosurface frame; negative: no limit."""
    tex, ray = [], []
    done = np.zeros(len(R["x"]), np.int64)
    for act, t, runs in march(R, inv_scale):
        ordinal = done[act][:, None] + np.arange(1, runs.shape[1] + 1)[None, :]
        if ordinal_limit is not None:
            lim = ordinal_limit[act][:, None]
            runs = runs & ((lim < 0) | (ordinal <= lim))
        done[act] += runs.sum(axis=1)
        tex.append(t[runs]); ray.append(np.broadcast_to(act[:, None], runs.shape)[runs])
    if not tex:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int64)
    return np.concatenate(tex), np.concatenate(ray)


class Visit:
    """A `visit` callback for witness.render: collects the executed samples of a composite frame, and for a Phong frame every entry 1..30 of every chunk
    a ray begins."""
    def __init__(self):
        self.executed, self.entries = [], []

    def __call__(self, tex, ran, started):
        self.executed.append(tex[ran])
        self.entries.append(tex[started][:, 1:31].reshape(-1, 3))

    def samples(self):
        return np.concatenate(self.executed) if self.executed else np.zeros((0, 3), np.float32)

    def all_entries(self):
        return np.concatenate(self.entries) if self.entries else np.zeros((0, 3), np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# c. instruments
# ---------------------------------------------------------------------------------------------------------------------
def _words(bit_numbers, bits):
    """uint32 words of a bitmap of `bits` bits with the given bits set (bit b = word b >> 5, value 1 << (b & 31))."""
    flags = np.zeros(((bits + 31) // 32) * 32, np.uint8)
    b = np.asarray(bit_numbers, np.int64)
    flags[b[b < bits]] = 1
    return np.packbits(flags, bitorder="little").view(np.uint32)


def brick_bits(dims):
    nx, ny, nz = dims
    return ((nx + 7) // 8) * ((ny + 7) // 8) * ((nz + 7) // 8)


def bricks(tex, dims):
    """touched_bricks: one bit per 8^3 brick (x fastest) under the 2 x 2 x 2 footprint, upper corners clamped to n - 1, of every sample of tex [n, 3]
    that lies in the volume.  uint32 words."""
    nx, ny, nz = dims
    tex = tex[in_volume(tex)]
    ix, iy, iz = base_texels(tex, dims)
    bnx, bny = (nx + 7) // 8, (ny + 7) // 8
    hit = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x = np.minimum(ix + dx, nx - 1) >> 3; y = np.minimum(iy + dy, ny - 1) >> 3; z = np.minimum(iz + dz, nz - 1) >> 3
                hit.append((z * bny + y) * bnx + x)
    return _words(np.concatenate(hit) if hit else [], brick_bits(dims))


def _gather_lines(tex, layout, vtype, geom, dims):
    """The 128-byte lines (offsets from the layout's base / 128) under gathers() of every sample of tex that lies in the volume, with repeats."""
    tex = tex[in_volume(tex)]
    ix, iy, iz = base_texels(tex, dims)
    got = []
    for off, length in gathers(layout, vtype, geom, ix, iy, iz):
        got += [off >> 7, (off + length - 1) >> 7]              # (no load is longer than a line: it touches one or two)
    return np.concatenate(got) if got else np.zeros(0, np.int64)


def line_numbers(tex, layout, vtype, geom, dims):
    """The distinct lines under gathers() of every sample of tex that lies in the volume, ascending."""
    return np.unique(_gather_lines(tex, layout, vtype, geom, dims))


def lines(tex, layout, vtype, geom, dims, bits):
    """touched_lines with touched_lines_all = 0 and touched_line_bits = bits: the compulsory set, clipped at `bits`.  uint32 words."""
    return _words(_gather_lines(tex, layout, vtype, geom, dims), bits)


def phong_bounds(visit, layout, vtype, geom, dims, bits):
    """The two pairs (bricks, lines) that bracket a Phong frame's bitmaps: the kernel marks the cache entries 1..30 of its own rays that lie in the
    volume, chunk by chunk, executed or not -- at least the executed samples, at most every entry of every chunk a ray begins."""
    lo, hi = visit.samples(), visit.all_entries()
    return (bricks(lo, dims), lines(lo, layout, vtype, geom, dims, bits)), (bricks(hi, dims), lines(hi, layout, vtype, geom, dims, bits))


def bit_count(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def contains(outer, inner):
    return not np.any(np.asarray(inner) & ~np.asarray(outer))
