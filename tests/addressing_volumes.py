"""What tests/test_addressing.py needs for the volume-to-volume families (derive, stencil, resample, label and mask) and is not a test: the linear
layout's arithmetic, the calls each family makes on a box, the voxel that decides each output voxel, the models' outputs, and the wide label box:
its foreground as a coordinate list and a sparse model of the labelling contract over that list.  Nothing here touches the GPU or the library."""
import numpy as np

import derive_model as DM
import hist_model as HM
import label_model as LM
import resample_model as RM
import stencil_model as StM
import witness as Wt

f32 = np.float32
FAMILIES = ("derive", "stencil", "resample", "label and mask")
STRADDLING = ("inside a row", "across slices")
EULER = (0.02, -0.015, 0.01)                                    # the small rotation of the resampled boxes
MIN_SIZE = 3


def pitches(dims, itemsize):
    """(row pitch, slice pitch) of the linear layout in bytes: rows of a multiple of 1 KiB are re-pitched by 32 bytes, with one more row if the slice
    would still be a multiple of 4 KiB (the rule Loaded.__init__ of test_addressing.py holds the library to)."""
    nx, ny, _ = dims
    row = nx * itemsize + (32 if nx * itemsize % 1024 == 0 else 0)
    rows = ny + (1 if row != nx * itemsize and ny * row % 4096 == 0 else 0)
    return row, rows * row


class Layout:
    """The linear layout of one volume: byte offsets of voxels."""

    def __init__(self, dims, itemsize, row_bytes, slice_bytes, limit):
        self.dims, self.size, self.row_bytes, self.slice_bytes, self.limit = tuple(dims), itemsize, row_bytes, slice_bytes, limit

    def at(self, x, y, z):
        return np.asarray(z, np.int64) * self.slice_bytes + np.asarray(y, np.int64) * self.row_bytes + np.asarray(x, np.int64) * self.size

    def grid(self, xs, ys, zs):
        """Offsets [len(zs), len(ys), len(xs)] of the voxels of three coordinate lists."""
        return self.at(np.asarray(xs)[None, None, :], np.asarray(ys)[None, :, None], np.asarray(zs)[:, None, None])

    def ends(self, box):
        """The offsets of a box's first and last voxel."""
        (x0, y0, z0), (x1, y1, z1) = box
        return int(self.at(x0, y0, z0)), int(self.at(x1 - 1, y1 - 1, z1 - 1))


def family_box(family, box, dims):
    """The box a family runs on: derive's starts at a multiple of 16 voxels in x, so that factor (1, 1, 1) takes the vector loads wherever the pitches
    allow them; the label calls' is 24 voxels wider on either side in x, so that the two straddling boxes of a three-slice volume hold 20 components.
    A box only grows inside its rows and slices: its first voxel moves to a lower address, its last one to a higher one, and the property it is
    named for is asserted again by the caller."""
    (x0, y0, z0), (x1, y1, z1) = box
    if family == "derive":
        x0 = x0 // 16 * 16
    if family == "label and mask":
        x0, x1 = max(x0 - 24, 0), min(x1 + 24, dims[0])
    return (x0, y0, z0), (x1, y1, z1)


def box_property(name, box, L, dims):
    """The property a box of _hist_boxes is named for, by the same first / last offsets."""
    first, last = L.ends(box)
    if name == "below":
        return first == 0 and last < L.limit
    if name in STRADDLING:
        return first < L.limit <= last
    return first >= L.limit and tuple(box[1]) == tuple(dims)


def centre_of(box, dims):
    return tuple((l + h) / 2.0 / n for l, h, n in zip(box[0], box[1], dims))


def rotation_centre(box, dims):
    """The `centre` to hand resample_matrix so that the rotation by EULER leaves the box's centre c where it is.  The matrix is p = A (q - 1/2) +
    centre: `centre` is where the grid's centre lands, so the fixed point c needs centre = c + A (1/2 - c)."""
    A = RM.matrix(EULER, 1.0).reshape(3, 4)[:, :3].astype(np.float64)
    c = np.array(centre_of(box, dims))
    return tuple(float(v) for v in c + A @ (0.5 - c))


def rotation(box, dims):
    """resample_matrix(euler=EULER, zoom=1, centre=rotation_centre) as the model states it: a small rotation about the box's centre."""
    return RM.matrix(EULER, 1.0, rotation_centre(box, dims))


def cases(family, bname, src_type, other_type=False):
    """The calls of one family on one box, as keyword dicts (resample: `rotated` stands for the matrix).  other_type: the stencil calls once more
    with the other output type."""
    if family == "derive":
        factors = ((1, 1, 1), (2, 3, 1)) if bname != "last voxel" else ((1, 1, 1), (2, 3, 1), (4, 4, 4))
        return [dict(factor=f, mode=m, out_type=t) for f in factors for m in (DM.MEAN, DM.MAX) for t in (DM.U8, DM.F32)]
    if family == "stencil":
        taps = [StM.taps(StM.BINOMIAL, r) for r in (2, 1, 1)]
        kinds = [dict(kind=StM.SEPARABLE, radius=(2, 1, 1), taps=taps), dict(kind=StM.MEDIAN), dict(kind=StM.GRADMAG)]
        return [dict(k, out_type=t) for t in ((src_type, 1 - src_type) if other_type else (src_type,)) for k in kinds]
    if family == "resample":
        return [dict(rotated=r, filter=f) for r in (False, True) for f in (RM.TEX8, RM.EXACT, RM.NEAREST)]
    assert family == "label and mask"
    return [dict(connectivity=c) for c in (6, 26)]


def deciding(family, case, box, L):
    """The byte offset of the voxel that decides each output voxel of one call, in the output's shape, and which outputs a voxel decides at all
    (a resampled voxel outside the volume holds the fill value).  derive: the cell's first voxel; stencil: the centre voxel; label and mask: the
    source voxel; resample: the lower corner of the position resample_model.positions gives."""
    (x0, y0, z0), (x1, y1, z1) = box
    nx, ny, nz = L.dims
    if family == "resample":
        p = RM.positions(L.dims, rotation(box, L.dims) if case["rotated"] else None, box)
        ok = RM.inside(p)
        with np.errstate(invalid="ignore"):
            lower = [Wt._axis(np.where(ok, p[..., a], f32(0)), n, Wt.FILTER_EXACT)[0] for a, n in enumerate((nx, ny, nz))]
        return L.at(*lower), ok
    fx, fy, fz = case["factor"] if family == "derive" else (1, 1, 1)
    off = L.grid(np.arange(x0, x1, fx), np.arange(y0, y1, fy), np.arange(z0, z1, fz))
    return off, np.ones(off.shape, bool)


def _stencil_crop(host, box, halo=2):
    """The box with `halo` voxels around it, cut at the volume's faces, and the box inside that crop.  A stencil clamps its coordinates to the volume;
    the crop ends before the box's halo only where the volume does, so the model of the crop clamps where the model of the volume would."""
    nz, ny, nx = host.shape
    lo = tuple(max(l - halo, 0) for l in box[0])
    hi = tuple(min(h + halo, n) for h, n in zip(box[1], (nx, ny, nz)))
    sub = host[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    return sub, (tuple(a - b for a, b in zip(box[0], lo)), tuple(a - b for a, b in zip(box[1], lo)))


def want(family, case, host, box):
    """The model's output of one call (label and mask: (labels, sizes, stats))."""
    dims = host.shape[::-1]
    if family == "derive":
        return DM.derive(host, box, case["factor"], case["mode"], case["out_type"])
    if family == "stencil":
        sub, inner = _stencil_crop(host, box)
        return StM.stencil(sub, case["kind"], inner, case["out_type"], case.get("radius", (0, 0, 0)), case.get("taps"))
    if family == "resample":
        return RM.resample(host, dims, rotation(box, dims) if case["rotated"] else None, case["filter"], 0.0, None, box)
    return LM.label(host, label_bins(host, box), case["connectivity"], box)


def label_bins(host, box):
    """The bin range of a box's label calls, chosen from the noise: bins 0 ... the 33rd percentile of the box's own bins: a foreground share of 0.33
    and what the ties of that bin add, just above the percolation threshold of the 6-neighbourhood (0.31), where the components are many."""
    return 0, int(np.percentile(HM.bins(HM.crop(host, box)), 33))


def mask_cases():
    return [dict(keep=k, min_size=MIN_SIZE if k == LM.KEEP_MIN_SIZE else 0, out_type=t, fill=7.0 if t == LM.U8 else 0.37)
            for k in (LM.KEEP_FOREGROUND, LM.KEEP_MIN_SIZE) for t in (LM.U8, LM.F32)]


def want_mask(host, labels, sizes, box, mc):
    return LM.mask(host, labels, mc["keep"], min_size=mc["min_size"], sizes=sizes, fill=mc["fill"], box=box, out_type=mc["out_type"])


def same(family, got, want_):
    return {"derive": DM.same, "stencil": StM.same, "resample": RM.same, "label and mask": LM.same}[family](got, want_)


def records(family, w, host, box):
    """What is compared of one call whose model output is `w`, one record per output voxel, for the distinct-values condition: the output's patterns
    (label and mask: the labels, the sizes and the KEEP_MIN_SIZE mask side by side)."""
    if family != "label and mask":
        return np.ascontiguousarray(w).view(np.uint32 if w.dtype == np.float32 else np.uint8).reshape(-1, 1).astype(np.uint32)
    labels, sizes, _ = w
    m = want_mask(host, labels, sizes, box, mask_cases()[2])
    return np.column_stack([labels.ravel(), sizes.ravel(), m.ravel().astype(np.uint32)])


def shares(family, boxes, L):
    """Per distinct set of deciding voxels of a family (derive: per factor; resample: per matrix): (what, offsets of the deciding voxels of the two
    straddling boxes together): from the layout alone."""
    out = []
    seen = set()
    for case in cases(family, "inside a row", 0):
        key = {"derive": case.get("factor"), "resample": case.get("rotated")}.get(family)
        if key in seen:
            continue
        seen.add(key)
        offs = []
        for bname in STRADDLING:
            off, ok = deciding(family, case, family_box(family, boxes[bname], L.dims), L)
            offs.append(off[ok])
        out.append((f"{family} {key}", np.concatenate(offs)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the wide label box: a sparse foreground and its sparse model
# ---------------------------------------------------------------------------------------------------------------------
WIDE_DIMS = (2047, 2049, 1023)                                  # 4 290 771 969 voxels: above 2^31, below 2^32 - 2; no extent a multiple of the 16 x 8 x 8 tile
WIDE = dict(dims=WIDE_DIMS, half=1 << 31, island=(24, 12, 12), loop=(20, 10), stairs=64)
SMALL = dict(dims=(63, 41, 39), half=63 * 41 * 39 // 2, island=(10, 6, 6), loop=(8, 5), stairs=16)


def wide_foreground(dims, half, island, loop, stairs, seed=5):
    """The foreground of the wide label box as sorted flat indices, and its structures by name (flat indices each): three islands with about half
    their voxels set (at the origin, centred on the voxel of index `half`, ending at the last voxel); a one-voxel wire from the first island along z to
    the last slice and there along y and x into the last island; a closed wire and a staircase of `stairs` voxels that touch at edges and corners
    only, both wholly above `half`.  Structures that are not meant to touch keep at least 2 voxels between their bounding boxes."""
    nx, ny, nz = dims
    ix, iy, iz = island
    rng = np.random.default_rng(seed)
    flat = lambda x, y, z: (np.asarray(z, np.int64) * ny + np.asarray(y, np.int64)) * nx + np.asarray(x, np.int64)
    hz, rem = divmod(int(half), nx * ny)
    hy, hx = divmod(rem, nx)
    parts, bounds = {}, {}

    def put(name, x, y, z):
        x, y, z = np.broadcast_arrays(np.asarray(x), np.asarray(y), np.asarray(z))
        assert x.min() >= 0 and x.max() < nx and y.min() >= 0 and y.max() < ny and z.min() >= 0 and z.max() < nz, name
        parts[name] = np.unique(np.concatenate([parts.get(name, np.zeros(0, np.int64)), flat(x, y, z).ravel()]))
        b = ((int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max())))
        if name in bounds:
            b = (tuple(min(p, q) for p, q in zip(b[0], bounds[name][0])), tuple(max(p, q) for p, q in zip(b[1], bounds[name][1])))
        bounds[name] = b

    for name, lo in (("island first", (0, 0, 0)), ("island half", tuple(int(np.clip(h - s // 2, 0, n - s)) for h, s, n in zip((hx, hy, hz), island, dims))),
                     ("island last", (nx - ix, ny - iy, nz - iz))):
        z, y, x = np.nonzero(rng.random((iz, iy, ix)) < 0.5)
        put(name, x + lo[0], y + lo[1], z + lo[2])
    put("island half", hx, hy, hz)                              # the voxel of index `half` itself
    put("wire", 2, 2, np.arange(nz))
    put("wire", 2, np.arange(2, ny), nz - 1)
    put("wire", np.arange(2, nx), ny - 1, nz - 1)
    lx, ly = loop
    zl, x0, y0 = hz + (nz - hz) // 2, nx // 4, ny // 4
    put("loop", np.arange(x0, x0 + lx + 1), y0, zl); put("loop", np.arange(x0, x0 + lx + 1), y0 + ly, zl)
    put("loop", x0, np.arange(y0, y0 + ly + 1), zl); put("loop", x0 + lx, np.arange(y0, y0 + ly + 1), zl)
    k = np.arange(stairs)
    put("stairs", nx // 2 + 6 + k, ny // 2 + k, hz + (nz - hz) // 4 + (k % 4 >= 2))      # steps across an edge and across a corner in turn
    names = list(parts)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if "wire" in (a, b) and ("island first" in (a, b) or "island last" in (a, b)):
                continue                                        # meant to touch
            gap = max(max(bounds[a][0][c] - bounds[b][1][c], bounds[b][0][c] - bounds[a][1][c]) for c in range(3))
            if "wire" in (a, b):                                # the wire's bounding box is the volume's: measure its three legs
                w, o = (a, b) if a == "wire" else (b, a)
                (ox0, oy0, oz0), (ox1, oy1, oz1) = bounds[o]
                cheb = lambda lo, hi, v: max(lo - v, v - hi, 0)
                gap = min(max(cheb(ox0, ox1, 2), cheb(oy0, oy1, 2)), max(cheb(ox0, ox1, 2), cheb(oz0, oz1, nz - 1)), max(cheb(oy0, oy1, ny - 1), cheb(oz0, oz1, nz - 1)))
            assert gap >= 3, (a, b, gap)
    for name in ("loop", "stairs"):
        assert parts[name].min() > half, name
    return np.unique(np.concatenate(list(parts.values()))), parts


def sparse_label(idx, dims, connectivity):
    """vv_label_volume's rules 2-6 over a sorted list of foreground flat indices of a box of `dims`: (labels, sizes) per listed voxel and the stats
    tuple (foreground, components, largest_size, largest_label, 0).  Minimum propagation with pointer jumping over the neighbour graph of the list."""
    nx, ny, nz = dims
    idx = np.asarray(idx, np.int64)
    assert (np.diff(idx) > 0).all()
    z, rem = np.divmod(idx, nx * ny)
    y, x = np.divmod(rem, nx)
    a, b = [], []
    for dz, dy, dx in LM.offsets(connectivity):
        ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
        nb = ((z + dz) * ny + (y + dy)) * nx + (x + dx)
        pos = np.searchsorted(idx, nb)
        ok &= (pos < len(idx)) & (idx[np.minimum(pos, len(idx) - 1)] == nb)
        a.append(np.flatnonzero(ok)); b.append(pos[ok])
    a, b = np.concatenate(a), np.concatenate(b)
    lab = np.arange(len(idx))
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        while True:
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    count = np.bincount(lab, minlength=len(idx))
    labels = (idx[lab] + 1).astype(np.uint32)
    sizes = np.where(lab == np.arange(len(idx)), count, 0).astype(np.uint32)       # a component's size sits at its least voxel
    largest = int(count.max()) if len(idx) else 0
    stats = (len(idx), int((count > 0).sum()), largest, int(idx[np.argmax(count)]) + 1 if largest else 0, 0)
    return labels, sizes, stats
