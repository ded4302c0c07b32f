"""The region contract of include/volviz.h (vv_region_table, rules 1-6) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; `labels` and `aux` are uint32 arrays with the box's shape [bz, by, bx]; a box is
((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive.  Nothing here comes from the library: ownership is two gathers on the labels, the rank a
cumulative sum over the roots, every sum an np.add.at on 64-bit integers, every extremum an np.minimum.at / np.maximum.at, the bins are hist_model's,
the faces come from comparing the owners with shifted copies of themselves."""
from types import SimpleNamespace

import numpy as np

import hist_model as HM

LABELS, NONZERO = 0, 1
DTYPE = np.dtype([("label", "<u4"), ("reserved", "<u4"), ("voxels", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum", "<u8", 3), ("sum2", "<u8", 6),
                  ("bin_min", "<u4"), ("bin_max", "<u4"), ("bin_sum", "<u8"), ("bin_sum2", "<u8"), ("vmin", "<f4"), ("vmax", "<f4"),
                  ("faces", "<u8", 3), ("aux_sum", "<u8"), ("aux_argmax", "<u4"), ("aux_max", "<u4")])
assert DTYPE.itemsize == 184
OUTSIDE = -2                                               # the owner of a voxel beyond the box's faces


def ownership(labels, source=LABELS):
    """Rules 1 and 2 on the flat labels: (roots: their indices ascending, owner: the owning root's index per voxel or -1, rank: the owner's rank or -1)."""
    flat = np.ascontiguousarray(labels, np.uint32).ravel().astype(np.int64)
    n = flat.size
    idx = np.arange(n, dtype=np.int64)
    if source == NONZERO:
        nz = flat != 0
        roots = np.flatnonzero(nz)[:1]
        owner = np.where(nz, roots[0] if len(roots) else -1, -1)
        return roots, owner, np.where(nz, 0, -1)
    assert source == LABELS
    is_root = flat == idx + 1
    points_in = (flat != 0) & (flat - 1 < n)
    r = np.where(points_in, flat - 1, 0)
    owned = points_in & is_root[r]
    owner = np.where(owned, r, -1)
    rank_of = np.cumsum(is_root) - 1                            # at a root: the number of roots below it
    return np.flatnonzero(is_root), owner, np.where(owned, rank_of[r], -1)


def _key_inverse(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def face_counts(owner3):
    """Per voxel [3, bz, by, bx]: the number (0..2) of its faces perpendicular to x, y, z whose neighbour lies outside the box or has another owner."""
    pad = np.pad(owner3, 1, constant_values=OUTSIDE)
    core = (slice(1, -1),) * 3
    out = np.zeros((3,) + owner3.shape, np.int64)
    for a, axis in enumerate((2, 1, 0)):                        # x is the last array axis
        for shift in (1, -1):
            out[a] += np.roll(pad, shift, axis)[core] != owner3
    return out


def region_table(vol, labels, aux=None, source=LABELS, box=None, max_regions=None):
    """(table: DTYPE[min(K, max_regions)], compact: uint32 like labels, summary: regions, written, foreground, stray)."""
    sub = HM.crop(np.asarray(vol), box)
    labels = np.ascontiguousarray(labels, np.uint32)
    assert labels.shape == sub.shape, (labels.shape, sub.shape)
    lo = (0, 0, 0) if box is None else tuple(int(v) for v in box[0])
    roots, owner, rank = ownership(labels, source)
    flat = labels.ravel()
    K = len(roots)
    written = K if max_regions is None else min(K, int(max_regions))
    compact = np.where(rank >= 0, rank + 1, 0).astype(np.uint32).reshape(labels.shape)
    foreground = int((flat != 0).sum())
    summary = SimpleNamespace(regions=K, written=written, foreground=foreground, stray=foreground - int((rank >= 0).sum()))
    t = np.zeros(written, DTYPE)
    if written == 0:
        return t, compact, summary
    sel = np.flatnonzero((rank >= 0) & (rank < written))
    row = rank[sel]
    t["label"] = (roots[:written] + 1).astype(np.uint32)
    np.add.at(t["voxels"], row, np.uint64(1))
    z, y, x = (c.ravel()[sel].astype(np.int64) for c in np.indices(labels.shape))
    coords = (x + lo[0], y + lo[1], z + lo[2])
    t["lo"] = np.iinfo(np.int32).max
    for a, c in enumerate(coords):
        np.minimum.at(t["lo"][:, a], row, c.astype(np.int32))
        np.maximum.at(t["hi"][:, a], row, (c + 1).astype(np.int32))
        np.add.at(t["sum"][:, a], row, c.astype(np.uint64))
    for k, (p, q) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        np.add.at(t["sum2"][:, k], row, (coords[p] * coords[q]).astype(np.uint64))
    bins = HM.bins(sub).ravel()[sel].astype(np.int64)
    t["bin_min"] = 0xFFFFFFFF
    np.minimum.at(t["bin_min"], row, bins.astype(np.uint32))
    np.maximum.at(t["bin_max"], row, bins.astype(np.uint32))
    np.add.at(t["bin_sum"], row, bins.astype(np.uint64))
    np.add.at(t["bin_sum2"], row, (bins * bins).astype(np.uint64))
    values = np.ascontiguousarray(sub, np.float32).ravel()[sel]           # u8: (float)byte
    real = ~np.isnan(values)
    keys = HM.keys(values)
    kmin, kmax = np.full(written, 0xFFFFFFFF, np.uint32), np.zeros(written, np.uint32)
    np.minimum.at(kmin, row[real], keys[real])
    np.maximum.at(kmax, row[real], keys[real])
    none = kmax == 0                                             # no key of a value is 0
    t["vmin"] = np.where(none, np.float32(np.inf), _key_inverse(kmin))
    t["vmax"] = np.where(none, np.float32(-np.inf), _key_inverse(kmax))
    faces = face_counts(owner.reshape(labels.shape))
    for a in range(3):
        np.add.at(t["faces"][:, a], row, faces[a].ravel()[sel].astype(np.uint64))
    if aux is not None:
        av = np.ascontiguousarray(aux, np.uint32).ravel()[sel]
        np.add.at(t["aux_sum"], row, av.astype(np.uint64))
        np.maximum.at(t["aux_max"], row, av)
        at_max = av == t["aux_max"][row]
        arg = np.full(written, 0xFFFFFFFF, np.uint32)
        np.minimum.at(arg, row[at_max], sel[at_max].astype(np.uint32))
        t["aux_argmax"] = arg
    return t, compact, summary


def same_rows(got, want):
    """The indices of the rows that differ in any byte."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), DTYPE.itemsize)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), DTYPE.itemsize)
    return np.flatnonzero((g != w).any(axis=1))
