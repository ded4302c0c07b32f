"""The segmentation contract of include/volviz.h (vv_label_volume rules 1-6, vv_mask_volume rules M1-M2) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; a box is ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive, None = the whole
volume.  Nothing here comes from the library and nothing from scipy.  The foreground is hist_model.bins inside [bin_lo, bin_hi]; the components come
from minimum propagation with pointer jumping: every foreground voxel holds the index of a voxel of its component (at first its own), takes the least
value among itself and its neighbours, and then follows the values as pointers until they stop changing; repeated until a round changes nothing, every
voxel then holds the least index of its component.  The output stages of the mask are restated from the header (they are also derive_model.finish and
resample_model.finish; test_label.py ties them together).  Results are compared exactly."""
from types import SimpleNamespace

import numpy as np

import hist_model as HM

f32 = np.float32
U8, F32 = 0, 1
KEEP_LABEL, KEEP_FOREGROUND, KEEP_MIN_SIZE = 0, 1, 2
CONNECTIVITIES = (6, 18, 26)


def offsets(connectivity):
    """Rule 2: the (dz, dy, dx) of a voxel's neighbours: differing on exactly one axis (6), at most two (18), up to three (26)."""
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 < (dz != 0) + (dy != 0) + (dx != 0) <= reach]


def foreground(vol, bins, box=None):
    """Rule 1: the box's foreground, bool [bz, by, bx]."""
    lo, hi = (bins, bins) if np.isscalar(bins) else bins
    b = HM.bins(HM.crop(np.asarray(vol), box))
    return (b >= lo) & (b <= hi)


def least_index(fg, connectivity):
    """Rules 2-3: for every foreground voxel the least index i of its component (int64, same shape; background holds fg.size)."""
    fg = np.asarray(fg, bool)
    n = fg.size
    cur = np.where(fg, np.arange(n, dtype=np.int64).reshape(fg.shape), n)
    offs = offsets(connectivity)
    nz, ny, nx = fg.shape
    while True:
        pad = np.pad(cur, 1, constant_values=n)                 # voxels outside the box do not exist
        m = cur.copy()
        for dz, dy, dx in offs:
            np.minimum(m, pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx], out=m)
        m[~fg] = n
        flat = np.append(m.ravel(), n)                          # flat[n] = n: background points at itself
        while True:                                             # pointer jumping: a value is the index of a voxel of the same component
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        m = flat[:n].reshape(fg.shape)
        if np.array_equal(m, cur):
            return cur
        cur = m


def components(fg, connectivity=6):
    """Rules 4-6 for a foreground array: labels uint32, sizes uint32, stats."""
    fg = np.asarray(fg, bool)
    assert fg.ndim == 3 and fg.size <= 2 ** 32 - 2
    least = least_index(fg, connectivity)
    labels = np.where(fg, least + 1, 0).astype(np.uint32)
    sizes = np.bincount(least[fg], minlength=fg.size)[:fg.size].astype(np.uint32).reshape(fg.shape)
    flat = sizes.ravel()
    largest = int(flat.max()) if flat.size else 0
    stats = SimpleNamespace(foreground=int(fg.sum()), components=int((flat > 0).sum()), largest_size=largest,
                            largest_label=int(np.argmax(flat)) + 1 if largest else 0, reserved=0)       # argmax: the first = the smallest label
    return labels, sizes, stats


def label(vol, bins, connectivity=6, box=None):
    """vv_label_volume: (labels, sizes, stats) of the box."""
    return components(foreground(vol, bins, box), connectivity)


def stats_without_sizes(stats):
    """Rule 6 when `sizes` is NULL."""
    return SimpleNamespace(foreground=stats.foreground, components=stats.components, largest_size=0, largest_label=0, reserved=0)


def copy_stage(sub, out_type):
    """Rule M2, a kept voxel: vv_derive_volume's rule 3 without a window."""
    with np.errstate(all="ignore"):
        if sub.dtype == np.uint8:
            return sub.copy() if out_type == U8 else sub.astype(f32) / f32(255)      # correctly rounded: IEEE division
        return sub.copy() if out_type == F32 else HM.bins(sub)


def fill_stage(fill, src_dtype, out_type):
    """Rule M2, any other voxel: vv_resample_volume's rule 4 on `fill`; a 0-d array of the output's dtype."""
    r = f32(fill)
    if src_dtype == np.float32:
        return np.asarray(r) if out_type == F32 else HM.bins(np.asarray(r, f32).reshape(1))[0]
    if out_type == F32:
        return np.asarray(r / f32(255))
    if not r >= f32(0.5):
        return np.uint8(0)
    return np.uint8(255) if r >= f32(254.5) else np.uint8(int(np.trunc(f32(r + f32(0.5)))))


def kept(labels, keep, label=0, min_size=0, sizes=None, invert=False):
    """Rule M1: bool, the shape of labels."""
    labels = np.asarray(labels, np.uint32)
    if keep == KEEP_LABEL:
        test = labels == np.uint32(label)
    elif keep == KEEP_FOREGROUND:
        test = labels != 0
    else:
        assert keep == KEEP_MIN_SIZE and sizes is not None
        flat = np.asarray(sizes, np.uint32).ravel()
        lab = labels.astype(np.int64)
        ok = (lab != 0) & (lab - 1 < labels.size)
        test = np.zeros(labels.shape, bool)
        test[ok] = flat[lab[ok] - 1] >= np.uint32(min_size)
    return test != bool(invert)


def mask(vol, labels, keep, label=0, min_size=0, sizes=None, invert=False, fill=0.0, box=None, out_type=None):
    """vv_mask_volume: the output volume [bz, by, bx], uint8 or float32."""
    sub = HM.crop(np.asarray(vol), box)
    assert sub.dtype in (np.uint8, np.float32) and sub.shape == np.shape(labels)
    if out_type is None:
        out_type = U8 if sub.dtype == np.uint8 else F32
    k = kept(labels, keep, label, min_size, sizes, invert)
    copied = np.ascontiguousarray(copy_stage(sub, out_type))
    out = np.empty(sub.shape, copied.dtype)
    out[...] = fill_stage(fill, sub.dtype, out_type)
    raw = np.uint32 if out.dtype == np.float32 else np.uint8            # a kept f32 voxel keeps its pattern, NaNs included
    out.view(raw)[k] = copied.view(raw)[k]
    return out


def same(got, want):
    """Exact: integers, or uint32 patterns of float32.  Returns the indices that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        return np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    return np.argwhere(got != want)
