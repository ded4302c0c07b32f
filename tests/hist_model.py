"""The histogram contract of include/volviz.h (vv_volume_histogram, pins 1-3 and 5) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; a box is ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive.
Nothing here comes from the oracle or from the library: bins are the pin's three cases on a binary32 product, the range is an argmin / argmax
over integer keys of the bit patterns."""
from types import SimpleNamespace

import numpy as np

f32 = np.float32


def bins(vol):
    """Pin 1: the classification index of every voxel, uint8, same shape."""
    vol = np.asarray(vol)
    if vol.dtype == np.uint8:
        return vol.copy()
    assert vol.dtype == np.float32
    with np.errstate(all="ignore"):
        s = vol * f32(255.0)                                    # binary32, one rounding
        assert s.dtype == np.float32
        mid = (s >= f32(1)) & (s < f32(255))
        out = np.zeros(vol.shape, np.uint8)                     # NaN, s < 1
        out[mid] = np.trunc(s[mid]).astype(np.int64).astype(np.uint8)
        out[s >= f32(255)] = 255                                # +Inf included
    return out


def keys(vol):
    """Total order of binary32 bit patterns as uint32: negative patterns complemented, the others with the top bit set."""
    u = np.ascontiguousarray(vol, f32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))


def value_range(vol):
    """Pin 2: (vmin, vmax) as np.float32, copies of voxels (compare them as uint32 patterns)."""
    vol = np.asarray(vol)
    if vol.dtype == np.uint8:
        return f32(vol.min()), f32(vol.max())
    flat = np.ascontiguousarray(vol, f32).ravel()
    flat = flat[~np.isnan(flat)]
    if flat.size == 0:
        return f32(np.inf), f32(-np.inf)
    k = keys(flat)
    return flat[np.argmin(k)], flat[np.argmax(k)]


def crop(vol, box):
    if box is None:
        return vol
    (x0, y0, z0), (x1, y1, z1) = box
    nz, ny, nx = vol.shape
    assert 0 <= x0 < x1 <= nx and 0 <= y0 < y1 <= ny and 0 <= z0 < z1 <= nz, box
    return vol[z0:z1, y0:y1, x0:x1]


def histogram(vol, box=None):
    """Pins 1-3: counts uint64[256], voxels, nan_voxels, vmin, vmax (np.float32) of the box."""
    sub = crop(np.asarray(vol), box)
    vmin, vmax = value_range(sub)
    return SimpleNamespace(counts=np.bincount(bins(sub).ravel(), minlength=256).astype(np.uint64), voxels=int(sub.size),
                           nan_voxels=int(np.isnan(sub).sum()) if sub.dtype == np.float32 else 0, vmin=vmin, vmax=vmax)


def histogram_indices(index):
    """Pin 5: the number of bytes equal to k, uint64[256]."""
    index = np.asarray(index, np.uint8).ravel()
    return np.array([(index == k).sum() for k in range(256)], np.uint64)
