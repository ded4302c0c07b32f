"""The host plumbing of the calls that are not frames (csrc/vv_api.cpp): where an output lives and who waits, which of several bad
arguments a call reports, and what the context says it holds on the device.

  * output home x stream form: a host buffer and a device buffer receive the same bytes, the device buffer in each of the three stream
    forms of the C-ABI (NULL = synchronous, VV_STREAM_DEFAULT_ASYNC and a caller's stream = enqueue only).  Every output starts as a
    non-zero byte pattern with a guard behind it: elements a kernel skips keep the pattern in both homes, and so does the guard.
    (The slab, histogram, MIP / iso / projection and vv_render cells of this matrix are in test_slab, test_hist, test_mip, test_iso,
    test_proj and test_gpu_parity.)
  * error precedence: calls with two bad arguments, each of which is rejected on the host before the device is touched, report the
    code and the vv_last_error text recorded below.  The literals were taken from the library as it was before the staging path, the
    slice / slab host path and the volume allocator were unified (one run of this table against that build), not from the code under test.
    The rows of the label, mask, distance, region-table and mesh calls were taken in the same way from the library as it was before those
    five calls were given one opening, one buffer-role list and one overlap rule (every row observed on that build, code and text).
  * scratch accounting: vv_device_bytes()[3] counts every scratch buffer of the context.
"""
import ctypes as C

import numpy as np
import pytest

import volviz_amd as vv

pytestmark = pytest.mark.gpu

FILL = 0xA5                                   # every output byte before a call
GUARD = 16                                    # bytes behind every output that no call may touch
INVALID, NO_VOLUME = -1, -2                   # vv_status (include/volviz.h)
NX, NY, NZ = 12, 10, 9


def _volume(dtype):
    rng = np.random.default_rng(7)
    if dtype == np.uint8:
        return rng.integers(0, 256, (NZ, NY, NX), dtype=np.uint8)
    return rng.random((NZ, NY, NX), dtype=np.float32)


@pytest.fixture(scope="module")
def torch_side():
    """torch and one side stream (a caller's stream of the enqueue-only form)."""
    import torch
    return torch, torch.cuda.Stream(device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def loaded():
    """One context per voxel type with the 12 x 10 x 9 volume and a transfer function, and one that has loaded nothing."""
    ctxs = {"u8": vv.Context(0), "f32": vv.Context(0), "fresh": vv.Context(0)}
    ctxs["u8"].load_volume(_volume(np.uint8), vv.transfer_preset(vv.TF_ENGINE))
    ctxs["f32"].load_volume(_volume(np.float32), vv.transfer_preset(vv.TF_HEAD))
    yield ctxs
    for c in ctxs.values():
        c.close()


def _both_homes(torch_side, sizes, call, inputs=None):
    """call(out_ptrs, on_device, stream) -> rc writes outputs of `sizes` bytes.  Runs it on host buffers, then on device buffers in the
    three stream forms, all prefilled with FILL and followed by a guard; the device bytes must equal the host bytes, guard included.
    `inputs`: {name: uint8 array} handed to `call` as pointers of the same home as the outputs (keyword `inp`).  Returns the host outputs."""
    torch, side = torch_side
    dev = torch.device("cuda", 0)
    inputs = inputs or {}
    host = [np.full(n + GUARD, FILL, np.uint8) for n in sizes]
    rc = call([h.ctypes.data for h in host], 0, None, inp={k: v.ctypes.data for k, v in inputs.items()})
    assert rc == 0
    for h, n in zip(host, sizes):
        assert np.all(h[n:] == FILL), "a host-buffer call wrote behind its output"
    dev_in = {k: torch.from_numpy(v.copy()).to(dev) for k, v in inputs.items()}
    for name, stream in (("synchronous", None), ("default stream, enqueue only", vv.STREAM_DEFAULT_ASYNC), ("caller's stream, enqueue only", vv.stream_handle(side))):
        out = [torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=dev) for n in sizes]
        torch.cuda.synchronize()                                  # the prefill (torch's stream) before the library writes on another stream
        rc = call([o.data_ptr() for o in out], 1, stream, inp={k: v.data_ptr() for k, v in dev_in.items()})
        assert rc == 0, name
        if stream is not None:
            torch.cuda.synchronize()                              # enqueue only: the work is done when the device is idle
        for h, o in zip(host, out):
            assert np.array_equal(o.cpu().numpy(), h), f"device buffer ({name}) differs from the host buffer"
    return [h[:n] for h, n in zip(host, sizes)]


# ---- output home x stream form ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("height,width", [(5, 17), (17, 5)])
@pytest.mark.parametrize("voxels", ["u8", "f32"])
@pytest.mark.parametrize("advanced", [False, True])
def test_slice_host_and_device_buffers_agree(loaded, torch_side, voxels, height, width, advanced):
    """vv_slice / vv_slice_advanced.  The kernels address element (row j, column i) as j * height + i.  5 x 17: width > height, so neighbouring rows
    overlap (the larger row wins) and only elements 0..36 are written; 17 x 5: only five rows fit, and 12 of every 17 elements are never written.
    What is not written keeps the caller's bytes."""
    ctx = loaded[voxels]
    sc = (C.c_float * 3)(1.0, 0.9, 1.1)
    trans = (C.c_float * 16)(*[float(v) for v in vv.slice_matrix(0.1, -0.05, 0.2, 0.3, 0.2, 0.1).reshape(16)])

    def call(ptrs, on_device, stream, inp):
        if advanced:
            return ctx.lib.vv_slice_advanced(ctx.h, ptrs[0], height, width, C.byref(trans), C.byref(sc), vv.FILTER_TEX8, on_device, stream)
        return ctx.lib.vv_slice(ctx.h, ptrs[0], height, width, 0.05, 0.1, 0.3, vv.CORONAL, C.byref(sc), 0, vv.FILTER_EXACT, on_device, stream)

    (img,) = _both_homes(torch_side, [height * width * 4], call)
    img = img.view(np.uint32)
    offsets = {j * height + i for j in range(height) for i in range(width) if j * height + i < height * width}      # (what slice_kernel writes)
    skipped = np.array(sorted(set(range(height * width)) - offsets), dtype=int)
    assert len(skipped) == {(5, 17): 85 - 37, (17, 5): 85 - 25}[(height, width)]
    assert np.all(img[skipped] == 0xA5A5A5A5) and np.all(img[sorted(offsets)] != 0xA5A5A5A5)
    assert np.any(img[sorted(offsets)] != 0), "the slice misses the volume: nothing is sampled"


def test_first_pass_host_and_device_buffers_agree(loaded, torch_side):
    ctx = loaded["fresh"]                                         # (needs no volume)
    W, H = 9, 7
    cam = vv.Camera.orbit(3.0, 1.0, 0.7)
    cp = cam.params(W, H); rs = vv.analytic_rays(cam)

    def call(ptrs, on_device, stream, inp):
        return ctx.lib.vv_first_pass(ctx.h, W, H, C.byref(cp), C.byref(rs), ptrs[0], ptrs[1], on_device, stream)

    front, back = _both_homes(torch_side, [W * H * 4, W * H * 4], call)
    assert np.any(back.view(np.uint32) != 0) and not np.array_equal(front, back), "the view should hit the cube"


@pytest.mark.parametrize("n", [0, 1, 1027])
@pytest.mark.parametrize("own_table", [False, True])
def test_classify_host_and_device_buffers_agree(loaded, torch_side, n, own_table):
    """vv_classify_indices through the context's table and through a table of the call's own (always a host pointer); n = 0 stages nothing."""
    ctx = loaded["u8"]
    index = np.random.default_rng(n).integers(0, 256, max(n, 1), dtype=np.uint8)      # (n = 0: a valid pointer nobody reads)
    tf = vv.transfer_preset(vv.TF_MRI) if own_table else None

    def call(ptrs, on_device, stream, inp):
        return ctx.lib.vv_classify_indices(ctx.h, inp["index"], n, None if tf is None else tf.ctypes.data, ptrs[0], on_device, stream)

    (rgba,) = _both_homes(torch_side, [n * 4], call, {"index": index})
    if n > 1:
        assert len(np.unique(rgba.view(np.uint32))) > 1


GEN = (17, 16, 3)                                                 # rows of 17 voxels: one whole 16-voxel chunk and an unaligned tail


def test_generator_host_and_device_buffers_agree(loaded, torch_side):
    ctx = loaded["fresh"]
    nx, ny, nz = GEN

    def call(ptrs, on_device, stream, inp):
        return ctx.lib.vv_generate_default_brain(ctx.h, ptrs[0], on_device, nx, ny, nz, stream)

    (vol,) = _both_homes(torch_side, [nx * ny * nz], call)
    assert set(np.unique(vol)) > {0} and FILL not in vol, "a fresh volume is written whole"


def test_draw_in_place_host_and_device_buffers_agree(loaded, torch_side):
    """vv_draw_ellipsoid draws into the volume it is given: here one of FILL bytes, which the voxels outside the ellipsoid keep in both homes."""
    ctx = loaded["fresh"]
    nx, ny, nz = GEN
    center = np.array([0.5, 0.5, 0.5], np.float32); axes = np.array([0.3, 0.35, 0.4], np.float32)

    def call(ptrs, on_device, stream, inp):
        return ctx.lib.vv_draw_ellipsoid(ctx.h, ptrs[0], on_device, nx, ny, nz, center.ctypes.data, axes.ctypes.data, 200, stream)

    (vol,) = _both_homes(torch_side, [nx * ny * nz], call)
    assert 200 in vol and FILL in vol


def test_draw_in_place_uploads_the_host_volume(loaded):
    """vv_draw_ellipsoid on a host volume of 20 x 6 x 3 that holds a byte pattern (rows of 20: a 16-voxel chunk and a tail): the call's staging buffer
    starts as the caller's bytes, so the result is that of the same call on a device copy of the volume, and the voxels outside the ellipsoid keep
    their bytes in both."""
    import torch
    ctx = loaded["fresh"]
    nx, ny, nz = 20, 6, 3
    color = 200
    pattern = (1 + np.arange(nx * ny * nz) * 37 % 199).astype(np.uint8)                    # 1..199: never the colour
    assert len(np.unique(pattern)) > 100 and color not in pattern
    center = np.array([0.45, 0.5, 0.5], np.float32); axes = np.array([0.3, 0.35, 0.4], np.float32)
    host = pattern.copy()
    dev = torch.from_numpy(pattern.copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    for ptr, on_device in ((host.ctypes.data, 0), (dev.data_ptr(), 1)):
        assert ctx.lib.vv_draw_ellipsoid(ctx.h, ptr, on_device, nx, ny, nz, center.ctypes.data, axes.ctypes.data, color, None) == 0
    assert np.array_equal(host, dev.cpu().numpy()), "the host volume differs from the device volume"
    inside = host == color
    assert 0 < inside.sum() < host.size and np.array_equal(host[~inside], pattern[~inside]), "voxels outside the ellipsoid lost their bytes"


# ---- error precedence ------------------------------------------------------------------------------------------------------------------------

_SC = (C.c_float * 3)(1.0, 1.0, 1.0)
_TRANS = (C.c_float * 16)(*([0.0] * 16))
_BUF = np.zeros(64, np.float32)
_AUX = np.zeros(64, np.int32)
_BYTES = np.zeros(4096, np.uint8)
_NAN_TF = np.full(1024, np.nan, np.float32)
_HIST = vv.vv_histogram()
_LO = (C.c_int * 3)(0, 0, 0)
_BAD_HI = (C.c_int * 3)(0, 99, 99)
_HUGE = 65535 * 16 + 1


def _slab(mode=vv.SLAB_MAX, samples=1, thickness=0.0):
    return C.byref(vv.vv_slab(mode, samples, thickness))


def _cam(scale=(1.0, 1.0, 1.0)):
    cp = vv.Camera().params(8, 8)
    cp.scale[:] = scale
    return C.byref(cp)


def _rays(mode=vv.RAYS_ANALYTIC, look=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)):
    rs = vv.vv_ray_source()
    rs.mode = mode; rs.look[:] = look; rs.up[:] = up
    return C.byref(rs)


def _p(a):
    return a.ctypes.data


# (call name, context, arguments behind the context, expected code, expected vv_last_error).  Contexts: "fresh" has no volume and no transfer
# function, "u8" has both, "null" is a NULL context (its text is read with vv_last_error(NULL)); "dev+1" / "dev+4" stand for a device pointer
# that is misaligned by one byte / four bytes.
ERROR_CASES = [
    # vv_slice: scale, context, buffer, volume, size
    ("vv_slice", "null", (None, 0, 0, 0., 0., 0., vv.SAGITTAL, None, 0, 0, 0, None), INVALID, "vv_slice: NULL scale"),
    ("vv_slice", "null", (None, 0, 0, 0., 0., 0., vv.SAGITTAL, _SC, 0, 0, 0, None), INVALID, "vv_slice: NULL context"),
    ("vv_slice", "fresh", (None, 4, 4, 0., 0., 0., vv.SAGITTAL, None, 0, 0, 0, None), INVALID, "vv_slice: NULL scale"),
    ("vv_slice", "fresh", (None, 4, 4, 0., 0., 0., vv.SAGITTAL, _SC, 0, 0, 0, None), INVALID, "vv_slice: NULL buffer"),
    ("vv_slice", "fresh", (_p(_BUF), 0, 4, 0., 0., 0., vv.SAGITTAL, _SC, 0, 0, 0, None), NO_VOLUME, "vv_slice: no volume loaded"),
    ("vv_slice", "u8", (None, 4, 0, 0., 0., 0., vv.SAGITTAL, _SC, 0, 0, 0, None), INVALID, "vv_slice: NULL buffer"),
    ("vv_slice", "u8", (_p(_BUF), _HUGE, 0, 0., 0., 0., vv.SAGITTAL, _SC, 0, 0, 0, None), INVALID, "vv_slice: bad buffer size"),
    # vv_slice_advanced: scale / trans, then vv_slice's checks under vv_slice's name
    ("vv_slice_advanced", "fresh", (None, 4, 4, None, _SC, 0, 0, None), INVALID, "vv_slice_advanced: NULL argument"),
    ("vv_slice_advanced", "null", (None, 4, 4, _TRANS, None, 0, 0, None), INVALID, "vv_slice_advanced: NULL argument"),
    ("vv_slice_advanced", "null", (None, 4, 4, _TRANS, _SC, 0, 0, None), INVALID, "vv_slice: NULL context"),
    ("vv_slice_advanced", "fresh", (None, 4, 4, _TRANS, _SC, 0, 0, None), INVALID, "vv_slice: NULL buffer"),
    ("vv_slice_advanced", "fresh", (_p(_BUF), 4, 0, _TRANS, _SC, 0, 0, None), NO_VOLUME, "vv_slice: no volume loaded"),
    ("vv_slice_advanced", "u8", (_p(_BUF), 0, _HUGE, _TRANS, _SC, 0, 0, None), INVALID, "vv_slice: bad buffer size"),
    # vv_slice_slab: context, scale / slab, orientation, buffer, mode, samples, thickness, size, device aux, volume
    ("vv_slice_slab", "null", (None, None, 4, 4, 0., 0., 0., 7, None, 0, None, 0, None), INVALID, "vv_slice_slab: NULL context"),
    ("vv_slice_slab", "fresh", (None, None, 4, 4, 0., 0., 0., 7, _SC, 0, None, 0, None), INVALID, "vv_slice_slab: NULL argument"),
    ("vv_slice_slab", "fresh", (None, None, 4, 4, 0., 0., 0., 7, _SC, 0, _slab(), 0, None), INVALID,
     "vv_slice_slab: orientation must be VV_SAGITTAL, VV_HORIZONTAL or VV_CORONAL"),
    ("vv_slice_slab", "fresh", (None, None, 4, 4, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(mode=9), 0, None), INVALID, "vv_slice_slab: NULL buffer"),
    ("vv_slice_slab", "fresh", (_p(_BUF), None, 4, 4, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(mode=9, samples=0), 0, None), INVALID,
     "vv_slice_slab: mode must be VV_SLAB_MAX, VV_SLAB_MIN or VV_SLAB_MEAN"),
    ("vv_slice_slab", "fresh", (_p(_BUF), None, 4, 4, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(samples=2000, thickness=-1.0), 0, None), INVALID,
     "vv_slice_slab: samples must lie in 1..1024"),
    ("vv_slice_slab", "fresh", (_p(_BUF), None, 0, 4, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(thickness=float("nan")), 0, None), INVALID,
     "vv_slice_slab: thickness must be finite and >= 0"),
    ("vv_slice_slab", "fresh", (_p(_BUF), None, 4, 0, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(), 0, None), INVALID, "vv_slice_slab: bad buffer size"),
    ("vv_slice_slab", "fresh", ("dev+4", "dev+1", 4, 4, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(), 1, None), INVALID,
     "vv_slice_slab: a device aux must be 4-byte aligned"),
    ("vv_slice_slab", "u8", ("dev+4", "dev+1", 4, _HUGE, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(), 1, None), INVALID, "vv_slice_slab: bad buffer size"),
    ("vv_slice_slab", "fresh", (_p(_BUF), _p(_AUX), 4, 4, 0., 0., 0., vv.CORONAL, _SC, 0, _slab(), 0, None), NO_VOLUME, "vv_slice_slab: no volume loaded"),
    # vv_slice_advanced_slab: context, scale / trans / slab, then vv_slice_slab's checks under vv_slice_slab's name
    ("vv_slice_advanced_slab", "null", (None, None, 4, 4, None, _SC, 0, _slab(), 0, None), INVALID, "vv_slice_advanced_slab: NULL context"),
    ("vv_slice_advanced_slab", "fresh", (None, None, 4, 4, None, _SC, 0, _slab(), 0, None), INVALID, "vv_slice_advanced_slab: NULL argument"),
    ("vv_slice_advanced_slab", "fresh", (None, None, 4, 4, _TRANS, _SC, 0, _slab(mode=9), 0, None), INVALID, "vv_slice_slab: NULL buffer"),
    ("vv_slice_advanced_slab", "fresh", (_p(_BUF), None, 4, 4, _TRANS, _SC, 0, _slab(samples=0, thickness=float("inf")), 0, None), INVALID,
     "vv_slice_slab: samples must lie in 1..1024"),
    ("vv_slice_advanced_slab", "fresh", (_p(_BUF), None, 0, 4, _TRANS, _SC, 0, _slab(), 0, None), INVALID, "vv_slice_slab: bad buffer size"),
    # vv_classify_indices: context, index / output, table
    ("vv_classify_indices", "null", (None, 8, None, None, 0, None), INVALID, "vv_classify_indices: NULL context"),
    ("vv_classify_indices", "fresh", (None, 8, None, _p(_BYTES), 0, None), INVALID, "vv_classify_indices: NULL argument"),
    ("vv_classify_indices", "fresh", (_p(_BYTES), 8, _p(_NAN_TF), None, 0, None), INVALID, "vv_classify_indices: NULL argument"),
    ("vv_classify_indices", "fresh", (_p(_BYTES), 8, None, _p(_BYTES), 0, None), NO_VOLUME, "vv_classify_indices: no transfer function loaded"),
    ("vv_classify_indices", "u8", (_p(_BYTES), 8, _p(_NAN_TF), None, 0, None), INVALID, "vv_classify_indices: NULL argument"),
    ("vv_classify_indices", "u8", (_p(_BYTES), 8, _p(_NAN_TF), _p(_BYTES), 0, None), INVALID, "vv_classify_indices: transfer function must be finite"),
    # vv_first_pass: context, pointers and size, ray source, camera scale, camera basis
    ("vv_first_pass", "null", (0, 8, None, None, None, None, 0, None), INVALID, "vv_first_pass: NULL context"),
    ("vv_first_pass", "fresh", (8, 8, _cam(), _rays(mode=vv.RAYS_IMAGES), None, _p(_BYTES), 0, None), INVALID, "vv_first_pass: bad argument"),
    ("vv_first_pass", "fresh", (0, 8, _cam(scale=(0.0, 1.0, 1.0)), _rays(), _p(_BYTES), _p(_BYTES), 0, None), INVALID, "vv_first_pass: bad argument"),
    ("vv_first_pass", "fresh", (8, 8, _cam(scale=(1.0, float("nan"), 1.0)), _rays(mode=vv.RAYS_IMAGES), _p(_BYTES), _p(_BYTES), 0, None), INVALID,
     "vv_first_pass: needs an analytic ray source"),
    ("vv_first_pass", "fresh", (8, 8, _cam(scale=(1.0, 1.0, -1.0)), _rays(look=(0.0, 0.0, 0.0)), _p(_BYTES), _p(_BYTES), 0, None), INVALID,
     "vv_first_pass: camera scale must be finite and > 0"),
    ("vv_first_pass", "fresh", (8, 8, _cam(), _rays(look=(0.0, 0.0, 0.0), up=(0.0, 0.0, 0.0)), _p(_BYTES), _p(_BYTES), 0, None), INVALID,
     "vv_render: look vector is zero"),
    ("vv_first_pass", "fresh", (8, 8, _cam(), _rays(look=(0.0, 2.0, 0.0), up=(0.0, 1.0, 0.0)), _p(_BYTES), _p(_BYTES), 0, None), INVALID,
     "vv_render: up vector is parallel to look"),
    # vv_volume_histogram: context, out, box pointers, device alignment, volume, box
    ("vv_volume_histogram", "null", (_LO, None, None, 0, None), INVALID, "vv_volume_histogram: NULL context"),
    ("vv_volume_histogram", "fresh", (_LO, None, None, 0, None), INVALID, "vv_volume_histogram: NULL out"),
    ("vv_volume_histogram", "fresh", (_LO, None, C.addressof(_HIST), 0, None), INVALID,
     "vv_volume_histogram: box_lo and box_hi must both be given or both be NULL"),
    ("vv_volume_histogram", "u8", (None, _BAD_HI, "dev+4", 1, None), INVALID, "vv_volume_histogram: box_lo and box_hi must both be given or both be NULL"),
    ("vv_volume_histogram", "fresh", (None, None, "dev+4", 1, None), INVALID, "vv_volume_histogram: a device out must be 8-byte aligned"),
    ("vv_volume_histogram", "u8", (_LO, _BAD_HI, "dev+4", 1, None), INVALID, "vv_volume_histogram: a device out must be 8-byte aligned"),
    ("vv_volume_histogram", "fresh", (_LO, _BAD_HI, C.addressof(_HIST), 0, None), NO_VOLUME, "vv_volume_histogram: no volume loaded"),
    ("vv_volume_histogram", "u8", (_LO, _BAD_HI, C.addressof(_HIST), 0, vv.STREAM_DEFAULT_ASYNC), INVALID,
     "vv_volume_histogram: the box must satisfy 0 <= lo < hi <= dims on every axis"),
    # vv_histogram_indices: context, counts / index, device alignment
    ("vv_histogram_indices", "null", (None, 5, None, 0, None), INVALID, "vv_histogram_indices: NULL context"),
    ("vv_histogram_indices", "fresh", (None, 5, None, 0, None), INVALID, "vv_histogram_indices: NULL argument"),
    ("vv_histogram_indices", "fresh", (None, 5, "dev+4", 1, None), INVALID, "vv_histogram_indices: NULL argument"),
    ("vv_histogram_indices", "fresh", (None, 0, "dev+4", 1, None), INVALID, "vv_histogram_indices: device counts must be 8-byte aligned"),
    # vv_generate_ellipsoids: context, pointers / sizes / count, chunks of a slice
    ("vv_generate_ellipsoids", "null", (None, 0, 0, 4, 4, 65, None, None, None, None), INVALID, "vv_generate_ellipsoids: NULL context"),
    ("vv_generate_ellipsoids", "fresh", (None, 0, 4, 4, 4, 65, None, None, None, None), INVALID, "vv_generate_ellipsoids: bad argument (n <= 64)"),
    ("vv_generate_ellipsoids", "fresh", (_p(_BYTES), 0, 2 ** 31 - 1, 16, 1, 65, None, None, None, None), INVALID,
     "vv_generate_ellipsoids: bad argument (n <= 64)"),
    ("vv_generate_ellipsoids", "fresh", (_p(_BYTES), 0, 2 ** 31 - 1, 16, 1, 1, None, _p(_BUF), _p(_BYTES), None), INVALID,
     "vv_generate_ellipsoids: bad argument (n <= 64)"),
    ("vv_generate_ellipsoids", "fresh", (_p(_BYTES), 0, 2 ** 31 - 1, 16, 0, -1, None, None, None, None), INVALID,
     "vv_generate_ellipsoids: bad argument (n <= 64)"),
    # vv_load_volume_stream_begin: context, dimensions / type, slice limit, row limit -- all before the old volume is given up and anything is allocated
    ("vv_load_volume_stream_begin", "null", (7, 0, 1, 1, None), INVALID, "stream_begin: NULL context"),
    ("vv_load_volume_stream_begin", "u8", (7, 0, 1, 1, None), INVALID, "stream_begin: bad dims / voxel type"),
    ("vv_load_volume_stream_begin", "u8", (7, 65536, 65536, 1, None), INVALID, "stream_begin: bad dims / voxel type"),
    ("vv_load_volume_stream_begin", "u8", (vv.VOXEL_U8, 2 ** 24, 1, -1, None), INVALID, "stream_begin: bad dims / voxel type"),
    ("vv_load_volume_stream_begin", "u8", (vv.VOXEL_U8, 65536, 65536, 1, None), INVALID, "stream_begin: one slice must stay below 4 GiB"),
    ("vv_load_volume_stream_begin", "u8", (vv.VOXEL_F32, 2 ** 24, 2 ** 8, 1, None), INVALID, "stream_begin: one slice must stay below 4 GiB"),
    ("vv_load_volume_stream_begin", "u8", (vv.VOXEL_U8, 2 ** 24, 1, 1, None), INVALID,
     "stream_begin: a volume row must be below 16 MiB and each dimension below 2^24"),
    ("vv_load_volume_stream_begin", "fresh", (vv.VOXEL_U8, 2 ** 24, 1, 2 ** 24, None), INVALID,
     "stream_begin: a volume row must be below 16 MiB and each dimension below 2^24"),
    ("vv_load_volume_stream_begin", "u8", (vv.VOXEL_F32, 2 ** 22, 1, 2 ** 24, None), INVALID,
     "stream_begin: a volume row must be below 16 MiB and each dimension below 2^24"),
]


# ---- the label, mask, distance, region-table and mesh calls: each call's refusal order walked from end to end, two adjacent steps violated per row ----
# Device rows lay their buffers out in the 4096 bytes behind "dev+0"; the box is 4 x 4 x 4 (64 voxels, 256 bytes of words), so the site grid
# without a cap is 3 x 3 x 3 (108 bytes of index).  Not reachable here: the 2^32 - 2 voxel / site limits and vv_distance_volume's extent
# above 2048 (no such volume is loaded), the overlap of an output with the loaded volume (no public call tells the allocation's address),
# and the accepted out == labels alias of vv_distance_volume (it reaches a launch: tests/test_distance.py has it).
_BOX = ((0, 0, 0), (4, 4, 4))
_BAD_BOX = ((0, 0, 0), (4, 99, 4))
_WORDS = 256                                  # bytes of a word-per-voxel array of _BOX
_DIMS = (C.c_int * 3)()
_NAN = float("nan")


def _desc(cls, box=_BOX, **fields):
    d = cls()
    d.box_lo[:], d.box_hi[:] = box
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return C.byref(d)


def _label(box=_BOX, bins=(3, 9), connectivity=6):
    return _desc(vv.vv_label, box, bin_lo=bins[0], bin_hi=bins[1], connectivity=connectivity)


def _mask(box=_BOX, out_type=vv.VOXEL_U8, keep=vv.KEEP_FOREGROUND, invert=0, fill=0.0):
    return _desc(vv.vv_mask, box, out_type=out_type, keep=keep, invert=invert, fill=fill)


def _dist(box=_BOX, seed=vv.SEED_NONZERO, bins=(3, 9), invert=0, spacing=(1, 1, 1), out=vv.DIST_SQUARED):
    return _desc(vv.vv_distance, box, seed=seed, bin_lo=bins[0], bin_hi=bins[1], invert=invert, spacing=spacing, out=out)


def _regions(box=_BOX, source=vv.REGION_LABELS, max_regions=2):
    return _desc(vv.vv_regions, box, source=source, max_regions=max_regions)


def _mesh(box=_BOX, source=vv.MESH_NONZERO, level=1, bins=(3, 9), cap=0, max_vertices=4, max_quads=4):
    return _desc(vv.vv_mesh, box, source=source, level=level, bin_lo=bins[0], bin_hi=bins[1], cap=cap, max_vertices=max_vertices, max_quads=max_quads)


_H = _p(_BYTES)                               # a host pointer no refused call reads
_ROW = C.sizeof(vv.vv_region)
# device layouts: region table {labels 0, aux 256, compact 512, table 1024 (2 rows), summary 2048}; mesh {labels 0, index 256, vertices 512,
# normals 640, quads 768 (4 records of 16 bytes each), summary 1024}
_RL, _RA, _RC, _RT, _RS = "dev+0", "dev+256", "dev+512", "dev+1024", "dev+2048"
_ML, _MI, _MV, _MN, _MQ, _MS = "dev+0", "dev+256", "dev+512", "dev+640", "dev+768", "dev+1024"

ERROR_CASES += [
    # vv_label_volume (rule 9): context, d / labels, volume, box, bins, connectivity, capacity, 4-byte alignment, stats alignment, labels / sizes overlap
    ("vv_label_volume", "null", (None, _H, _WORDS, None, None, 0, None), INVALID, "vv_label_volume: NULL context"),
    ("vv_label_volume", "fresh", (None, _H, _WORDS, None, None, 0, None), INVALID, "vv_label_volume: NULL argument"),
    ("vv_label_volume", "fresh", (_label(), None, _WORDS, None, None, 0, None), INVALID, "vv_label_volume: NULL argument"),
    ("vv_label_volume", "fresh", (_label(box=_BAD_BOX), _H, _WORDS, None, None, 0, None), NO_VOLUME, "vv_label_volume: no volume loaded"),
    ("vv_label_volume", "u8", (_label(box=_BAD_BOX, bins=(9, 3)), _H, _WORDS, None, None, 0, None), INVALID,
     "vv_label_volume: the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)"),
    ("vv_label_volume", "u8", (_label(bins=(9, 3), connectivity=8), _H, _WORDS, None, None, 0, None), INVALID,
     "vv_label_volume: bins must satisfy 0 <= bin_lo <= bin_hi <= 255"),
    ("vv_label_volume", "f32", (_label(bins=(0, 256), connectivity=8), _H, _WORDS, None, None, 0, None), INVALID,
     "vv_label_volume: bins must satisfy 0 <= bin_lo <= bin_hi <= 255"),
    ("vv_label_volume", "u8", (_label(connectivity=8), _H, _WORDS - 1, None, None, 0, None), INVALID, "vv_label_volume: connectivity must be 6, 18 or 26"),
    ("vv_label_volume", "u8", (_label(), "dev+1", _WORDS - 1, None, None, 1, None), INVALID, "vv_label_volume: capacity is below 4 bytes per voxel of the box"),
    ("vv_label_volume", "u8", (_label(), "dev+1", _WORDS, None, "dev+2052", 1, None), INVALID, "vv_label_volume: device labels and sizes must be 4-byte aligned"),
    ("vv_label_volume", "u8", (_label(), "dev+0", _WORDS, "dev+514", "dev+2052", 1, None), INVALID, "vv_label_volume: device labels and sizes must be 4-byte aligned"),
    ("vv_label_volume", "u8", (_label(), "dev+0", _WORDS, "dev+128", "dev+2052", 1, None), INVALID, "vv_label_volume: a device stats must be 8-byte aligned"),
    ("vv_label_volume", "f32", (_label(), "dev+128", _WORDS, "dev+0", "dev+2048", 1, None), INVALID, "vv_label_volume: labels and sizes overlap"),
    # vv_mask_volume (rule M5): context, m / labels / out, volume, box, out_type, keep, invert, fill, sizes under VV_KEEP_MIN_SIZE, capacity, a device
    # f32 out's alignment, labels / sizes alignment, out over labels or sizes
    ("vv_mask_volume", "null", (None, _H, None, _H, 64, 0, None), INVALID, "vv_mask_volume: NULL context"),
    ("vv_mask_volume", "fresh", (None, _H, None, _H, 64, 0, None), INVALID, "vv_mask_volume: NULL argument"),
    ("vv_mask_volume", "fresh", (_mask(), None, None, _H, 64, 0, None), INVALID, "vv_mask_volume: NULL argument"),
    ("vv_mask_volume", "fresh", (_mask(), _H, None, None, 64, 0, None), INVALID, "vv_mask_volume: NULL argument"),
    ("vv_mask_volume", "fresh", (_mask(box=_BAD_BOX), _H, None, _H, 64, 0, None), NO_VOLUME, "vv_mask_volume: no volume loaded"),
    ("vv_mask_volume", "u8", (_mask(box=_BAD_BOX, out_type=7), _H, None, _H, 64, 0, None), INVALID,
     "vv_mask_volume: the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)"),
    ("vv_mask_volume", "u8", (_mask(out_type=7, keep=9), _H, None, _H, 64, 0, None), INVALID, "vv_mask_volume: out_type must be VV_VOXEL_U8 or VV_VOXEL_F32"),
    ("vv_mask_volume", "u8", (_mask(keep=9, invert=2), _H, None, _H, 64, 0, None), INVALID,
     "vv_mask_volume: keep must be VV_KEEP_LABEL, VV_KEEP_FOREGROUND or VV_KEEP_MIN_SIZE"),
    ("vv_mask_volume", "u8", (_mask(invert=2, fill=_NAN), _H, None, _H, 64, 0, None), INVALID, "vv_mask_volume: invert must be 0 or 1"),
    ("vv_mask_volume", "u8", (_mask(keep=vv.KEEP_MIN_SIZE, fill=_NAN), _H, None, _H, 64, 0, None), INVALID, "vv_mask_volume: fill must be finite"),
    ("vv_mask_volume", "u8", (_mask(keep=vv.KEEP_MIN_SIZE), _H, None, _H, 63, 0, None), INVALID, "vv_mask_volume: VV_KEEP_MIN_SIZE needs sizes"),
    ("vv_mask_volume", "f32", (_mask(out_type=vv.VOXEL_F32), "dev+0", None, "dev+1025", 255, 1, None), INVALID, "vv_mask_volume: capacity is below the output's bytes"),
    ("vv_mask_volume", "f32", (_mask(out_type=vv.VOXEL_F32), "dev+2", None, "dev+1025", 256, 1, None), INVALID, "vv_mask_volume: a device f32 out must be 4-byte aligned"),
    ("vv_mask_volume", "u8", (_mask(), "dev+2", None, "dev+3", 64, 1, None), INVALID, "vv_mask_volume: device labels and sizes must be 4-byte aligned"),
    ("vv_mask_volume", "u8", (_mask(), "dev+0", "dev+514", "dev+3", 64, 1, None), INVALID, "vv_mask_volume: device labels and sizes must be 4-byte aligned"),
    ("vv_mask_volume", "u8", (_mask(), "dev+0", None, "dev+255", 64, 1, None), INVALID, "vv_mask_volume: out overlaps labels or sizes (the pass is not in place)"),
    ("vv_mask_volume", "u8", (_mask(), "dev+0", "dev+512", "dev+500", 64, 1, None), INVALID, "vv_mask_volume: out overlaps labels or sizes (the pass is not in place)"),
    # vv_distance_volume (rule 10): context, d / out, volume, box, seed, bins, labels against the seed, invert, spacing, the squared-distance bound (one
    # term above 0xFFFF; the sum above 0xFFFFFFFE), out mode, capacity, alignment, out over labels; out == labels meets the alignment check like any pair
    ("vv_distance_volume", "null", (None, None, _H, _WORDS, 0, None), INVALID, "vv_distance_volume: NULL context"),
    ("vv_distance_volume", "fresh", (None, None, _H, _WORDS, 0, None), INVALID, "vv_distance_volume: NULL argument"),
    ("vv_distance_volume", "fresh", (_dist(), _H, None, _WORDS, 0, None), INVALID, "vv_distance_volume: NULL argument"),
    ("vv_distance_volume", "fresh", (_dist(box=_BAD_BOX), _H, _H, _WORDS, 0, None), NO_VOLUME, "vv_distance_volume: no volume loaded"),
    ("vv_distance_volume", "u8", (_dist(box=_BAD_BOX, seed=5), _H, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)"),
    ("vv_distance_volume", "u8", (_dist(seed=5, bins=(9, 3)), _H, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: seed must be VV_SEED_BINS, VV_SEED_LABEL or VV_SEED_NONZERO"),
    ("vv_distance_volume", "u8", (_dist(seed=vv.SEED_BINS, bins=(-1, 3)), _H, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: bins must satisfy 0 <= bin_lo <= bin_hi <= 255"),
    ("vv_distance_volume", "u8", (_dist(seed=vv.SEED_BINS, invert=2), _H, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: labels must be NULL for VV_SEED_BINS and given for the labels sources"),
    ("vv_distance_volume", "f32", (_dist(seed=vv.SEED_LABEL, bins=(9, 3), invert=2), None, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: labels must be NULL for VV_SEED_BINS and given for the labels sources"),
    ("vv_distance_volume", "u8", (_dist(invert=2, spacing=(1, 0, 1)), _H, _H, _WORDS, 0, None), INVALID, "vv_distance_volume: invert must be 0 or 1"),
    ("vv_distance_volume", "u8", (_dist(spacing=(70000, 1, 0)), _H, _H, _WORDS, 0, None), INVALID, "vv_distance_volume: every spacing must be at least 1"),
    ("vv_distance_volume", "u8", (_dist(spacing=(1, 1, 70000), out=2), _H, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: the largest squared distance of the box, sum of (spacing (extent - 1))^2, must be at most 0xFFFFFFFE"),
    ("vv_distance_volume", "u8", (_dist(spacing=(21845, 21845, 1), out=2), _H, _H, _WORDS, 0, None), INVALID,
     "vv_distance_volume: the largest squared distance of the box, sum of (spacing (extent - 1))^2, must be at most 0xFFFFFFFE"),
    ("vv_distance_volume", "u8", (_dist(out=2), _H, _H, _WORDS - 1, 0, None), INVALID, "vv_distance_volume: out must be VV_DIST_SQUARED or VV_DIST_WITHIN"),
    ("vv_distance_volume", "u8", (_dist(), "dev+0", "dev+1026", _WORDS - 1, 1, None), INVALID, "vv_distance_volume: capacity is below 4 bytes per voxel of the box"),
    ("vv_distance_volume", "u8", (_dist(), "dev+4", "dev+2", _WORDS, 1, None), INVALID, "vv_distance_volume: device labels and out must be 4-byte aligned"),
    ("vv_distance_volume", "u8", (_dist(), "dev+1", "dev+4", _WORDS, 1, None), INVALID, "vv_distance_volume: device labels and out must be 4-byte aligned"),
    ("vv_distance_volume", "u8", (_dist(), "dev+2", "dev+2", _WORDS, 1, None), INVALID, "vv_distance_volume: device labels and out must be 4-byte aligned"),
    ("vv_distance_volume", "u8", (_dist(), "dev+4", "dev+0", _WORDS, 1, None), INVALID, "vv_distance_volume: out overlaps labels without being the same pointer"),
    ("vv_distance_volume", "f32", (_dist(), "dev+0", "dev+252", _WORDS, 1, None), INVALID, "vv_distance_volume: out overlaps labels without being the same pointer"),
    # vv_region_table (rule 8): context, d / labels / compact, volume, box, source, table NULL with rows, compact capacity, table capacity, 4-byte
    # alignment (labels, aux, compact), 8-byte alignment (table, summary), compact's overlaps, table's overlaps
    ("vv_region_table", "null", (None, _H, None, _H, _WORDS, None, 0, None, 0, None), INVALID, "vv_region_table: NULL context"),
    ("vv_region_table", "fresh", (None, _H, None, _H, _WORDS, None, 0, None, 0, None), INVALID, "vv_region_table: NULL argument"),
    ("vv_region_table", "fresh", (_regions(), None, None, _H, _WORDS, None, 0, None, 0, None), INVALID, "vv_region_table: NULL argument"),
    ("vv_region_table", "fresh", (_regions(), _H, None, None, _WORDS, None, 0, None, 0, None), INVALID, "vv_region_table: NULL argument"),
    ("vv_region_table", "fresh", (_regions(box=_BAD_BOX), _H, None, _H, _WORDS, None, 0, None, 0, None), NO_VOLUME, "vv_region_table: no volume loaded"),
    ("vv_region_table", "u8", (_regions(box=_BAD_BOX, source=4), _H, None, _H, _WORDS, None, 0, None, 0, None), INVALID,
     "vv_region_table: the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)"),
    ("vv_region_table", "u8", (_regions(source=4), _H, None, _H, _WORDS, None, 0, None, 0, None), INVALID,
     "vv_region_table: source must be VV_REGION_LABELS or VV_REGION_NONZERO"),
    ("vv_region_table", "u8", (_regions(), _H, None, _H, _WORDS - 1, None, 0, None, 0, None), INVALID, "vv_region_table: table is NULL with max_regions != 0"),
    ("vv_region_table", "u8", (_regions(), _H, None, _H, _WORDS - 1, _H, 2 * _ROW - 1, None, 0, None), INVALID,
     "vv_region_table: compact capacity is below 4 bytes per voxel of the box"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+513", _WORDS, _RT, 2 * _ROW - 1, _RS, 1, None), INVALID,
     "vv_region_table: table capacity is below sizeof(vv_region) * max_regions"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+514", _WORDS, "dev+1028", 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: device labels, aux and compact must be 4-byte aligned"),
    ("vv_region_table", "u8", (_regions(), "dev+1", _RA, _RC, _WORDS, "dev+1028", 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: device labels, aux and compact must be 4-byte aligned"),
    ("vv_region_table", "u8", (_regions(), _RL, "dev+258", _RC, _WORDS, "dev+1028", 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: device labels, aux and compact must be 4-byte aligned"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+252", _WORDS, "dev+1028", 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: a device table and summary must be 8-byte aligned"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+252", _WORDS, _RT, 2 * _ROW, "dev+2052", 1, None), INVALID,
     "vv_region_table: a device table and summary must be 8-byte aligned"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+252", _WORDS, "dev+248", 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: compact overlaps labels, aux, table or the loaded volume"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+508", _WORDS, "dev+248", 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: compact overlaps labels, aux, table or the loaded volume"),
    ("vv_region_table", "f32", (_regions(), _RL, None, "dev+1020", _WORDS, _RT, 2 * _ROW, _RS, 1, None), INVALID,
     "vv_region_table: compact overlaps labels, aux, table or the loaded volume"),
    ("vv_region_table", "u8", (_regions(), _RL, _RA, "dev+2048", _WORDS, "dev+248", 2 * _ROW, None, 1, None), INVALID,
     "vv_region_table: table overlaps labels, aux or the loaded volume"),
    ("vv_region_table", "u8", (_regions(), "dev+2048", _RA, "dev+3072", _WORDS, "dev+504", 2 * _ROW, None, 1, None), INVALID,
     "vv_region_table: table overlaps labels, aux or the loaded volume"),
    # vv_mesh_dims (rule 11 up to the site grid, then cap): context, d / out_dims, volume, box, cap
    ("vv_mesh_dims", "null", (None, _DIMS), INVALID, "vv_mesh_dims: NULL context"),
    ("vv_mesh_dims", "fresh", (None, _DIMS), INVALID, "vv_mesh_dims: NULL argument"),
    ("vv_mesh_dims", "fresh", (_mesh(box=_BAD_BOX), None), INVALID, "vv_mesh_dims: NULL argument"),
    ("vv_mesh_dims", "fresh", (_mesh(box=_BAD_BOX), _DIMS), NO_VOLUME, "vv_mesh_dims: no volume loaded"),
    ("vv_mesh_dims", "u8", (_mesh(box=_BAD_BOX, cap=2), _DIMS), INVALID, "vv_mesh_dims: the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)"),
    ("vv_mesh_dims", "f32", (_mesh(cap=2), _DIMS), INVALID, "vv_mesh_dims: cap must be 0 or 1"),
    # vv_surface_mesh (rule 11): context, d, volume, box, source, level, bins, labels against the source, cap, index / vertices / quads NULL with a
    # maximum, the three capacities, 4-byte (labels, index), 16-byte (vertices, normals, quads) and 8-byte (summary) alignment, one overlap per output
    ("vv_surface_mesh", "null", (None, None, None, 0, None, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: NULL context"),
    ("vv_surface_mesh", "fresh", (None, None, None, 0, None, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: NULL argument"),
    ("vv_surface_mesh", "fresh", (_mesh(box=_BAD_BOX), _H, None, 0, None, 0, None, None, 0, None, 0, None), NO_VOLUME, "vv_surface_mesh: no volume loaded"),
    ("vv_surface_mesh", "u8", (_mesh(box=_BAD_BOX, source=9), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)"),
    ("vv_surface_mesh", "u8", (_mesh(source=9, level=0, bins=(9, 3), cap=2), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: source must be VV_MESH_INDEX, VV_MESH_BINS, VV_MESH_LABEL or VV_MESH_NONZERO"),
    ("vv_surface_mesh", "u8", (_mesh(source=vv.MESH_INDEX, level=0, bins=(9, 3)), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: level must lie in 1..255"),
    ("vv_surface_mesh", "u8", (_mesh(source=vv.MESH_INDEX, level=256), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: level must lie in 1..255"),
    ("vv_surface_mesh", "u8", (_mesh(source=vv.MESH_BINS, level=0, bins=(9, 3)), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: bins must satisfy 0 <= bin_lo <= bin_hi <= 255"),
    ("vv_surface_mesh", "u8", (_mesh(source=vv.MESH_BINS, cap=2), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: labels must be given for the labels sources and NULL for VV_MESH_INDEX and VV_MESH_BINS"),
    ("vv_surface_mesh", "f32", (_mesh(source=vv.MESH_LABEL, level=0, bins=(9, 3), cap=2), None, None, 0, None, 0, None, None, 0, None, 0, None), INVALID,
     "vv_surface_mesh: labels must be given for the labels sources and NULL for VV_MESH_INDEX and VV_MESH_BINS"),
    ("vv_surface_mesh", "u8", (_mesh(cap=2), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: cap must be 0 or 1"),
    ("vv_surface_mesh", "u8", (_mesh(), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: index is NULL with a non-zero maximum"),
    ("vv_surface_mesh", "u8", (_mesh(max_vertices=0), _H, None, 0, None, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: index is NULL with a non-zero maximum"),
    ("vv_surface_mesh", "u8", (_mesh(), _H, _H, 0, None, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: vertices is NULL with max_vertices != 0"),
    ("vv_surface_mesh", "u8", (_mesh(), _H, _H, 0, _H, 0, None, None, 0, None, 0, None), INVALID, "vv_surface_mesh: quads is NULL with max_quads != 0"),
    ("vv_surface_mesh", "u8", (_mesh(), _H, _H, 107, _H, 63, None, _H, 63, None, 0, None), INVALID, "vv_surface_mesh: index capacity is below 4 bytes per site (vv_mesh_dims)"),
    ("vv_surface_mesh", "u8", (_mesh(), _H, _H, 108, _H, 63, None, _H, 63, None, 0, None), INVALID, "vv_surface_mesh: vertices capacity is below 16 bytes * max_vertices"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, "dev+258", 108, _MV, 64, None, _MQ, 63, None, 1, None), INVALID, "vv_surface_mesh: quads capacity is below 16 bytes * max_quads"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, "dev+258", 108, "dev+520", 64, None, _MQ, 64, None, 1, None), INVALID, "vv_surface_mesh: device labels and index must be 4-byte aligned"),
    ("vv_surface_mesh", "u8", (_mesh(), "dev+1", _MI, 108, "dev+520", 64, None, _MQ, 64, None, 1, None), INVALID, "vv_surface_mesh: device labels and index must be 4-byte aligned"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, _MI, 108, "dev+520", 64, None, _MQ, 64, "dev+1028", 1, None), INVALID,
     "vv_surface_mesh: device vertices, normals and quads must be 16-byte aligned"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, _MI, 108, _MV, 64, "dev+644", _MQ, 64, "dev+1028", 1, None), INVALID,
     "vv_surface_mesh: device vertices, normals and quads must be 16-byte aligned"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, _MI, 108, _MV, 64, None, "dev+776", 64, "dev+1028", 1, None), INVALID,
     "vv_surface_mesh: device vertices, normals and quads must be 16-byte aligned"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, "dev+252", 108, _MV, 64, None, _MQ, 64, "dev+1028", 1, None), INVALID, "vv_surface_mesh: a device summary must be 8-byte aligned"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, "dev+252", 108, "dev+240", 64, _MN, _MQ, 64, _MS, 1, None), INVALID,
     "vv_surface_mesh: index overlaps another buffer of the call or the loaded volume"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, _MI, 108, _MV, 64, "dev+560", "dev+608", 64, _MS, 1, None), INVALID,
     "vv_surface_mesh: vertices overlaps another buffer of the call or the loaded volume"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, _MI, 108, _MV, 64, _MN, "dev+688", 64, "dev+744", 1, None), INVALID,
     "vv_surface_mesh: normals overlaps another buffer of the call or the loaded volume"),
    ("vv_surface_mesh", "u8", (_mesh(), _ML, _MI, 108, _MV, 64, _MN, _MQ, 64, "dev+824", 1, None), INVALID,
     "vv_surface_mesh: quads overlaps another buffer of the call or the loaded volume"),
    ("vv_surface_mesh", "f32", (_mesh(), _ML, _MI, 108, _MV, 64, _MN, _MQ, 64, "dev+224", 1, None), INVALID,
     "vv_surface_mesh: summary overlaps another buffer of the call or the loaded volume"),
]


@pytest.mark.parametrize("case", range(len(ERROR_CASES)), ids=lambda k: f"{ERROR_CASES[k][0]}-{k}")
def test_error_precedence(loaded, torch_side, case):
    """Two bad arguments at once (or a NULL context and one): the call reports what it reported before its plumbing was shared -- code and text -- and
    touches nothing: the loaded volume is still there afterwards."""
    torch, _ = torch_side
    name, which, args, code, text = ERROR_CASES[case]
    raw = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", 0))              # real memory behind the misaligned device pointers
    args = tuple(raw.data_ptr() + int(a[4:]) if isinstance(a, str) else a for a in args)
    lib = loaded["fresh"].lib
    h = None if which == "null" else loaded[which].h
    assert getattr(lib, name)(h, *args) == code
    assert (lib.vv_last_error(h) or b"").decode() == text
    dims = (C.c_int * 3)()
    assert lib.vv_volume_dims(loaded["u8"].h, C.byref(dims), None) == 0 and tuple(dims) == (NX, NY, NZ)
    assert lib.vv_volume_dims(loaded["fresh"].h, C.byref(dims), None) == NO_VOLUME


# ---- scratch accounting ----------------------------------------------------------------------------------------------------------------------

def test_device_bytes_counts_the_generator_tables():
    """vv_device_bytes()[3] is "tables and scratch" (include/volviz.h): a call that makes the context allocate a scratch buffer raises it.  The generator's
    per-axis tables are such a buffer (the host volume itself goes through a buffer the call frees again)."""
    with vv.Context(0) as ctx:
        before = ctx.device_bytes()
        vol = ctx.generate_ellipsoids(16, 16, 16, [[0.5, 0.5, 0.5]], [[0.3, 0.3, 0.3]], [99])
        assert 99 in vol
        after = ctx.device_bytes()
        assert after[:3] == before[:3] == [0, 0, 0]
        assert after[3] > before[3]
