"""Volume and index-image histograms (vv_volume_histogram / vv_histogram_indices) against tests/hist_model.py, every field exactly.

CPU part: the model's bin of a voxel is the witness' classification at the voxel's centre (what ties the histogram to the march), its counts are
np.bincount on u8 volumes, the f32 special volume holds what it must, and the library and the binding export the calls.  GPU part: the kernel equals
the model on every volume, row shape, box, layout, launch geometry and load path -- floats compared as uint32 patterns, the output prefilled with
garbage -- and the calls leave the context alone."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import hist_model as HM
import volviz_amd as vv
import witness as Wt

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2                        # include/volviz.h: vv_status
GARBAGE = 0xA5                                             # the byte every output structure holds before a call
TF = np.linspace(0.0, 1.0, 1024, dtype=np.float32)
VOLUMES = ("aniso", "rand_u8", "rand_f32", "special_f32", "const7", "nan_f32")
ROW_NX = (1, 3, 15, 16, 17, 63, 64, 65, 257)
BOUNDARIES = (1, 2, 3, 127, 128, 254, 255)                 # k of the k / 255 boundaries the special volume straddles


def _special_values():
    """What the f32 special volume must contain (test_special_volume_is_not_trivial checks the volume itself)."""
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 2.0 ** 126, -(2.0 ** 126), -0.25, -3.0, 1.5, 7.0, 1.0]
    v = [f32(x) for x in v]
    for k in BOUNDARIES:
        b = f32(k) / f32(255)
        v += [b, np.nextafter(b, f32(-np.inf)), np.nextafter(b, f32(np.inf))]
    return np.array(v, f32)


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name == "aniso":                                        # few distinct values: the contended path
        v = np.fromfile(os.path.join(HERE, "golden", "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
    elif name == "rand_u8":
        v = np.random.default_rng(21).integers(0, 256, (11, 9, 13), dtype=np.uint8)
    elif name == "rand_f32":                                   # signed, inside the f32 value domain
        v = np.random.default_rng(22).normal(0.0, 1.0, (11, 9, 13)).astype(f32)
    elif name == "special_f32":
        rng = np.random.default_rng(23)
        v = rng.uniform(-0.5, 1.5, 11 * 9 * 13).astype(f32)
        sp = np.tile(_special_values(), 6)                      # every special value six times, scattered
        v[rng.choice(v.size, sp.size, replace=False)] = sp
        v = v.reshape(11, 9, 13)
    elif name == "const7":                                     # 81 920 voxels into one bin: a lost update shows
        v = np.full((20, 64, 64), 7, np.uint8)
    elif name == "nan_f32":                                    # the identity range
        v = np.full((2, 3, 5), np.nan, f32)
    elif name == "geometry":                                   # several trips of the grid-stride loop under VV_HIST_BLOCKS
        v = np.random.default_rng(24).integers(0, 256, (72, 80, 96), dtype=np.uint8)
    else:
        kind, nx = name.split(":")                             # "row_u8:17": ny = 3, nz = 2
        rng = np.random.default_rng(100 + int(nx))
        v = rng.integers(0, 256, (2, 3, int(nx)), dtype=np.uint8) if kind == "row_u8" else rng.normal(0.3, 0.5, (2, 3, int(nx))).astype(f32)
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


def _boxes(shape, seed):
    """whole; one voxel; one row; one slice; x starting at 1, 5, 15 and 17 (where the volume is that wide); 12 random boxes"""
    nz, ny, nx = shape
    out = [None, ((nx // 2, ny // 2, nz // 2), (nx // 2 + 1, ny // 2 + 1, nz // 2 + 1)), ((0, ny - 1, nz // 2), (nx, ny, nz // 2 + 1)),
           ((0, 0, nz - 1), (nx, ny, nz))]
    for x0 in (1, 5, 15, 17):
        if x0 < nx:
            out.append(((x0, 0, 0), (nx, ny, nz)))
            out.append(((x0, min(1, ny - 1), 0), (max(x0 + 1, nx - 1), ny, nz)))
    rng = np.random.default_rng(seed)
    for _ in range(12):
        lo = [int(rng.integers(0, n)) for n in (nx, ny, nz)]
        hi = [int(rng.integers(l + 1, n + 1)) for l, n in zip(lo, (nx, ny, nz))]
        out.append((tuple(lo), tuple(hi)))
    return out


@functools.lru_cache(maxsize=None)
def _want(volname, box):
    """The model's histogram of one (volume, box): computed once, shared by the tests."""
    h = HM.histogram(_volume(volname), box)
    h.counts.setflags(write=False)
    return h


def _bits(x):
    return int(np.asarray(x, f32).reshape(1).view(np.uint32)[0])


def _same(got, want, what):
    bad = np.flatnonzero(np.asarray(got.counts, np.uint64) != want.counts)
    assert len(bad) == 0, f"{what}: {len(bad)} bins differ, first {bad[0]}: {got.counts[bad[0]]} vs {want.counts[bad[0]]}"
    assert got.voxels == want.voxels == int(want.counts.sum()), f"{what}: voxels {got.voxels} vs {want.voxels}"
    assert got.nan_voxels == want.nan_voxels, f"{what}: nan_voxels {got.nan_voxels} vs {want.nan_voxels}"
    assert _bits(got.vmin) == _bits(want.vmin), f"{what}: vmin {got.vmin!r} ({_bits(got.vmin):#x}) vs {want.vmin!r} ({_bits(want.vmin):#x})"
    assert _bits(got.vmax) == _bits(want.vmax), f"{what}: vmax {got.vmax!r} ({_bits(got.vmax):#x}) vs {want.vmax!r} ({_bits(want.vmax):#x})"


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_histogram_calls():
    lib = vv.load_library()
    for name in ("vv_volume_histogram", "vv_histogram_indices"):
        assert name in vv.EXPORTS and hasattr(lib, name), f"{name} is not exported"
    for name in ("histogram", "histogram_device", "histogram_indices", "histogram_indices_device"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert C.sizeof(vv.vv_histogram) == 2072 and vv.vv_histogram.voxels.offset == 2048 and vv.vv_histogram.vmin.offset == 2064


def _centre_coords(n):
    """Texture coordinates of the n voxel centres of an axis, and whether each one is hit exactly.

    The sampler takes voxel coordinate fma(p, n, -0.5).  Among the binary32 neighbours of (x + .5) / n the one that gives x exactly is taken.
    Voxel 0 has none unless n is a power of two: there the neighbour that gives a coordinate just below 0 is taken, whose two clamped
    corners are both voxel 0, so the sample is the voxel whatever the weight.  A few other centres are not representable either (x = 3,
    26, 30 of 52; 3 of 13; 6 of 11): no sample can fall exactly on them, the nearest coordinate is returned and flagged."""
    p, exact = np.zeros(n, f32), np.zeros(n, bool)
    for x in range(n):
        p0 = (f32(x) + f32(0.5)) / f32(n)
        cands, a, b = [p0], p0, p0
        for _ in range(3):
            a, b = np.nextafter(a, f32(-1)), np.nextafter(b, f32(2))
            cands += [a, b]
        vc = [Wt.fma(c, f32(n), f32(-0.5)) for c in cands]
        hit = [c for c, v in zip(cands, vc) if v == f32(x)] or ([max(c for c, v in zip(cands, vc) if v < 0)] if x == 0 else [])
        p[x], exact[x] = (hit[0], True) if hit else (p0, False)
    return p, exact


@pytest.mark.parametrize("volname", ["aniso", "rand_u8", "rand_f32"])
def test_model_bin_is_the_witness_classification_at_the_voxel_centre(volname):
    """Pin 1: the bin of voxel (x, y, z) is the index a sample on its centre gets.  TEX8 (weights rounded to 1 / 256): every voxel.  EXACT
    (full binary32 weights): every voxel whose centre a binary32 coordinate can hit (_centre_coords), at least 80 % of each volume: 12 / 13 x 10 / 11 of the random ones."""
    assert callable(getattr(vv.Context, "histogram", None)), "Context.histogram is missing"       # the model describes a call the library must have
    vol = _volume(volname)
    nz, ny, nx = vol.shape
    (px, ex), (py, ey), (pz, ez) = _centre_coords(nx), _centre_coords(ny), _centre_coords(nz)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([px[x], py[y], pz[z]], axis=-1)
    on_centre = ex[x] & ey[y] & ez[z]
    assert on_centre.mean() >= 0.8 and on_centre[:, :, 0].any() and on_centre[0].any()
    want = HM.bins(vol)
    for filt in (Wt.FILTER_TEX8, Wt.FILTER_EXACT):
        got = Wt.classify(vol, p, filt)
        bad = np.argwhere((got != want) & (on_centre | (filt == Wt.FILTER_TEX8)))
        assert len(bad) == 0, f"{volname} filter {filt}: {len(bad)} voxels differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    assert len(np.unique(want)) > 3


@pytest.mark.parametrize("volname", ["aniso", "rand_u8", "const7", "geometry"])
def test_model_counts_are_bincount_on_u8(volname):
    assert hasattr(vv.load_library(), "vv_volume_histogram"), "vv_volume_histogram is not exported"
    vol = _volume(volname)
    for box in _boxes(vol.shape, 5):
        h = HM.histogram(vol, box)
        sub = HM.crop(vol, box)
        assert np.array_equal(h.counts, np.bincount(sub.ravel(), minlength=256).astype(np.uint64))
        assert h.voxels == sub.size and h.nan_voxels == 0 and h.vmin == sub.min() and h.vmax == sub.max()
    assert np.array_equal(HM.histogram_indices(vol), np.bincount(vol.ravel(), minlength=256).astype(np.uint64))


def test_special_volume_is_not_trivial():
    """NaN, both infinities, both zeros, a denormal, +-2^126, both sides of several k / 255 boundaries, negatives, values above 1: in the volume,
    and told apart by the model."""
    assert hasattr(vv.load_library(), "vv_volume_histogram"), "vv_volume_histogram is not exported"
    v = _volume("special_f32").ravel()
    u = v.view(np.uint32)
    assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any()
    assert (u == 0).any() and (u == 0x80000000).any()                                  # +0.0, -0.0
    assert ((u & 0x7F800000) == 0).any() and ((u & 0x7FFFFFFF) != 0)[(u & 0x7F800000) == 0].any()      # a denormal
    assert (v == f32(2.0 ** 126)).any() and (v == f32(-(2.0 ** 126))).any()
    assert (v < 0).any() and (v > 1).any()
    b = HM.bins(v)
    for k in BOUNDARIES:
        edge = f32(k) / f32(255)
        below, above = np.nextafter(edge, f32(-np.inf)), np.nextafter(edge, f32(np.inf))
        assert (v == below).any() and (v == above).any() and (v == edge).any()
        assert b[v == below][0] == k - 1 and b[v == above][0] == k                     # the two sides fall into different bins
    h = HM.histogram(_volume("special_f32"))
    assert h.nan_voxels == 6 and h.counts[0] > h.nan_voxels and h.counts[255] > 0
    assert _bits(h.vmin) == _bits(-np.inf) and _bits(h.vmax) == _bits(np.inf)
    # the order of the keys: -Inf < -2^126 < -denormal < -0 < +0 < +denormal < 2^126 < +Inf
    ladder = np.array([-np.inf, -(2.0 ** 126), -1e-40, -0.0, 0.0, 1e-40, 2.0 ** 126, np.inf], f32)
    assert np.all(np.diff(HM.keys(ladder).astype(np.int64)) > 0)
    lo, hi = HM.value_range(np.array([0.0, -0.0, 0.0], f32))
    assert _bits(lo) == 0x80000000 and _bits(hi) == 0
    lo, hi = HM.value_range(_volume("nan_f32"))
    assert _bits(lo) == 0x7F800000 and _bits(hi) == 0xFF800000


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_KNOBS = ("VV_PITCH_FORCE", "VV_PITCH_ROWS", "VV_PITCH_PAD", "VV_FORCE_BIG", "VV_HIST_BLOCKS")


def _load(ctx, monkeypatch, volname):
    for k in LAYOUT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    ctx.load_volume(_volume(volname), TF)                       # (the knobs are read at volume load)


@pytest.mark.gpu
@pytest.mark.parametrize("volname", VOLUMES)
def test_histogram_matches_model_on_every_box(ctx, volname, monkeypatch):
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    for box in _boxes(vol.shape, 31):
        want = _want(volname, box)
        got = ctx.histogram(box, prefill=GARBAGE)
        _same(got, want, f"{volname} box {box}")
        bx = box if box is not None else ((0, 0, 0), vol.shape[::-1])
        assert got.voxels == int(np.prod([h - l for l, h in zip(*bx)])) == int(got.counts.sum())
    whole = ctx.histogram(prefill=0)
    _same(whole, _want(volname, None), f"{volname} whole, zero prefill")
    if volname == "const7":
        assert whole.counts[7] == 81920 and whole.vmin == 7 and whole.vmax == 7
    if volname == "nan_f32":
        assert whole.nan_voxels == 30 and whole.counts[0] == 30 and _bits(whole.vmin) == 0x7F800000 and _bits(whole.vmax) == 0xFF800000


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["row_u8", "row_f32"])
@pytest.mark.parametrize("nx", ROW_NX)
def test_histogram_row_shapes(ctx, kind, nx, monkeypatch):
    """Head and tail masks of the 16-byte loads, and dense rows no vector load can be aligned to."""
    name = f"{kind}:{nx}"
    _load(ctx, monkeypatch, name)
    boxes = [None, ((0, 1, 0), (nx, 2, 2)), ((nx - 1, 0, 0), (nx, 3, 2)), ((nx // 3, 0, 1), (nx - nx // 4, 3, 2)), ((min(1, nx - 1), 1, 0), (nx, 3, 1))]
    for box in boxes:
        _same(ctx.histogram(box, prefill=GARBAGE), _want(name, box), f"{name} box {box}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nx", [("u8", 64), ("f32", 16)])
@pytest.mark.parametrize("knobs", [{"VV_PITCH_FORCE": "1"}, {"VV_PITCH_FORCE": "1", "VV_PITCH_ROWS": "1"}, {"VV_PITCH_FORCE": "1", "VV_FORCE_BIG": "1"}, {"VV_FORCE_BIG": "1"}])
def test_histogram_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume (32 bytes of zeros behind every row, with and without an extra row of zeros per slice) and the 64-bit addressing
    build: the padding is never counted -- no voxel is 0, so counts[0] must be 0."""
    for k in LAYOUT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ny, nz = 5, 4
    rng = np.random.default_rng(41)
    if kind == "u8":
        vol = rng.integers(1, 256, (nz, ny, nx), dtype=np.uint8)
    else:
        vol = (rng.integers(1, 256, (nz, ny, nx)).astype(f32) / f32(255)).astype(f32)
    with vv.Context(0) as ctx:                                  # a context created under the environment
        ctx.load_volume(vol, TF)
        dense = vol.nbytes + ny * nx * vol.itemsize + 2 * nx * vol.itemsize + 4096
        if "VV_PITCH_FORCE" in knobs:
            row = nx * vol.itemsize + 32
            rows = ny + 1 if "VV_PITCH_ROWS" in knobs else ny
            assert ctx.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096 != dense     # the volume is re-pitched
        else:
            assert ctx.device_bytes()[0] == dense
        for box in _boxes(vol.shape, 43):
            want = HM.histogram(vol, box)
            got = ctx.histogram(box, prefill=GARBAGE)
            _same(got, want, f"{kind} {knobs} box {box}")
            assert got.counts[0] == 0


@pytest.mark.gpu
def test_histogram_launch_geometry(ctx, monkeypatch):
    """VV_HIST_BLOCKS = 1, 3 and unset: 68, 23 and one trip of the grid-stride loop per wave on the whole volume (540 chunks, 8 waves per block);
    the same numbers."""
    _load(ctx, monkeypatch, "geometry")
    boxes = [None, ((3, 2, 1), (91, 77, 70)), ((0, 0, 5), (96, 80, 9)), ((16, 0, 0), (80, 80, 72))]
    try:
        for blocks in ("1", "3", None):
            if blocks is None:
                monkeypatch.delenv("VV_HIST_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("VV_HIST_BLOCKS", blocks)
            ctx.reread_env()
            for box in boxes:
                _same(ctx.histogram(box, prefill=GARBAGE), _want("geometry", box), f"VV_HIST_BLOCKS={blocks} box {box}")
            idx = _volume("geometry").ravel()[3:200003]
            assert np.array_equal(ctx.histogram_indices(idx), HM.histogram_indices(idx)), f"VV_HIST_BLOCKS={blocks} index image"
    finally:
        monkeypatch.delenv("VV_HIST_BLOCKS", raising=False)
        ctx.reread_env()


@pytest.mark.gpu
def test_histogram_load_paths(ctx, monkeypatch):
    import torch
    for k in LAYOUT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    dev = torch.device("cuda", 0)
    box = ((2, 1, 3), (11, 9, 10))
    for volname in ("rand_u8", "special_f32"):
        vol = _volume(volname)
        nz, ny, nx = vol.shape
        ctx.load_volume(vol, TF)
        _same(ctx.histogram(prefill=GARBAGE), _want(volname, None), f"{volname} load_volume")
        t = torch.from_numpy(vol.copy()).to(dev)
        ctx.load_volume_device(t.data_ptr(), vv.VOXEL_U8 if vol.dtype == np.uint8 else vv.VOXEL_F32, nx, ny, nz, TF)
        torch.cuda.synchronize()
        del t
        _same(ctx.histogram(prefill=GARBAGE), _want(volname, None), f"{volname} load_volume_device")
        _same(ctx.histogram(box, prefill=GARBAGE), _want(volname, box), f"{volname} load_volume_device, box")
    # streamed upload, u8 slabs promoted on the device: the model runs on v / 255 in binary32, whatever bins that gives
    vol8 = _volume("rand_u8")
    nz, ny, nx = vol8.shape
    promoted = (vol8.astype(f32) / f32(255)).astype(f32)
    ctx.load_volume_streamed([(4, vol8[4:]), (0, vol8[:4])], vv.VOXEL_F32, nx, ny, nz, TF)
    _same(ctx.histogram(prefill=GARBAGE), HM.histogram(promoted), "streamed upload with promotion")
    _same(ctx.histogram(box, prefill=GARBAGE), HM.histogram(promoted, box), "streamed upload with promotion, box")
    ctx.load_volume_streamed([(0, vol8)], vv.VOXEL_U8, nx, ny, nz, TF)
    _same(ctx.histogram(prefill=GARBAGE), _want("rand_u8", None), "streamed upload, u8")


def _device_hist(buf):
    return vv.Histogram.from_bytes(buf.cpu().numpy().tobytes())


@pytest.mark.gpu
def test_histogram_device_output(ctx, monkeypatch):
    import torch
    _load(ctx, monkeypatch, "special_f32")
    dev = torch.device("cuda", 0)
    box = ((1, 0, 2), (12, 8, 11))
    for ts in (torch.cuda.Stream(device=dev), torch.cuda.default_stream(dev)):
        bufs = [torch.full((2072,), GARBAGE, dtype=torch.uint8, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            ctx.histogram_device(bufs[0].data_ptr(), stream=vv.stream_handle(ts))          # enqueue only, two calls in a row
            ctx.histogram_device(bufs[1].data_ptr(), stream=vv.stream_handle(ts))
            ctx.histogram_device(bufs[2].data_ptr(), box, stream=vv.stream_handle(ts))
        ts.synchronize()
        assert torch.equal(bufs[0], bufs[1])
        _same(_device_hist(bufs[0]), _want("special_f32", None), "enqueue-only")
        _same(_device_hist(bufs[2]), _want("special_f32", box), "enqueue-only, box")
        host = ctx.histogram(prefill=GARBAGE)
        _same(_device_hist(bufs[0]), host, "device against host call")
    buf = torch.full((2072,), GARBAGE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.histogram_device(buf.data_ptr(), box)                       # no stream: complete on return
    _same(_device_hist(buf), _want("special_f32", box), "synchronous device call")


@pytest.mark.gpu
def test_histogram_of_index_images(ctx, monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(51)
    ts = torch.cuda.Stream(device=dev)
    for n in (0, 1, 15, 16, 17, 4097):
        idx = rng.integers(0, 256, n, dtype=np.uint8)
        idx[: n // 2] = 9                                           # half of it one value
        want = HM.histogram_indices(idx)
        assert np.array_equal(ctx.histogram_indices(idx), want), f"host, n = {n}"
        for off in (0, 3):                                          # a device image at any byte offset, 0xFF around it
            raw = torch.full((n + 64,), 255, dtype=torch.uint8, device=dev)
            raw[16 + off:16 + off + n] = torch.from_numpy(idx).to(dev)
            counts = torch.full((256,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                ctx.histogram_indices_device(raw.data_ptr() + 16 + off, n, counts.data_ptr(), stream=vv.stream_handle(ts))
            ts.synchronize()
            assert np.array_equal(counts.cpu().numpy().view(np.uint64), want), f"device, n = {n}, offset {off}"
    # the index image of a MIP frame of the brain; no volume is needed for the call, one is needed for the frame
    _load(ctx, monkeypatch, "aniso")
    _, idx = ctx.render_mip(61, 47, vv.Camera.orbit(3.0, 1.0, 0.6), return_index=True)
    got = ctx.histogram_indices(idx)
    assert np.array_equal(got, np.bincount(idx.ravel(), minlength=256).astype(np.uint64)) and got.sum() == 61 * 47 and (got[1:] > 0).any()
    with vv.Context(0) as empty:
        assert np.array_equal(empty.histogram_indices(idx), got)


@pytest.mark.gpu
def test_histogram_errors_and_state(ctx, monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h
    I3 = C.c_int * 3
    out = vv.vv_histogram()
    counts = (C.c_ulonglong * 256)()
    idx = np.arange(40, dtype=np.uint8)
    with vv.Context(0) as empty:                                    # before a load
        assert lib.vv_volume_histogram(empty.h, None, None, C.addressof(out), 0, None) == ERR_NO_VOLUME
        with pytest.raises(vv.VolvizError) as e:
            empty.histogram()
        assert e.value.code == ERR_NO_VOLUME
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    nz, ny, nx = vol.shape
    cam = vv.Camera.orbit(3.0, 1.0, 0.6)
    frame_before = ctx.render(57, 43, cam, fill=1)
    state, dbytes, ms = ctx.layout_state(), ctx.device_bytes()[:3], ctx.last_frame_ms()

    def volume(ctx_h=hnd, lo=None, hi=None, o=C.addressof(out), on_device=0):
        return lib.vv_volume_histogram(ctx_h, C.byref(I3(*lo)) if lo else None, C.byref(I3(*hi)) if hi else None, o, on_device, None)

    assert volume() == 0 and volume(lo=(0, 0, 0), hi=(nx, ny, nz)) == 0
    assert volume(ctx_h=None) == ERR_INVALID
    assert volume(o=None) == ERR_INVALID
    assert volume(lo=(0, 0, 0)) == ERR_INVALID and volume(hi=(nx, ny, nz)) == ERR_INVALID       # a one-sided box
    for lo, hi in (((-1, 0, 0), (nx, ny, nz)), ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny + 1, nz)), ((0, 0, 0), (nx, ny, nz + 1)),
                   ((3, 0, 0), (3, ny, nz)), ((0, 5, 0), (nx, 4, nz)), ((0, 0, nz), (nx, ny, nz)), ((0, 0, 0), (0, 0, 0))):
        assert volume(lo=lo, hi=hi) == ERR_INVALID, (lo, hi)
    raw = torch.full((4096,), GARBAGE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for off in (1, 2, 4, 7):                                        # a misaligned device pointer
        assert volume(o=raw.data_ptr() + off, on_device=1) == ERR_INVALID
        assert lib.vv_histogram_indices(hnd, raw.data_ptr(), 16, raw.data_ptr() + 2048 + off, 1, None) == ERR_INVALID
    assert bool((raw == GARBAGE).all()), "a refused call writes nothing"
    assert lib.vv_histogram_indices(None, idx.ctypes.data, idx.size, counts, 0, None) == ERR_INVALID
    assert lib.vv_histogram_indices(hnd, idx.ctypes.data, idx.size, None, 0, None) == ERR_INVALID
    assert lib.vv_histogram_indices(hnd, None, idx.size, counts, 0, None) == ERR_INVALID
    assert lib.vv_histogram_indices(hnd, None, 0, counts, 0, None) == 0 and not any(counts)      # n = 0: 256 zeros, no index needed
    assert lib.vv_histogram_indices(hnd, idx.ctypes.data, idx.size, counts, 0, None) == 0 and list(counts) == [1] * 40 + [0] * 216
    # the context is still usable and untouched: volume, layout copies, residency, frame time, frames
    for box in (None, ((1, 2, 3), (19, 30, 50)), ((5, 0, 0), (6, 36, 52))):
        _same(ctx.histogram(box, prefill=GARBAGE), _want("aniso", box), f"a good call after the refused ones, box {box}")
    assert ctx.layout_state() == state and ctx.device_bytes()[:3] == dbytes and ctx.last_frame_ms() == ms
    assert np.array_equal(ctx.render(57, 43, cam, fill=1), frame_before)
    assert ctx.layout_state() == state and ctx.device_bytes()[:3] == dbytes
