"""Derived volumes (vv_derive_dims / vv_derive_volume) against tests/derive_model.py, every voxel exactly.

CPU part: the model is tied to independent statements (identity, the binary64 mean, composition of maxima, the histogram model) and the library and
the binding export the calls.  GPU part: the kernel equals the model on every volume, mode, output type, factor, box and window of the issue -- u8 as
bytes, f32 as uint32 patterns (NaN results of MEAN: NaN on both sides) --, into a device buffer prefilled with 0xA5 whose bytes before and behind the
output must survive, and through the host path; on every layout, launch geometry and load path; and the calls leave the context alone."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import derive_model as DM
import hist_model as HM
import test_hist as TH
import volume_out as VO
import volviz_amd as vv
from volume_out import GARBAGE, GUARD

f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2
TF = TH.TF
MODES = (DM.MEAN, DM.MAX, DM.MIN)
MODE_IDS = ("mean", "max", "min")
FACTORS = ((1, 1, 1), (2, 2, 2), (3, 1, 2), (4, 2, 1), (1, 8, 1), (8, 8, 8), (7, 5, 3))
VOLUMES = ("aniso", "rand_u8", "rand_f32", "special_f32", "nan_f32")
ROWS = tuple(f"{kind}:{nx}" for kind in ("row_u8", "row_f32") for nx in TH.ROW_NX)
LAYOUT_KNOBS = TH.LAYOUT_KNOBS + ("VV_DERIVE_BLOCKS",)


def _volume(name):
    return TH._volume(name)


def _boxes(shape, seed):
    """test_hist's: whole; one voxel; one row; one slice; x starting at 1, 5, 15 and 17; a dozen seeded random boxes"""
    return TH._boxes(shape, seed)


def _windows(vol, hist_range):
    """None; one inside the data's range; one far outside it; the histogram's vmin / vmax (storage units)"""
    if vol.dtype == np.uint8:
        return (None, (50.5, 200.25), (1000.0, 5000.0), hist_range)
    return (None, (-0.25, 0.625), (1.0e6, 3.0e6), hist_range)


@functools.lru_cache(maxsize=None)
def _reduced(volname, box, factor, mode):
    """Stage 1 of the model for one (volume, box, factor, mode): computed once, shared by the output types and windows."""
    r = DM.reduce(_volume(volname), box, factor, mode)
    r.setflags(write=False)
    return r


def _check(got, want, what, mean_f32):
    VO.report(got, want, DM.same(got, want, nan_free_for_all=mean_f32), what)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_derive_calls():
    lib = vv.load_library()
    for name in ("vv_derive_dims", "vv_derive_volume"):
        assert name in vv.EXPORTS and hasattr(lib, name), f"{name} is not exported"
    for name in ("derive_dims", "derive", "derive_device"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert (vv.REDUCE_MEAN, vv.REDUCE_MAX, vv.REDUCE_MIN) == (0, 1, 2) == MODES
    assert C.sizeof(vv.vv_derive) == 56 and vv.vv_derive.factor.offset == 24 and vv.vv_derive.mode.offset == 36 and vv.vv_derive.win_lo.offset == 48


@pytest.mark.parametrize("volname", ["aniso", "rand_u8", "rand_f32", "special_f32", "nan_f32"])
def test_model_factor_one_is_the_identity(volname):
    """Property 1 in the model: factor 1, no window, the volume's type: the box, byte for byte (MEAN: whatever the voxel; MAX / MIN: NaN as 0x7FC00000,
    which is the only NaN of these volumes)."""
    assert hasattr(vv.load_library(), "vv_derive_volume"), "vv_derive_volume is not exported"
    vol = _volume(volname)
    for box in _boxes(vol.shape, 7):
        for mode in MODES:
            got = DM.derive(vol, box, 1, mode)
            assert got.dtype == vol.dtype and got.tobytes() == np.ascontiguousarray(HM.crop(vol, box)).tobytes(), (volname, box, mode)


@pytest.mark.parametrize("volname", ["rand_u8", "row_u8:65"])
def test_model_u8_mean_is_the_mean_rounded_half_up(volname):
    assert callable(getattr(vv.Context, "derive", None)), "Context.derive is missing"
    vol = _volume(volname)
    for factor in FACTORS:
        for box in _boxes(vol.shape, 8)[:10]:
            sub = HM.crop(vol, box)
            got = DM.derive(vol, box, factor, DM.MEAN)
            fx, fy, fz = factor
            for (Z, Y, X), g in np.ndenumerate(got):
                cell = sub[Z * fz:(Z + 1) * fz, Y * fy:(Y + 1) * fy, X * fx:(X + 1) * fx]
                assert cell.size >= 1 and g == int(np.floor(cell.astype(np.float64).mean() + 0.5)), (box, factor, (Z, Y, X))


def test_model_f32_mean_of_exact_sums_is_the_binary64_mean():
    """Voxels k / 256, k < 2^12: every partial sum of up to 512 of them is exact in binary32, so the ordered sum is the sum; the mean is one rounding of it."""
    assert callable(getattr(vv.Context, "derive", None)), "Context.derive is missing"
    vol = (np.random.default_rng(61).integers(0, 4096, (11, 9, 13)).astype(f32) / f32(256)).astype(f32)
    for factor in FACTORS:
        for box in _boxes(vol.shape, 9)[:10]:
            sub = HM.crop(vol, box)
            got = DM.derive(vol, box, factor, DM.MEAN)
            fx, fy, fz = factor
            for (Z, Y, X), g in np.ndenumerate(got):
                cell = sub[Z * fz:(Z + 1) * fz, Y * fy:(Y + 1) * fy, X * fx:(X + 1) * fx].astype(np.float64)
                assert g == f32(cell.sum() / cell.size), (box, factor, (Z, Y, X))


@pytest.mark.parametrize("volname", ["aniso", "rand_u8"])
def test_model_u8_max_by_two_twice_is_max_by_four(volname):
    assert callable(getattr(vv.Context, "derive", None)), "Context.derive is missing"
    vol = _volume(volname)
    nz, ny, nx = vol.shape
    box = ((1, 1, 3), (1 + (nx - 1) // 4 * 4, 1 + (ny - 1) // 4 * 4, 3 + (nz - 3) // 4 * 4))       # extents that are multiples of 4
    assert all((h - l) % 4 == 0 and h > l for l, h in zip(*box))
    for mode in (DM.MAX, DM.MIN):
        once = DM.derive(vol, box, 4, mode)
        twice = DM.derive(DM.derive(vol, box, 2, mode), None, 2, mode)
        assert np.array_equal(once, twice) and once.shape == tuple((h - l) // 4 for l, h in zip(*box))[::-1]


@pytest.mark.parametrize("volname", ["rand_f32", "special_f32", "nan_f32", "rand_u8"])
def test_model_quantised_volume_has_the_histogram_of_the_box(volname):
    """Property 2 in the model."""
    assert hasattr(vv.load_library(), "vv_derive_volume"), "vv_derive_volume is not exported"
    vol = _volume(volname)
    for box in _boxes(vol.shape, 10):
        q = DM.derive(vol, box, 1, DM.MEAN, DM.U8)
        assert q.dtype == np.uint8
        assert np.array_equal(np.bincount(q.ravel(), minlength=256).astype(np.uint64), HM.histogram(vol, box).counts), (volname, box)


def test_derive_dims_is_the_ceiling_formula():
    assert hasattr(vv.load_library(), "vv_derive_dims"), "vv_derive_dims is not exported"
    for e in range(1, 18):
        for f in range(1, 9):
            assert DM.dims((e, e, e), (f, f, f)) == (int(np.ceil(e / f)),) * 3
            r = DM.reduce(np.zeros((1, 1, e), np.uint8), None, (f, 1, 1), DM.MAX)
            assert r.shape == (1, 1, int(np.ceil(e / f)))
    assert DM.dims((17, 9, 1), DM._factor((8, 0, 3))) == (3, 9, 1)                 # a factor of 0 is read as 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _clear_env(monkeypatch):
    VO.clear_env(monkeypatch, LAYOUT_KNOBS)


def _load(ctx, monkeypatch, volname):
    VO.load(ctx, monkeypatch, LAYOUT_KNOBS, _volume(volname), TF)


def _device_run(dev, ctx, dtype, **kw):
    """vv_derive_volume into the guarded device buffer: of the extents vv_derive_dims gives, which the call must return too."""
    m = ctx.derive_dims(kw.get("box"), kw.get("factor", 1))
    return dev.run(lambda ptr, capacity: ctx.derive_device(ptr, capacity, **kw), m[::-1], dtype, kw)          # no stream: complete on return


def _sweep(ctx, volname, vol, modes, factors, boxes, windows, reduced, what, host_too=True):
    """Every (mode, factor, box, output type, window) against the model: device output with guard; the host path without a window."""
    dev = VO.DeviceOut(vol.size * 4)
    for mode, factor, box in itertools.product(modes, factors, boxes):
        r = reduced(box, factor, mode)
        mean_f32 = mode == DM.MEAN and vol.dtype == np.float32
        for out_type, window in itertools.product((DM.U8, DM.F32), windows):
            tag = f"{what} {volname} mode {mode} factor {factor} box {box} out {out_type} window {window}"
            kw = dict(box=box, factor=factor, mode=mode, out_type=out_type, window=window)
            if window is not None and not DM.window_ok(window):
                with pytest.raises(vv.VolvizError) as e:
                    ctx.derive(**kw)
                assert e.value.code == ERR_INVALID, tag
                continue
            want = DM.finish(r, out_type, window)
            dtype = np.float32 if out_type == DM.F32 else np.uint8
            _check(_device_run(dev, ctx, dtype, **kw), want, tag + " (device)", mean_f32)
            if host_too and window is None:
                _check(ctx.derive(prefill=GARBAGE, **kw), want, tag + " (host)", mean_f32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("volname", VOLUMES + ROWS)
def test_derive_matches_model(ctx, volname, mode, monkeypatch):
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    h = ctx.histogram()
    windows = _windows(vol, (float(h.vmin), float(h.vmax)))
    _sweep(ctx, volname, vol, (mode,), FACTORS, _boxes(vol.shape, 71), windows, lambda b, f, m: _reduced(volname, b, f, m), "sweep")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nx", [("u8", 64), ("f32", 16)])
@pytest.mark.parametrize("knobs", [{"VV_PITCH_FORCE": "1"}, {"VV_PITCH_FORCE": "1", "VV_PITCH_ROWS": "1"}, {"VV_PITCH_FORCE": "1", "VV_FORCE_BIG": "1"}],
                         ids=["pitch", "pitch_rows", "pitch_big"])
def test_derive_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume (32 bytes of zeros behind every row, with and without an extra row of zeros per slice, and under the 64-bit addressing
    build): the padding holds zeros and the volume holds none, so padding that was read shows as a MIN of 0 or a low mean."""
    _clear_env(monkeypatch)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ny, nz = 5, 4
    rng = np.random.default_rng(41)
    if kind == "u8":
        vol = rng.integers(1, 256, (nz, ny, nx), dtype=np.uint8)
    else:
        vol = (rng.integers(1, 256, (nz, ny, nx)).astype(f32) / f32(255)).astype(f32)
    with vv.Context(0) as c:                                    # a context created under the environment
        c.load_volume(vol, TF)
        row = nx * vol.itemsize + 32
        rows = ny + 1 if "VV_PITCH_ROWS" in knobs else ny
        assert c.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096             # the volume is re-pitched
        windows = (None, (50.5, 200.25) if kind == "u8" else (0.125, 0.75))
        _sweep(c, kind, vol, MODES, FACTORS, _boxes(vol.shape, 43), windows, lambda b, f, m: DM.reduce(vol, b, f, m), f"layout {knobs}", host_too=False)
        for factor in FACTORS:
            assert c.derive(None, factor, DM.MIN, DM.U8 if kind == "u8" else DM.F32).min() > 0, "padding was read as data"


@pytest.mark.gpu
def test_derive_load_paths(ctx, monkeypatch):
    """test_histogram_load_paths' three ways into HBM, the streamed promotion included."""
    import torch
    _clear_env(monkeypatch)
    dev = torch.device("cuda", 0)
    boxes = (None, ((2, 1, 3), (11, 9, 10)))
    factors = ((1, 1, 1), (2, 2, 2), (7, 5, 3))

    def check(vol, what):
        _sweep(ctx, what, vol, MODES, factors, boxes, (None, (0.1, 0.9) if vol.dtype == np.float32 else (20.0, 220.0)),
               lambda b, f, m: DM.reduce(vol, b, f, m), "load path", host_too=False)

    for volname in ("rand_u8", "special_f32"):
        vol = _volume(volname)
        nz, ny, nx = vol.shape
        ctx.load_volume(vol, TF)
        check(vol, f"{volname} load_volume")
        t = torch.from_numpy(vol.copy()).to(dev)
        ctx.load_volume_device(t.data_ptr(), vv.VOXEL_U8 if vol.dtype == np.uint8 else vv.VOXEL_F32, nx, ny, nz, TF)
        torch.cuda.synchronize()
        del t
        check(vol, f"{volname} load_volume_device")
    vol8 = _volume("rand_u8")
    nz, ny, nx = vol8.shape
    promoted = (vol8.astype(f32) / f32(255)).astype(f32)
    ctx.load_volume_streamed([(4, vol8[4:]), (0, vol8[:4])], vv.VOXEL_F32, nx, ny, nz, TF)
    check(promoted, "streamed upload with promotion")
    # ... and the promotion of the derive call is the upload's: u8 -> f32 of the u8 volume is the promoted volume
    ctx.load_volume_streamed([(0, vol8)], vv.VOXEL_U8, nx, ny, nz, TF)
    check(vol8, "streamed upload, u8")
    assert ctx.derive(out_type=vv.VOXEL_F32, prefill=GARBAGE).tobytes() == promoted.tobytes()


@pytest.mark.gpu
def test_derive_dims_on_the_library(ctx, monkeypatch):
    """vv_derive_dims is the ceiling formula for every factor 1..8 on extents 1..17 (and reads a factor of 0 as 1)."""
    _clear_env(monkeypatch)
    ctx.load_volume(np.ones((17, 17, 17), np.uint8), TF)
    for e in range(1, 18):
        for f in range(0, 9):
            lo = (17 - e, 0, (17 - e) // 2)
            box = (lo, (lo[0] + e, e, lo[2] + e))
            assert ctx.derive_dims(box, f) == (int(np.ceil(e / max(f, 1))),) * 3, (e, f)
            assert ctx.derive_dims(box, (f, 1, 8)) == (int(np.ceil(e / max(f, 1))), e, int(np.ceil(e / 8)))
    assert ctx.derive_dims() == (17, 17, 17) and ctx.derive(factor=(8, 3, 17 // 2), mode=DM.MAX).shape == (3, 6, 3)


@pytest.mark.gpu
def test_derive_launch_geometry(ctx, monkeypatch):
    """VV_DERIVE_BLOCKS = 1, 3 and unset on the 96 x 80 x 72 volume: many trips, a few trips and one trip of the grid-stride loop; the same bytes."""
    _load(ctx, monkeypatch, "geometry")
    vol = _volume("geometry")
    cases = [dict(box=None, factor=1, mode=DM.MEAN, out_type=DM.U8), dict(box=None, factor=2, mode=DM.MEAN, out_type=DM.F32),
             dict(box=((3, 2, 1), (91, 77, 70)), factor=(3, 1, 2), mode=DM.MAX, out_type=DM.U8),
             dict(box=((16, 0, 5), (80, 80, 9)), factor=(8, 8, 8), mode=DM.MIN, out_type=DM.F32, window=(10.0, 250.0)),
             dict(box=((0, 0, 0), (96, 80, 72)), factor=(4, 2, 1), mode=DM.MEAN, out_type=DM.U8)]
    wants = [DM.derive(vol, **kw) for kw in cases]
    try:
        for blocks in ("1", "3", None):
            if blocks is None:
                monkeypatch.delenv("VV_DERIVE_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("VV_DERIVE_BLOCKS", blocks)
            ctx.reread_env()
            for kw, want in zip(cases, wants):
                _check(ctx.derive(prefill=GARBAGE, **kw), want, f"VV_DERIVE_BLOCKS={blocks} {kw}", False)
    finally:
        monkeypatch.delenv("VV_DERIVE_BLOCKS", raising=False)
        ctx.reread_env()


@pytest.mark.gpu
def test_derive_reads_back_a_generated_volume(ctx, monkeypatch):
    """Property 1: a volume that exists only in HBM (generated there, loaded from there) comes back as the host generator writes it."""
    import torch
    _clear_env(monkeypatch)
    nx, ny, nz = 40, 36, 28
    t = torch.zeros(nx * ny * nz, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.generate_default_brain_device(t.data_ptr(), nx, ny, nz)
    ctx.load_volume_device(t.data_ptr(), vv.VOXEL_U8, nx, ny, nz, TF)
    torch.cuda.synchronize()
    del t
    want = ctx.generate_default_brain(nx, ny, nz)
    assert len(np.unique(want)) > 3
    got = ctx.derive(prefill=GARBAGE)
    assert got.dtype == np.uint8 and got.shape == (nz, ny, nx) and np.array_equal(got, want)
    box = ((3, 5, 7), (38, 30, 21))
    assert np.array_equal(ctx.derive(box, prefill=GARBAGE), HM.crop(want, box))


@pytest.mark.gpu
@pytest.mark.parametrize("volname", ["rand_f32", "special_f32"])
def test_derive_quantised_volume_has_the_source_histogram(ctx, volname, monkeypatch):
    """Property 2: f32 -> u8 at factor 1, loaded, has the histogram counts of the source box."""
    vol = _volume(volname)
    for box in (None, ((2, 1, 3), (11, 9, 10))):
        _load(ctx, monkeypatch, volname)
        src = ctx.histogram(box, prefill=GARBAGE)
        q = ctx.derive(box, 1, out_type=vv.VOXEL_U8, prefill=GARBAGE)
        assert np.array_equal(q, HM.bins(HM.crop(vol, box)))
        ctx.load_volume(q, TF)
        got = ctx.histogram(prefill=GARBAGE)
        assert np.array_equal(got.counts, src.counts) and np.array_equal(src.counts, TH._want(volname, box).counts) and got.voxels == src.voxels


@pytest.mark.gpu
def test_derive_round_trip_into_a_second_context(ctx, monkeypatch):
    """The preview: 2x MAX into a torch buffer on a second stream (enqueue only), loaded into a second context from there, rendered as a MIP frame:
    the frame of the model's volume loaded from the host."""
    import torch
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    want_vol = DM.derive(vol, None, 2, DM.MAX)
    mz, my, mx = want_vol.shape
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    buf = torch.full((want_vol.size + GUARD,), GARBAGE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cam = vv.Camera.orbit(3.0, 1.0, 0.6)
    with vv.Context(0) as second, vv.Context(0) as third:
        with torch.cuda.stream(ts):
            m = ctx.derive_device(buf.data_ptr(), want_vol.size, None, 2, DM.MAX, stream=vv.stream_handle(ts))
            assert m == (mx, my, mz) == ctx.derive_dims(None, 2)
            second.load_volume_device(buf.data_ptr(), vv.VOXEL_U8, mx, my, mz, TF, stream=vv.stream_handle(ts))
        ts.synchronize()
        raw = buf.cpu().numpy()
        assert np.array_equal(raw[:want_vol.size].reshape(mz, my, mx), want_vol) and (raw[want_vol.size:] == GARBAGE).all()
        got = second.render_mip(61, 47, cam, fill=1, return_index=True)
        third.load_volume(want_vol, TF)
        want = third.render_mip(61, 47, cam, fill=1, return_index=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[1] > 0).any()


@pytest.mark.gpu
def test_derive_errors_and_state(ctx, monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h
    I3 = C.c_int * 3
    with vv.Context(0) as empty:                                    # before a load
        d, m = vv.vv_derive(), I3()
        out = np.full(64, GARBAGE, np.uint8)
        assert lib.vv_derive_dims(empty.h, C.byref(d), C.byref(m)) == ERR_NO_VOLUME
        assert lib.vv_derive_volume(empty.h, C.byref(d), out.ctypes.data, out.nbytes, 0, None) == ERR_NO_VOLUME and (out == GARBAGE).all()
        for call in (empty.derive, empty.derive_dims):
            with pytest.raises(vv.VolvizError) as e:
                call()
            assert e.value.code == ERR_NO_VOLUME
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    nz, ny, nx = vol.shape
    cam = vv.Camera.orbit(3.0, 1.0, 0.6)
    frame_before = ctx.render(57, 43, cam, fill=1)
    state, dbytes, ms = ctx.layout_state(), ctx.device_bytes(), ctx.last_frame_ms()

    host = np.full(vol.size * 4 + GUARD, GARBAGE, np.uint8)
    raw = torch.full((vol.size * 4 + GUARD,), GARBAGE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def make(lo=(0, 0, 0), hi=(0, 0, 0), factor=(1, 1, 1), mode=0, out_type=vv.VOXEL_U8, window=0, win=(0.0, 1.0)):
        d = vv.vv_derive()
        d.box_lo[:], d.box_hi[:], d.factor[:] = lo, hi, factor
        d.mode, d.out_type, d.window, d.win_lo, d.win_hi = mode, out_type, window, win[0], win[1]
        return d

    def both(d):
        """The status of vv_derive_dims and of vv_derive_volume (host and device out, ample capacity) for one descriptor: they must agree."""
        m = I3(-7, -7, -7)
        rc = [lib.vv_derive_dims(hnd, C.byref(d), C.byref(m)), lib.vv_derive_volume(hnd, C.byref(d), host.ctypes.data, host.nbytes, 0, None),
              lib.vv_derive_volume(hnd, C.byref(d), raw.data_ptr(), raw.numel(), 1, None)]
        assert rc[0] == rc[1] == rc[2], rc
        if rc[0]:
            assert tuple(m) == (-7, -7, -7)
        return rc[0]

    good = make()
    m = I3()
    assert lib.vv_derive_dims(hnd, C.byref(good), C.byref(m)) == 0 and tuple(m) == (nx, ny, nz)
    assert lib.vv_derive_dims(None, C.byref(good), C.byref(m)) == ERR_INVALID
    assert lib.vv_derive_dims(hnd, None, C.byref(m)) == ERR_INVALID and lib.vv_derive_dims(hnd, C.byref(good), None) == ERR_INVALID
    assert lib.vv_derive_volume(None, C.byref(good), host.ctypes.data, host.nbytes, 0, None) == ERR_INVALID
    assert lib.vv_derive_volume(hnd, None, host.ctypes.data, host.nbytes, 0, None) == ERR_INVALID
    assert lib.vv_derive_volume(hnd, C.byref(good), None, host.nbytes, 0, None) == ERR_INVALID
    # the box
    for lo, hi in (((-1, 0, 0), (nx, ny, nz)), ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny + 1, nz)), ((0, 0, 0), (nx, ny, nz + 1)),
                   ((3, 0, 0), (3, ny, nz)), ((0, 5, 0), (nx, 4, nz)), ((0, 0, nz), (nx, ny, nz)), ((0, 0, 0), (nx, 0, 0)), ((1, 0, 0), (0, 0, 0))):
        assert both(make(lo=lo, hi=hi)) == ERR_INVALID, (lo, hi)
    # factor, mode, output type, window flag
    for factor in ((9, 1, 1), (1, -1, 1), (1, 1, 100)):
        assert both(make(factor=factor)) == ERR_INVALID, factor
    for mode in (-1, 3):
        assert both(make(mode=mode)) == ERR_INVALID
    for out_type in (-1, 2):
        assert both(make(out_type=out_type)) == ERR_INVALID
    for window in (-1, 2):
        assert both(make(window=window)) == ERR_INVALID
    # the window's values: not finite, empty, reversed, a difference that overflows binary32 or rounds to zero
    big = float(np.finfo(f32).max)
    for win in ((np.nan, 1.0), (0.0, np.nan), (-np.inf, 1.0), (0.0, np.inf), (1.0, 1.0), (2.0, 1.0), (-big, big), (1.0, 1.0 + 1e-9)):
        assert both(make(window=1, win=win)) == ERR_INVALID, win
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    assert both(make(window=0, win=(np.nan, np.nan))) == 0             # not looked at without a window
    host[:] = GARBAGE
    raw.fill_(GARBAGE)
    torch.cuda.synchronize()
    # capacity, alignment
    f4 = make(out_type=vv.VOXEL_F32, factor=(2, 2, 2))
    need = DM.dims((nx, ny, nz), (2, 2, 2))
    need = need[0] * need[1] * need[2] * 4
    assert lib.vv_derive_volume(hnd, C.byref(f4), host.ctypes.data, need - 1, 0, None) == ERR_INVALID
    assert lib.vv_derive_volume(hnd, C.byref(f4), raw.data_ptr(), need - 1, 1, None) == ERR_INVALID
    assert lib.vv_derive_volume(hnd, C.byref(good), host.ctypes.data, 0, 0, None) == ERR_INVALID
    for off in (1, 2, 3, 5):
        assert lib.vv_derive_volume(hnd, C.byref(f4), raw.data_ptr() + off, need, 1, None) == ERR_INVALID
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # exactly the needed capacity is enough; a u8 device out may start anywhere; 0 factors are 1
    assert lib.vv_derive_volume(hnd, C.byref(f4), host.ctypes.data, need, 0, None) == 0
    _check(host[:need].view(f32).reshape(DM.dims((nx, ny, nz), (2, 2, 2))[::-1]), DM.derive(vol, None, 2, DM.MEAN, DM.F32), "exact capacity", False)
    assert (host[need:] == GARBAGE).all()
    assert lib.vv_derive_volume(hnd, C.byref(make(factor=(0, 0, 0))), raw.data_ptr() + 3, vol.size, 1, None) == 0
    got = raw.cpu().numpy()
    assert np.array_equal(got[3:3 + vol.size].reshape(vol.shape), vol) and (got[:3] == GARBAGE).all() and (got[3 + vol.size:] == GARBAGE).all()
    # the context is still usable and untouched: volume, layout copies, residency, scratch, frame time, frames
    for box in (None, ((1, 2, 3), (19, 30, 50))):
        _check(ctx.derive(box, (3, 1, 2), DM.MAX, prefill=GARBAGE), DM.derive(vol, box, (3, 1, 2), DM.MAX), f"a good call after the refused ones, box {box}", False)
    assert ctx.layout_state() == state and ctx.device_bytes() == dbytes and ctx.last_frame_ms() == ms
    assert np.array_equal(ctx.render(57, 43, cam, fill=1), frame_before)
    assert ctx.layout_state() == state and ctx.device_bytes() == dbytes
