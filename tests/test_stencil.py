"""Neighbourhood filters (vv_stencil_volume / vv_stencil_taps) against tests/stencil_model.py, every voxel exactly.

CPU part: the library and the binding export the calls, vv_stencil_taps equals its closed forms, and the model is tied to independent statements
(the crop identity, exact binary64 convolutions, np.median, monotone look-up tables, a linear ramp's gradient).  GPU part: the kernels equal the
model on every volume, kind, radius, tap set, gscale, output type and box of the issue -- u8 as bytes, f32 as uint32 patterns (arithmetic results:
NaN on both sides) --, into a device buffer prefilled with 0xA5 at a start address that changes from call to call and whose bytes before and behind
the output must survive, and through the host path; on every layout, launch geometry and load path; and the calls leave the context alone.

The overlap refusal of rule 9 (a device `out` inside the context's volume allocation) is not tested: no public call tells where the context keeps
its volume."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import derive_model as DM
import hist_model as HM
import stencil_model as SM
import test_hist as TH
import volume_out as VO
import volviz_amd as vv
from volume_out import GARBAGE, GUARD, bits as _bits

f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2
TF = TH.TF
KINDS = (SM.SEPARABLE, SM.MEDIAN, SM.GRADMAG)
KIND_IDS = ("separable", "median", "gradmag")
VOLUMES = ("aniso", "rand_u8", "rand_f32", "special_f32", "nan_f32")
ROWS = tuple(f"{kind}:{nx}" for kind in ("row_u8", "row_f32") for nx in TH.ROW_NX)
THIN = tuple(f"thin_{t}:{s}" for t in ("u8", "f32") for s in ("1x1x1", "2x1x3", "3x9x2", "1x40x1"))
TILE_X, TILE_YS, SEGMENT = 32, (8, 16), 32                 # the kernels' tiles in (x, y) -- 32 x 8 (3x3x3), 32 x 16 (separable) -- and their shortest z segment (csrc/vv_stencil.hip)
TILES = tuple(f"tile_{t}:{TILE_X + d}x{ty + d}x{SEGMENT + d}" for t in ("u8", "f32") for ty in TILE_YS for d in (0, 1, -1))
RADII = ((0, 0, 0), (1, 1, 1), (4, 4, 4), (2, 0, 3), (0, 4, 0), (1, 2, 4))
TAPSETS = ("binomial", "box", "gauss", "asym")
ASYM = ((0.6, 0.3, -0.15, 0.05, 0.02), (1.5, -0.25, -0.125, 0.0625, 0.03), (-0.5, 0.75, 0.1, -0.2, 0.05))      # negative taps: u8 -> u8 clamps at both ends
GSCALES = (None, (0.5, 0.5, 0.5), (1.0, 0.0, 2.5))
LAYOUT_KNOBS = TH.LAYOUT_KNOBS + ("VV_DERIVE_BLOCKS", "VV_STENCIL_BLOCKS")


@functools.lru_cache(maxsize=None)
def _volume(name):
    if ":" in name and name.split(":")[0].split("_")[0] in ("thin", "tile", "geo"):
        kind, shape = name.split(":")
        nx, ny, nz = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(1000 + nx * 7 + ny * 3 + nz)
        if kind.endswith("u8"):
            v = rng.integers(0, 256, (nz, ny, nx), dtype=np.uint8)
        else:
            v = rng.normal(0.4, 0.6, (nz, ny, nx)).astype(f32)
        v.setflags(write=False)
        return v
    return TH._volume(name)


def _tap_rows(tapset, radius):
    """The three rows of taps of a named set for these radii: float32 [3, 5] (read-only: it is a cache key's value)."""
    if tapset == "asym":
        return SM.tap_rows(ASYM)
    shape, sigma = {"binomial": (SM.BINOMIAL, 0.0), "box": (SM.BOX, 0.0), "gauss": (SM.GAUSS, 1.3)}[tapset]
    return np.stack([SM.taps(shape, r, sigma) for r in radius])


@functools.lru_cache(maxsize=None)
def _whole(volname, kind, radius=(0, 0, 0), tapset="binomial", gscale=None):
    """The model's r for the whole of a named volume: computed once, shared by the boxes, the output types and the tests."""
    r = SM.result(_volume(volname), kind, None, radius, _tap_rows(tapset, radius), gscale)
    r.setflags(write=False)
    return r


def _want(vol, r_whole, kind, box, out_type):
    """The output volume of a box: rule 6 on the crop of the whole volume's r (that the crop is the box's own result is the model's
    test_model_crop_identity and the kernels' test_stencil_box_is_the_crop_of_the_whole)."""
    return SM.finish(HM.crop(r_whole, box), vol.dtype, out_type, kind)


def _arith(kind, radius):
    """Whether a call's result went through arithmetic (NaN on both sides is then equal whatever its pattern)."""
    return kind == SM.GRADMAG or (kind == SM.SEPARABLE and any(radius))


def _check(got, want, what, nan_free_for_all):
    VO.report(got, want, SM.same(got, want, nan_free_for_all), what)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_stencil_calls():
    lib = vv.load_library()
    for name in ("vv_stencil_volume", "vv_stencil_taps"):
        assert name in vv.EXPORTS and hasattr(lib, name), f"{name} is not exported"
    for name in ("stencil", "stencil_device", "smooth", "median", "gradient_magnitude"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert callable(getattr(vv, "stencil_taps", None))
    assert (vv.STENCIL_SEPARABLE, vv.STENCIL_MEDIAN, vv.STENCIL_GRADMAG) == (0, 1, 2) == KINDS
    assert (vv.TAPS_BOX, vv.TAPS_BINOMIAL, vv.TAPS_GAUSS) == (0, 1, 2) == (SM.BOX, SM.BINOMIAL, SM.GAUSS)
    s = vv.vv_stencil
    assert C.sizeof(s) == 116
    assert (s.box_lo.offset, s.box_hi.offset, s.kind.offset, s.out_type.offset, s.radius.offset, s.taps.offset, s.gscale.offset) == (0, 12, 24, 28, 32, 44, 104)


def test_stencil_taps_closed_forms_and_errors():
    assert callable(getattr(vv, "stencil_taps", None)), "vv.stencil_taps is missing"
    for R in range(5):
        box, binom = vv.stencil_taps(vv.TAPS_BOX, R), vv.stencil_taps(vv.TAPS_BINOMIAL, R)
        assert box.dtype == np.float32 and box.shape == (5,)
        for k in range(5):
            assert _bits(box[k]) == _bits(f32(1) / f32(2 * R + 1) if k <= R else 0.0), (R, k)
            assert float(binom[k]) == (math.comb(2 * R, R + k) / 4.0 ** R if k <= R else 0.0), (R, k)        # an exact dyadic
        assert float(binom[0]) + 2 * float(binom[1:].sum()) == 1.0
        assert np.array_equal(_bits(box), _bits(SM.taps(SM.BOX, R))) and np.array_equal(_bits(binom), _bits(SM.taps(SM.BINOMIAL, R)))
        for sigma in (0.5, 1.0, 2.5):
            got = vv.stencil_taps(vv.TAPS_GAUSS, R, sigma)
            w = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(R + 1)]                    # binary64
            total = w[0]
            for k in range(1, R + 1):
                total += 2.0 * w[k]
            want = np.zeros(5, f32)
            want[:R + 1] = [f32(v / total) for v in w]                                                # one rounding
            assert np.array_equal(_bits(got), _bits(want)), (R, sigma, got, want)
            assert np.array_equal(_bits(got), _bits(SM.taps(SM.GAUSS, R, sigma)))
            assert abs(float(got[0]) + 2 * float(got[1:].sum()) - 1.0) < 1e-6 and np.all(np.diff(got[:R + 1]) < 0)
        assert np.array_equal(_bits(vv.stencil_taps(vv.TAPS_BOX, R, float("nan"))), _bits(box))       # the other shapes ignore sigma
    lib = vv.load_library()
    t = (C.c_float * 5)(*[7.0] * 5)
    for shape, radius, sigma in ((-1, 1, 1.0), (3, 1, 1.0), (0, -1, 1.0), (1, 5, 1.0), (2, 2, 0.0), (2, 2, -1.0), (2, 2, float("nan")), (2, 2, float("inf"))):
        assert lib.vv_stencil_taps(shape, radius, sigma, C.byref(t)) == ERR_INVALID, (shape, radius, sigma)
        with pytest.raises(vv.VolvizError):
            vv.stencil_taps(shape, radius, sigma)
    assert list(t) == [7.0] * 5, "a refused call writes nothing"
    assert lib.vv_stencil_taps(0, 1, 0.0, None) == ERR_INVALID


@pytest.mark.parametrize("volname", ["aniso", "rand_u8", "rand_f32"])
def test_model_crop_identity(volname):
    """Consequence (a) in the model: the result computed for a box (its own gathers, clipped to the volume) is the crop of the whole volume's."""
    assert hasattr(vv.load_library(), "vv_stencil_volume"), "vv_stencil_volume is not exported"
    vol = _volume(volname)
    boxes = TH._boxes(vol.shape, 5)
    cases = [(SM.MEDIAN, {}), (SM.GRADMAG, {}), (SM.GRADMAG, dict(gscale=(1.0, 0.0, 2.5))),
             (SM.SEPARABLE, dict(radius=(0, 0, 0))), (SM.SEPARABLE, dict(radius=(4, 4, 4), taps=_tap_rows("gauss", (4, 4, 4)))),
             (SM.SEPARABLE, dict(radius=(1, 2, 4), taps=SM.tap_rows(ASYM))), (SM.SEPARABLE, dict(radius=(2, 0, 3), taps=_tap_rows("box", (2, 0, 3))))]
    for kind, kw in cases:
        whole = SM.result(vol, kind, None, **kw)
        assert whole.shape == vol.shape
        for box in boxes[1:]:
            got = SM.result(vol, kind, box, **kw)
            assert len(SM.same(got, HM.crop(whole, box))) == 0, (volname, kind, kw, box)


def _pad(a, r):
    rx, ry, rz = r
    return np.pad(a, ((rz, rz), (ry, ry), (rx, rx)), mode="edge")


def _conv64(vol, radius, rows):
    """The convolution of the edge-padded volume in binary64, as one sum over the (2 R_x + 1)(2 R_y + 1)(2 R_z + 1) offsets."""
    rx, ry, rz = radius
    nz, ny, nx = vol.shape
    p = _pad(vol.astype(np.float64), radius)
    full = lambda row, R: [float(row[abs(k)]) for k in range(-R, R + 1)]
    tx, ty, tz = full(rows[0], rx), full(rows[1], ry), full(rows[2], rz)
    out = np.zeros(vol.shape, np.float64)
    for dz in range(2 * rz + 1):
        for dy in range(2 * ry + 1):
            for dx in range(2 * rx + 1):
                out += tz[dz] * ty[dy] * tx[dx] * p[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return out


def test_model_smoothing_is_the_exact_convolution_where_binary32_is_exact():
    """Binomial taps with R <= 2 on bytes: every intermediate is a whole number of 1 / 4096ths below 2^8, exact in binary32, so the three passes in
    binary32 are the binary64 convolution of the edge-padded volume.  The same for f32 voxels k / 256, k < 4096, with R = 1."""
    assert callable(getattr(vv.Context, "smooth", None)), "Context.smooth is missing"
    vol8 = _volume("rand_u8")
    for radius in ((1, 1, 1), (2, 2, 2), (2, 0, 1), (0, 1, 2)):
        rows = _tap_rows("binomial", radius)
        got = SM.separable(vol8, None, radius, rows)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), _conv64(vol8, radius, rows)), radius
    volf = (np.random.default_rng(61).integers(0, 4096, (11, 9, 13)).astype(f32) / f32(256)).astype(f32)
    rows = _tap_rows("binomial", (1, 1, 1))
    got = SM.separable(volf, None, (1, 1, 1), rows)
    assert np.array_equal(got.astype(np.float64), _conv64(volf, (1, 1, 1), rows))
    # the u8 -> u8 output stage on exact values is the rounding half up of the convolution
    want = np.floor(_conv64(vol8, (1, 1, 1), rows) + 0.5).astype(np.uint8)
    assert np.array_equal(SM.stencil(vol8, SM.SEPARABLE, None, SM.U8, (1, 1, 1), rows), want)


def test_model_median_properties():
    assert callable(getattr(vv.Context, "median", None)), "Context.median is missing"
    const = np.full((4, 5, 6), 37, np.uint8)
    assert np.array_equal(SM.median(const), const)
    cf = np.full((3, 2, 4), -0.0, f32)
    assert np.array_equal(SM.median(cf).view(np.uint32), cf.view(np.uint32))
    for volname in ("rand_u8", "aniso", "rand_f32", "special_f32"):
        vol = _volume(volname)
        m = SM.median(vol)
        assert m.dtype == vol.dtype and m.shape == vol.shape
        as_int = (lambda a: a) if vol.dtype == np.uint8 else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        nb = SM._neighbourhood(as_int(vol), SM._box(vol, None))
        assert (nb == as_int(m)[None]).any(axis=0).all(), f"{volname}: the median is not a voxel of its neighbourhood"
    # the median commutes with a strictly increasing 256-entry table: order is all it looks at
    vol = _volume("rand_u8")
    lut = np.sort(np.random.default_rng(4).choice(1 << 16, 256, replace=False))                 # 256 distinct values below 2^16, increasing
    assert np.all(np.diff(lut) > 0)
    nb = SM._neighbourhood(vol, SM._box(vol, None))
    assert np.array_equal(np.sort(lut[nb], axis=0)[13], lut[SM.median(vol)])
    low = np.sort(np.random.default_rng(6).choice(256, 128, replace=False)).astype(np.uint8)    # ... and one that stays in bytes, on 0..127
    half = (vol >> 1).astype(np.uint8)
    assert np.array_equal(SM.median(low[half]), low[SM.median(half)])
    volf = _volume("rand_f32")
    nbf = SM._neighbourhood(volf, SM._box(volf, None))
    assert not np.isnan(volf).any() and np.array_equal(SM.median(volf), np.median(nbf, axis=0).astype(f32))
    # NaNs take part by their patterns: above +Inf with a positive sign, below -Inf with a negative one; the result is a copy
    for patterns, want in (((0x7F800000, 0x7FC00001, 0x7FC00002), 0x7FC00001), ((0xFF800000, 0xFFC00001, 0xFFC00002), 0xFFC00001),
                           ((0x7FC00000, 0x00000000, 0x80000000), 0x00000000), ((0xFFC00000, 0x00000001, 0x80000001), 0x80000001)):
        col = np.array(patterns, np.uint32).view(f32).reshape(3, 1, 1)
        assert int(SM.median(col).view(np.uint32)[1, 0, 0]) == want, [hex(v) for v in patterns]


def test_model_gradient_of_a_ramp():
    assert callable(getattr(vv.Context, "gradient_magnitude", None)), "Context.gradient_magnitude is missing"
    a, b, c = 0.5, 0.25, 2.0                                    # dyadic slopes: every voxel and every difference is exact
    z, y, x = np.meshgrid(np.arange(7), np.arange(6), np.arange(9), indexing="ij")
    vol = (a * x + b * y + c * z).astype(f32)
    g = SM.gradmag(vol)
    assert g.dtype == np.float32
    inner = np.sqrt(f32(4 * (a * a + b * b + c * c)))
    assert np.all(g[1:-1, 1:-1, 1:-1] == inner)
    assert np.all(g[1:-1, 1:-1, 0] == np.sqrt(f32(a * a + 4 * b * b + 4 * c * c)))                # a face: the one-sided difference, unscaled
    assert np.all(g[0, 1:-1, 1:-1] == np.sqrt(f32(4 * a * a + 4 * b * b + c * c)))
    assert g[0, 0, 0] == np.sqrt(f32(a * a + b * b + c * c)) == g[-1, -1, -1]
    gs = SM.gradmag(vol, None, (1.0, 0.0, 2.5))
    assert np.all(gs[1:-1, 1:-1, 1:-1] == np.sqrt(f32(4 * a * a + 25 * c * c)))
    assert np.array_equal(SM.gradmag(vol, None, (0.0, 0.0, 0.0)), g)                             # all three 0 = (1, 1, 1)
    box = ((1, 0, 2), (8, 5, 7))
    assert np.array_equal(SM.gradmag(vol, box), HM.crop(g, box))


@pytest.mark.parametrize("volname", ["aniso", "rand_f32", "special_f32", "nan_f32"])
def test_model_radius_zero_is_the_derive_model_at_factor_one(volname):
    """Consequence (b) in the models."""
    assert hasattr(vv.load_library(), "vv_stencil_volume"), "vv_stencil_volume is not exported"
    vol = _volume(volname)
    for box in TH._boxes(vol.shape, 6)[:8]:
        for out_type in (SM.U8, SM.F32):
            got, want = SM.stencil(vol, SM.SEPARABLE, box, out_type), DM.derive(vol, box, 1, DM.MEAN, out_type)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (volname, box, out_type)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _clear_env(monkeypatch):
    VO.clear_env(monkeypatch, LAYOUT_KNOBS)


def _load(ctx, monkeypatch, volname):
    VO.load(ctx, monkeypatch, LAYOUT_KNOBS, _volume(volname), TF)


def _box_shape(vol, box):
    return HM.crop(vol, box).shape


def _run_case(ctx, dev, vol, r_whole, kind, boxes, host_boxes, what, **kw):
    """One (kind, parameters) on these boxes and both output types: the device path with guards; the host path on `host_boxes`."""
    nan_ok = _arith(kind, kw.get("radius", (0, 0, 0)))
    for box in boxes:
        for out_type in (SM.U8, SM.F32):
            want = _want(vol, r_whole, kind, box, out_type)
            dtype = np.float32 if out_type == SM.F32 else np.uint8
            tag = f"{what} kind {kind} box {box} out {out_type} {({k: v for k, v in kw.items() if k != 'taps'})}"
            got = dev.run(lambda ptr, capacity: ctx.stencil_device(ptr, capacity, kind, box=box, out_type=out_type, **kw), want.shape, dtype, tag)    # no stream: complete on return
            _check(got, want, tag + " (device)", nan_ok)
            if box in host_boxes:
                _check(ctx.stencil(kind, box, out_type, prefill=GARBAGE, **kw), want, tag + " (host)", nan_ok)


def _sep_cases():
    """Every (radius, tap set) of the issue: radius (0, 0, 0) once (no tap is looked at), the others with all four sets."""
    out = [((0, 0, 0), "binomial")]
    for radius in RADII[1:]:
        out += [(radius, t) for t in TAPSETS]
    return out


def _sweep(ctx, volname, kind):
    vol = _volume(volname)
    boxes = TH._boxes(vol.shape, 71)
    dev = VO.DeviceOut(vol.size * 4)
    host_boxes = (None, boxes[-1])
    if kind == SM.SEPARABLE:
        for radius, tapset in _sep_cases():
            _run_case(ctx, dev, vol, _whole(volname, kind, radius, tapset), kind, boxes, host_boxes, f"{volname} taps {tapset}",
                      radius=radius, taps=_tap_rows(tapset, radius))
    elif kind == SM.MEDIAN:
        _run_case(ctx, dev, vol, _whole(volname, kind), kind, boxes, host_boxes, volname)
    else:
        for gscale in GSCALES:
            _run_case(ctx, dev, vol, _whole(volname, kind, gscale=gscale), kind, boxes, host_boxes, volname, gscale=gscale)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("volname", VOLUMES + ROWS + THIN + TILES)
def test_stencil_matches_model(ctx, volname, kind, monkeypatch):
    """Every kind on every volume: the brain, random, special-value and all-NaN volumes; rows of 1 ... 257 voxels; volumes thinner than the
    stencil (with R = 4 both clamps hit in one neighbourhood); one tile, one voxel more and one less on every axis."""
    _load(ctx, monkeypatch, volname)
    _sweep(ctx, volname, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("volname", ["aniso", "rand_f32"])
def test_stencil_box_is_the_crop_of_the_whole(ctx, volname, monkeypatch):
    """Consequence (a) through two calls, bit for bit (no model, no NaN rule)."""
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    cases = [(SM.MEDIAN, {}), (SM.GRADMAG, dict(gscale=(1.0, 0.0, 2.5))), (SM.SEPARABLE, dict(radius=(4, 4, 4), taps=_tap_rows("gauss", (4, 4, 4)))),
             (SM.SEPARABLE, dict(radius=(1, 2, 4), taps=_tap_rows("asym", (1, 2, 4))))]
    for kind, kw in cases:
        for out_type in (SM.U8, SM.F32):
            whole = ctx.stencil(kind, None, out_type, prefill=GARBAGE, **kw)
            assert whole.shape == vol.shape
            for box in TH._boxes(vol.shape, 72)[1:]:
                got = ctx.stencil(kind, box, out_type, prefill=0, **kw)
                assert got.tobytes() == np.ascontiguousarray(HM.crop(whole, box)).tobytes(), (volname, kind, out_type, box)


@pytest.mark.gpu
@pytest.mark.parametrize("volname", ["aniso", "rand_f32"])
def test_stencil_radius_zero_is_derive_at_factor_one(ctx, volname, monkeypatch):
    """Consequence (b): byte equality with vv_derive_volume for all four type pairs (two volumes x two output types)."""
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    for box in TH._boxes(vol.shape, 73):
        for out_type in (SM.U8, SM.F32):
            got = ctx.stencil(SM.SEPARABLE, box, out_type, prefill=GARBAGE)
            want = ctx.derive(box, 1, DM.MEAN, out_type, prefill=0)
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (volname, box, out_type)
    assert ctx.stencil(SM.SEPARABLE).tobytes() == vol.tobytes()


def _all_kind_cases():
    return [(SM.MEDIAN, {}), (SM.GRADMAG, {}), (SM.GRADMAG, dict(gscale=(1.0, 0.0, 2.5))), (SM.SEPARABLE, dict(radius=(0, 0, 0))),
            (SM.SEPARABLE, dict(radius=(1, 1, 1), taps=_tap_rows("binomial", (1, 1, 1)))), (SM.SEPARABLE, dict(radius=(4, 4, 4), taps=_tap_rows("gauss", (4, 4, 4)))),
            (SM.SEPARABLE, dict(radius=(2, 0, 3), taps=_tap_rows("asym", (2, 0, 3)))), (SM.SEPARABLE, dict(radius=(0, 4, 0), taps=_tap_rows("box", (0, 4, 0))))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nx", [("u8", 64), ("f32", 16)])
@pytest.mark.parametrize("knobs", [{"VV_PITCH_FORCE": "1"}, {"VV_PITCH_FORCE": "1", "VV_PITCH_ROWS": "1"}, {"VV_PITCH_FORCE": "1", "VV_FORCE_BIG": "1"}, {"VV_FORCE_BIG": "1"}],
                         ids=["pitch", "pitch_rows", "pitch_big", "big"])
def test_stencil_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume (32 bytes of zeros behind every row, with and without an extra row of zeros per slice) and the 64-bit addressing
    build.  The padding holds zeros and the volume holds none: padding read as data shows as a median of 0 or as a gradient at a face."""
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
        if "VV_PITCH_FORCE" in knobs:
            row = nx * vol.itemsize + 32
            rows = ny + 1 if "VV_PITCH_ROWS" in knobs else ny
            assert c.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096             # the volume is re-pitched
        dev = VO.DeviceOut(vol.size * 4)
        boxes = TH._boxes(vol.shape, 43)
        for kd, kw in _all_kind_cases():
            _run_case(c, dev, vol, SM.result(vol, kd, None, **kw), kd, boxes, (None,), f"layout {knobs}", **kw)
        assert c.median().min() > 0, "padding was read as data"
        flat = np.full_like(vol, vol[0, 0, 0])
        c.load_volume(flat, TF)
        assert not c.gradient_magnitude(out_type=vv.VOXEL_F32).any(), "padding was read as data"      # a constant volume has no gradient, at no face


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["geo_u8", "geo_f32"])
def test_stencil_launch_geometry(ctx, kind, monkeypatch):
    """VV_STENCIL_BLOCKS = 1, 3 and unset on a 96 x 80 x 72 volume (3 x 10 or 3 x 5 tiles, three z segments): one block takes every item in turn,
    three blocks take a third each, one block per item; the same bytes, and the same bytes from a second run (consequence (e))."""
    volname = f"{kind}:96x80x72"
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    cases = [(k, kw, box) for (k, kw), box in zip(_all_kind_cases(), [None, ((3, 2, 1), (91, 77, 70)), None, ((16, 0, 5), (80, 80, 9)), None, None,
                                                                     ((31, 7, 31), (65, 17, 66)), ((0, 0, 0), (96, 80, 72))])]
    own = SM.U8 if vol.dtype == np.uint8 else SM.F32
    wants = [SM.stencil(vol, k, box, own, **kw) for k, kw, box in cases]
    other = [SM.stencil(vol, k, box, 1 - own, **kw) for k, kw, box in cases[:3]]
    try:
        for blocks in ("1", "3", None):
            if blocks is None:
                monkeypatch.delenv("VV_STENCIL_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("VV_STENCIL_BLOCKS", blocks)
            ctx.reread_env()
            for i, ((k, kw, box), want) in enumerate(zip(cases, wants)):
                got = ctx.stencil(k, box, own, prefill=GARBAGE, **kw)
                _check(got, want, f"VV_STENCIL_BLOCKS={blocks} kind {k} box {box}", _arith(k, kw.get("radius", (0, 0, 0))))
                if i < 3:
                    _check(ctx.stencil(k, box, 1 - own, prefill=GARBAGE, **kw), other[i], f"VV_STENCIL_BLOCKS={blocks} kind {k} box {box} other type", True)
                if blocks is None:
                    assert ctx.stencil(k, box, own, prefill=0, **kw).tobytes() == got.tobytes(), "a second run differs"
    finally:
        monkeypatch.delenv("VV_STENCIL_BLOCKS", raising=False)
        ctx.reread_env()


@pytest.mark.gpu
def test_stencil_load_paths(ctx, monkeypatch):
    """test_histogram_load_paths' three ways into HBM, the streamed promotion included."""
    import torch
    _clear_env(monkeypatch)
    dev = torch.device("cuda", 0)
    boxes = (None, ((2, 1, 3), (11, 9, 10)))

    def check(vol, what):
        out = VO.DeviceOut(vol.size * 4)
        for kd, kw in _all_kind_cases():
            _run_case(ctx, out, vol, SM.result(vol, kd, None, **kw), kd, boxes, (), what, **kw)

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
    ctx.load_volume_streamed([(0, vol8)], vv.VOXEL_U8, nx, ny, nz, TF)
    check(vol8, "streamed upload, u8")
    assert ctx.median(out_type=vv.VOXEL_F32).tobytes() == SM.median(promoted).tobytes()      # the median commutes with the promotion, which is increasing


@pytest.mark.gpu
def test_stencil_conveniences(ctx, monkeypatch):
    """smooth / median / gradient_magnitude are stencil() with the taps of vv_stencil_taps."""
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    box = ((1, 2, 3), (19, 30, 50))
    for radius, shape, sigma in ((1, vv.TAPS_BINOMIAL, 0.0), ((2, 0, 3), vv.TAPS_BOX, 0.0), (4, vv.TAPS_GAUSS, 1.3)):
        r = SM.radii(radius)
        rows = np.stack([SM.taps(shape, v, sigma) for v in r])
        for out_type in (None, vv.VOXEL_F32):
            got = ctx.smooth(radius, shape, sigma, box, out_type)
            _check(got, SM.stencil(vol, SM.SEPARABLE, box, out_type, r, rows), f"smooth {radius} {shape}", True)
    assert np.array_equal(ctx.smooth(), SM.stencil(vol, SM.SEPARABLE, None, None, (1, 1, 1), _tap_rows("binomial", (1, 1, 1))))
    assert np.array_equal(ctx.median(box), SM.stencil(vol, SM.MEDIAN, box))
    assert np.array_equal(ctx.gradient_magnitude((0.5, 0.5, 0.5), box, vv.VOXEL_F32), SM.stencil(vol, SM.GRADMAG, box, SM.F32, gscale=(0.5, 0.5, 0.5)))
    assert np.array_equal(ctx.gradient_magnitude(), SM.stencil(vol, SM.GRADMAG))


@pytest.mark.gpu
def test_stencil_round_trip_into_a_second_context(ctx, monkeypatch):
    """The smoothed volume written into a torch buffer on a second stream (enqueue only), loaded into a second context from there: its histogram
    and its MIP frame are those of the model's volume loaded from the host."""
    import torch
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    rows = _tap_rows("binomial", (1, 1, 1))
    want_vol = SM.stencil(vol, SM.SEPARABLE, None, SM.U8, (1, 1, 1), rows)
    nz, ny, nx = want_vol.shape
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    buf = torch.full((want_vol.size + GUARD,), GARBAGE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cam = vv.Camera.orbit(3.0, 1.0, 0.6)
    with vv.Context(0) as second, vv.Context(0) as third:
        with torch.cuda.stream(ts):
            m = ctx.stencil_device(buf.data_ptr(), want_vol.size, vv.STENCIL_SEPARABLE, radius=(1, 1, 1), taps=rows, stream=vv.stream_handle(ts))
            assert m == (nx, ny, nz)
            second.load_volume_device(buf.data_ptr(), vv.VOXEL_U8, nx, ny, nz, TF, stream=vv.stream_handle(ts))
        ts.synchronize()
        raw = buf.cpu().numpy()
        assert np.array_equal(raw[:want_vol.size].reshape(nz, ny, nx), want_vol) and (raw[want_vol.size:] == GARBAGE).all()
        third.load_volume(want_vol, TF)
        TH._same(second.histogram(prefill=GARBAGE), third.histogram(prefill=0), "histogram of the smoothed volume")
        TH._same(second.histogram(prefill=GARBAGE), HM.histogram(want_vol), "histogram of the smoothed volume against the model")
        got = second.render_mip(61, 47, cam, fill=1, return_index=True)
        want = third.render_mip(61, 47, cam, fill=1, return_index=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[1] > 0).any()


@pytest.mark.gpu
def test_stencil_errors_and_state(ctx, monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h
    with vv.Context(0) as empty:                                    # before a load
        d = vv.vv_stencil()
        out = np.full(64, GARBAGE, np.uint8)
        assert lib.vv_stencil_volume(empty.h, C.byref(d), out.ctypes.data, out.nbytes, 0, None) == ERR_NO_VOLUME and (out == GARBAGE).all()
        d.kind = 7                                                  # no volume comes before a bad descriptor
        assert lib.vv_stencil_volume(empty.h, C.byref(d), out.ctypes.data, out.nbytes, 0, None) == ERR_NO_VOLUME
        assert lib.vv_stencil_volume(empty.h, None, out.ctypes.data, out.nbytes, 0, None) == ERR_INVALID      # ... and behind the NULL checks
        for call in (empty.median, empty.smooth, empty.gradient_magnitude):
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

    def make(lo=(0, 0, 0), hi=(0, 0, 0), kind=0, out_type=vv.VOXEL_U8, radius=(0, 0, 0), taps=None, gscale=(0.0, 0.0, 0.0)):
        d = vv.vv_stencil()
        d.box_lo[:], d.box_hi[:], d.radius[:], d.gscale[:] = lo, hi, radius, gscale
        d.kind, d.out_type = kind, out_type
        for a in range(3):
            for k in range(5):
                d.taps[a][k] = 0.25 if taps is None else taps[a][k]
        return d

    def both(d):
        """The status of a host-out and of a device-out call (ample capacity) for one descriptor: they must agree."""
        rc = [lib.vv_stencil_volume(hnd, C.byref(d), host.ctypes.data, host.nbytes, 0, None), lib.vv_stencil_volume(hnd, C.byref(d), raw.data_ptr(), raw.numel(), 1, None)]
        assert rc[0] == rc[1], rc
        return rc[0]

    good = make()
    assert lib.vv_stencil_volume(None, C.byref(good), host.ctypes.data, host.nbytes, 0, None) == ERR_INVALID
    assert lib.vv_stencil_volume(hnd, None, host.ctypes.data, host.nbytes, 0, None) == ERR_INVALID
    assert lib.vv_stencil_volume(hnd, C.byref(good), None, host.nbytes, 0, None) == ERR_INVALID
    # the box
    for lo, hi in (((-1, 0, 0), (nx, ny, nz)), ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny + 1, nz)), ((0, 0, 0), (nx, ny, nz + 1)),
                   ((3, 0, 0), (3, ny, nz)), ((0, 5, 0), (nx, 4, nz)), ((0, 0, nz), (nx, ny, nz)), ((0, 0, 0), (nx, 0, 0)), ((1, 0, 0), (0, 0, 0))):
        for kind in KINDS:
            assert both(make(lo=lo, hi=hi, kind=kind)) == ERR_INVALID, (lo, hi)
    # kind, output type
    for kind in (-1, 3):
        assert both(make(kind=kind)) == ERR_INVALID
    for out_type in (-1, 2):
        assert both(make(out_type=out_type)) == ERR_INVALID
    # SEPARABLE: radii, taps up to the radius
    for radius in ((5, 0, 0), (0, -1, 0), (1, 1, 100)):
        assert both(make(radius=radius)) == ERR_INVALID, radius
    for bad in (np.nan, np.inf, -np.inf):
        for a, k in ((0, 0), (1, 2), (2, 1)):
            t = [[0.25] * 5 for _ in range(3)]
            t[a][k] = bad
            assert both(make(radius=(2, 2, 2), taps=t)) == ERR_INVALID, (bad, a, k)
    # GRADMAG: gscale
    for gscale in ((np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (0.0, 0.0, -np.inf)):
        assert both(make(kind=vv.STENCIL_GRADMAG, gscale=gscale)) == ERR_INVALID, gscale
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # what is not looked at: taps beyond the radius, taps and radii of the other kinds, gscale of the other kinds
    t = [[0.25, 0.25, 0.25, np.nan, np.inf] for _ in range(3)]
    assert both(make(radius=(2, 1, 0), taps=t)) == 0
    assert both(make(kind=vv.STENCIL_MEDIAN, radius=(9, -3, 77), taps=[[np.nan] * 5] * 3, gscale=(np.nan, np.nan, np.nan))) == 0
    assert both(make(kind=vv.STENCIL_GRADMAG, radius=(9, -3, 77), taps=[[np.nan] * 5] * 3)) == 0
    assert both(make(kind=vv.STENCIL_SEPARABLE, gscale=(np.nan, np.nan, np.nan))) == 0
    host[:] = GARBAGE
    raw.fill_(GARBAGE)
    torch.cuda.synchronize()
    # capacity, alignment
    box = dict(lo=(1, 2, 3), hi=(19, 30, 50))
    f4 = make(out_type=vv.VOXEL_F32, kind=vv.STENCIL_MEDIAN, **box)
    need = 18 * 28 * 47 * 4
    assert lib.vv_stencil_volume(hnd, C.byref(f4), host.ctypes.data, need - 1, 0, None) == ERR_INVALID
    assert lib.vv_stencil_volume(hnd, C.byref(f4), raw.data_ptr(), need - 1, 1, None) == ERR_INVALID
    assert lib.vv_stencil_volume(hnd, C.byref(good), host.ctypes.data, 0, 0, None) == ERR_INVALID
    for off in (1, 2, 3, 5):
        assert lib.vv_stencil_volume(hnd, C.byref(f4), raw.data_ptr() + off, need, 1, None) == ERR_INVALID
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # exactly the needed capacity is enough; a u8 device out may start anywhere
    assert lib.vv_stencil_volume(hnd, C.byref(f4), host.ctypes.data, need, 0, None) == 0
    _check(host[:need].view(f32).reshape(47, 28, 18), SM.stencil(vol, SM.MEDIAN, ((1, 2, 3), (19, 30, 50)), SM.F32), "exact capacity", False)
    assert (host[need:] == GARBAGE).all()
    assert lib.vv_stencil_volume(hnd, C.byref(make(kind=vv.STENCIL_MEDIAN)), raw.data_ptr() + 3, vol.size, 1, None) == 0
    got = raw.cpu().numpy()
    assert np.array_equal(got[3:3 + vol.size].reshape(vol.shape), SM.median(vol)) and (got[:3] == GARBAGE).all() and (got[3 + vol.size:] == GARBAGE).all()
    # a device-out call allocates no device memory: the device's free bytes stay what they were (every kind has run before)
    rows = _tap_rows("gauss", (4, 4, 4))
    calls = [dict(kind=vv.STENCIL_SEPARABLE, radius=(4, 4, 4), taps=rows), dict(kind=vv.STENCIL_MEDIAN), dict(kind=vv.STENCIL_GRADMAG)]
    for kw in calls:
        ctx.stencil_device(raw.data_ptr(), raw.numel(), **kw)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(dev)[0]
    for kw in calls:
        for out_type in (vv.VOXEL_U8, vv.VOXEL_F32):
            ctx.stencil_device(raw.data_ptr(), raw.numel(), out_type=out_type, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(dev)[0] == free_before, "a device-out call changed the device's free memory"
    # the context is still usable and untouched: volume, layout copies, residency, scratch, frame time, frames
    for bx in (None, ((1, 2, 3), (19, 30, 50))):
        _check(ctx.stencil(SM.GRADMAG, bx, prefill=GARBAGE), SM.stencil(vol, SM.GRADMAG, bx), f"a good call after the refused ones, box {bx}", True)
    assert ctx.layout_state() == state and ctx.device_bytes() == dbytes and ctx.last_frame_ms() == ms
    assert np.array_equal(ctx.render(57, 43, cam, fill=1), frame_before)
    assert ctx.layout_state() == state and ctx.device_bytes() == dbytes
