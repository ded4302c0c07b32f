"""Thick-slab slices (vv_slice_slab / vv_slice_advanced_slab) against tests/slab_model.py, bit for bit.

CPU part: the model's layers are the oracle's slices at the displaced planes, K = 1 is the oracle's slice, the inputs are not trivial, and the
library and the binding export the calls.  GPU part: the kernel equals the model on every input -- values as uint32 patterns, aux as int32 --
with fills of -3.0 and -7 showing the elements the kernel must leave alone."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import oracle_lib as O
import slab_model as SM
import volviz_amd as vv
import witness as Wt

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
FILL, AUX_FILL = -3.0, -7
ERR_INVALID, ERR_NO_VOLUME = -1, -2                        # include/volviz.h: vv_status
MODES = ((SM.SLAB_MAX, "max"), (SM.SLAB_MIN, "min"), (SM.SLAB_MEAN, "mean"))
FILTERS = (vv.FILTER_TEX8, vv.FILTER_EXACT)
SHAPES = ((17, 23, 7, 0.5), (33, 19, 16, 1.4), (12, 40, 5, 0.25))       # (height, width, K, thickness); the last: width > height
SCALES = ((1.0, 1.0, 0.8), (1.57, 1.0, 1.0))
# displacements that leave the volume on some pixels, in the plane and (for some thicknesses) along the slab
CANONICAL = {"sagittal": (vv.SAGITTAL, (0.15, -0.2, 0.9)), "horizontal": (vv.HORIZONTAL, (-0.1, 0.45, 0.2)), "coronal": (vv.CORONAL, (0.1, 0.2, -0.15))}
VIEWS = ("sagittal", "horizontal", "coronal", "free")
VOLUMES = ("aniso", "rand_u8", "rand_f32")
INPUTS = list(itertools.product(FILTERS, VIEWS, range(len(SHAPES)), range(len(SCALES))))


@functools.lru_cache(maxsize=None)
def _free_form():
    """T(.5) T(.05, -.1, .1) Rx(.5) Ry(.4) T(-.5)"""
    m = vv.slice_matrix(0.05, -0.1, 0.1, 0.5, 0.4, 0.0)
    assert np.array_equal(np.asarray(m, f32).reshape(4, 4), O.slice_matrix(0.05, -0.1, 0.1, 0.5, 0.4, 0.0))
    return np.asarray(m, f32).reshape(16)


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name == "aniso":
        v = np.fromfile(os.path.join(HERE, "golden", "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
    elif name == "rand_u8":
        v = np.random.default_rng(11).integers(0, 256, (11, 9, 13), dtype=np.uint8)
    elif name == "rand_f32":
        v = np.random.default_rng(12).normal(0.0, 1.0, (11, 9, 13)).astype(f32)           # signed
    else:
        assert name == "ends_f32"                              # the ends of the f32 value domain (include/volviz.h: |v| <= 2^126)
        sign = np.random.default_rng(13).choice(np.array([1.0, -1.0], f32), (4, 3, 5))        # plateaus of 3^3 voxels: runs of equal samples
        v = (np.repeat(np.repeat(np.repeat(sign, 3, 0), 3, 1), 3, 2)[:11, :9, :13] * f32(2.0 ** 126)).astype(f32)
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _layers(volname, filt, view, shape, scale):
    """The model's layers of one input, computed once and shared by every test: (values, executed), read-only."""
    h, w, K, thick = SHAPES[shape]
    vol = _volume(volname)
    if view == "free":
        out = SM.layers_advanced(vol, h, w, _free_form(), K, thick, SCALES[scale], filt)
    else:
        orient, d = CANONICAL[view]
        out = SM.layers_canonical(vol, h, w, *d, orient, K, thick, SCALES[scale], filt)
    for a in out:
        a.setflags(write=False)
    return out


def _want(volname, filt, view, shape, scale, mode):
    h, w, _, _ = SHAPES[shape]
    return SM.store(h, w, *SM.reduce(*_layers(volname, filt, view, shape, scale), mode), FILL, AUX_FILL)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _same_pair(got, want, what):
    _same(got[0], want[0], f"{what}: values")
    _same(got[1], want[1], f"{what}: aux")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_slab_calls():
    lib = vv.load_library()
    for name in ("vv_slice_slab", "vv_slice_advanced_slab"):
        assert name in vv.EXPORTS and hasattr(lib, name), f"{name} is not exported"
    for name in ("slice_slab", "slice_advanced_slab", "slice_slab_device", "slice_advanced_slab_device"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert (vv.SLAB_MAX, vv.SLAB_MIN, vv.SLAB_MEAN) == (0, 1, 2)


@pytest.mark.parametrize("volname", VOLUMES)
def test_model_layers_are_oracle_slices(volname):
    """Layer k of a canonical slab = the oracle's slice at the displacement d_a + o_k (the sum taken in binary32)."""
    vol = _volume(volname)
    for filt, view, shape, scale in INPUTS:
        if view == "free":
            continue
        h, w, K, thick = SHAPES[shape]
        orient, d = CANONICAL[view]
        vals, oks = _layers(volname, filt, view, shape, scale)
        a = SM.AXIS_OF[orient]
        for k, o in enumerate(SM.offsets(K, thick).ravel()):
            dk = list(d)
            dk[a] = float(f32(d[a]) + o)
            want = O.slice(vol, h, w, *dk, orient, SCALES[scale], filter=filt, fill=FILL)
            got = Wt._slice_store(np.full(h * w, FILL, f32), h, w, vals[k])
            _same(got, want, f"{volname} {view} filter {filt} shape {SHAPES[shape]} scale {SCALES[scale]} layer {k}")
            assert not vals[k][~oks[k]].any()


@pytest.mark.parametrize("volname", VOLUMES)
def test_model_single_sample_is_the_oracle_slice(volname):
    vol = _volume(volname)
    for filt, (h, w, _, thick), scale in itertools.product(FILTERS, SHAPES, SCALES):
        for mode, mname in MODES:
            for view, (orient, d) in CANONICAL.items():
                got, _ = SM.slab_canonical(vol, h, w, *d, orient, mode, 1, thick, scale, filt, fill=FILL)
                _same(got, O.slice(vol, h, w, *d, orient, scale, filter=filt, fill=FILL), f"{volname} {view} {mname} K = 1")
                _same(got, Wt.slice_canonical(vol, h, w, *d, orient, scale, filt=filt, fill=FILL), f"{volname} {view} {mname} K = 1, witness")
            got, _ = SM.slab_advanced(vol, h, w, _free_form(), mode, 1, thick, scale, filt, fill=FILL)
            _same(got, O.slice_advanced(vol, h, w, _free_form(), scale, filter=filt, fill=FILL), f"{volname} free-form {mname} K = 1")


def test_inputs_are_not_trivial():
    """Pixels without a sample, with some and with all of them; ties in MAX; MAX != MIN: each on every volume."""
    for volname in VOLUMES:
        none = partial = full = ties = spread = 0
        by_view = {v: [0, 0, 0] for v in VIEWS}
        for filt, view, shape, scale in INPUTS:
            vals, oks = _layers(volname, filt, view, shape, scale)
            K = SHAPES[shape][2]
            n = oks.sum(axis=0)
            cls = [int((n == 0).sum()), int(((n > 0) & (n < K)).sum()), int((n == K).sum())]
            by_view[view] = [a + b for a, b in zip(by_view[view], cls)]
            none += cls[0]; partial += cls[1]; full += cls[2]
            vmax, _ = SM.reduce(vals, oks, SM.SLAB_MAX)
            vmin, _ = SM.reduce(vals, oks, SM.SLAB_MIN)
            ties += int(((oks & (vals == vmax[None])).sum(axis=0) >= 2).sum())
            spread += int(((n > 0) & (vmax != vmin)).sum())
        print(f"{volname}: pixels with no / some / all samples {none} / {partial} / {full}, by view {by_view}, MAX ties {ties}, MAX != MIN {spread}")
        assert none > 0 and partial > 0 and full > 0
        assert all(by_view["free"]), by_view                   # the free-form view shows all three classes by itself
        assert all(sum(by_view[v][1:]) > 0 for v in VIEWS), by_view
        assert spread > 0
        assert ties > 0 or volname != "aniso"                    # (random volumes have no equal samples; the brain's plateaus do)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
TF = np.linspace(0.0, 1.0, 1024, dtype=np.float32)


def _load(ctx, monkeypatch, volname, big=False):
    monkeypatch.delenv("VV_FORCE_BIG", raising=False)
    if big:
        monkeypatch.setenv("VV_FORCE_BIG", "1")
    ctx.load_volume(_volume(volname), TF)                       # (the knobs are read at volume load)


def _gpu(ctx, view, h, w, K, thick, scale, filt, mode, **kw):
    kw = dict(mode=mode, samples=K, thickness=thick, scale=scale, filter=filt, fill=FILL, return_aux=True, aux_fill=AUX_FILL, **kw)
    if view == "free":
        return ctx.slice_advanced_slab(h, w, _free_form(), **kw)
    orient, d = CANONICAL[view]
    return ctx.slice_slab(h, w, *d, orient, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("volname,big", [("aniso", False), ("rand_u8", False), ("rand_f32", False), ("rand_u8", True), ("rand_f32", True)])
def test_slab_matches_model(volname, big, monkeypatch):
    monkeypatch.delenv("VV_FORCE_BIG", raising=False)
    if big:
        monkeypatch.setenv("VV_FORCE_BIG", "1")
    with vv.Context(0) as ctx:                                  # a context created under the environment
        ctx.load_volume(_volume(volname), TF)
        for filt, view, shape, scale in INPUTS:
            h, w, K, thick = SHAPES[shape]
            for mode, mname in MODES:
                got = _gpu(ctx, view, h, w, K, thick, SCALES[scale], filt, mode)
                _same_pair(got, _want(volname, filt, view, shape, scale, mode),
                           f"{volname} big={big} {view} {mname} filter {filt} shape {SHAPES[shape]} scale {SCALES[scale]}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 7, 8, 9, 15, 17, 33, 64, 1024])
def test_slab_loop_remainder(ctx, K, monkeypatch):
    """Every remainder of a group of up to 8 samples, and the longest loop."""
    _load(ctx, monkeypatch, "rand_f32")
    vol = _volume("rand_f32")
    h = w = 8
    orient, d = CANONICAL["horizontal"]
    for mode in (SM.SLAB_MEAN, SM.SLAB_MAX):
        got = ctx.slice_slab(h, w, *d, orient, mode=mode, samples=K, thickness=1.3, scale=SCALES[0], fill=FILL, return_aux=True, aux_fill=AUX_FILL)
        _same_pair(got, SM.slab_canonical(vol, h, w, *d, orient, mode, K, 1.3, SCALES[0]), f"canonical K = {K} mode {mode}")
        got = ctx.slice_advanced_slab(h, w, _free_form(), mode=mode, samples=K, thickness=0.9, scale=SCALES[1], filter=vv.FILTER_EXACT, fill=FILL,
                                      return_aux=True, aux_fill=AUX_FILL)
        _same_pair(got, SM.slab_advanced(vol, h, w, _free_form(), mode, K, 0.9, SCALES[1], Wt.FILTER_EXACT), f"free-form K = {K} mode {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("volname", VOLUMES)
def test_slab_single_sample_is_the_slice(ctx, volname, monkeypatch):
    _load(ctx, monkeypatch, volname)
    for filt, (h, w, _, thick), scale in itertools.product(FILTERS, SHAPES, SCALES):
        for mode, mname in MODES:
            none, one = (0, 1) if mode == SM.SLAB_MEAN else (-1, 0)
            for view, (orient, d) in CANONICAL.items():
                got, aux = _gpu(ctx, view, h, w, 1, thick, scale, filt, mode)
                _same(got, ctx.slice(h, w, *d, orient, scale=scale, filter=filt, fill=FILL), f"{volname} {view} {mname} K = 1")
                assert set(np.unique(aux)) <= {none, one, AUX_FILL}
            got, aux = _gpu(ctx, "free", h, w, 1, thick, scale, filt, mode)
            _same(got, ctx.slice_advanced(h, w, _free_form(), scale=scale, filter=filt, fill=FILL), f"{volname} free-form {mname} K = 1")
            assert set(np.unique(aux)) <= {none, one, AUX_FILL} and (aux == none).any() and (aux == one).any()
            wv, wa = SM.slab_advanced(_volume(volname), h, w, _free_form(), mode, 1, thick, scale, filt)
            _same_pair((got, aux), (wv, wa), f"{volname} free-form {mname} K = 1, model")


@pytest.mark.gpu
def test_slab_f32_range_ends(ctx, monkeypatch):
    """Voxels of +-2^126: the extrema are exact, a mean of 8 may leave binary32 and is then the IEEE sum's +-Inf; never a NaN."""
    _load(ctx, monkeypatch, "ends_f32")
    vol = _volume("ends_f32")
    h, w, K = 17, 23, 8
    seen_inf = False
    for filt in FILTERS:
        for view in VIEWS:
            for mode, mname in MODES:
                got = _gpu(ctx, view, h, w, K, 0.5, SCALES[0], filt, mode)
                if view == "free":
                    want = SM.slab_advanced(vol, h, w, _free_form(), mode, K, 0.5, SCALES[0], filt)
                else:
                    orient, d = CANONICAL[view]
                    want = SM.slab_canonical(vol, h, w, *d, orient, mode, K, 0.5, SCALES[0], filt)
                _same_pair(got, want, f"range ends {view} {mname} filter {filt}")
                assert not np.isnan(got[0]).any()
                seen_inf |= mode == SM.SLAB_MEAN and bool(np.isinf(got[0]).any())
    assert seen_inf


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(1, 1), (16, 16), (17, 1), (1, 17)])
def test_slab_sizes(ctx, h, w, monkeypatch):
    _load(ctx, monkeypatch, "rand_u8")
    vol = _volume("rand_u8")
    for mode, mname in MODES:
        for view, (orient, d) in CANONICAL.items():
            got = ctx.slice_slab(h, w, *d, orient, mode=mode, samples=6, thickness=0.7, fill=FILL, return_aux=True, aux_fill=AUX_FILL)
            _same_pair(got, SM.slab_canonical(vol, h, w, *d, orient, mode, 6, 0.7), f"{h} x {w} {view} {mname}")
        got = ctx.slice_advanced_slab(h, w, _free_form(), mode=mode, samples=6, thickness=0.7, fill=FILL, return_aux=True, aux_fill=AUX_FILL)
        _same_pair(got, SM.slab_advanced(vol, h, w, _free_form(), mode, 6, 0.7), f"{h} x {w} free-form {mname}")


@pytest.mark.gpu
def test_slab_device_path(ctx, monkeypatch):
    import torch
    _load(ctx, monkeypatch, "aniso")
    dev = torch.device("cuda", 0)
    h, w, K, thick = SHAPES[2]
    orient, d = CANONICAL["sagittal"]
    kw = dict(mode=vv.SLAB_MEAN, samples=K, thickness=thick, scale=SCALES[0])
    want_c = ctx.slice_slab(h, w, *d, orient, fill=FILL, return_aux=True, aux_fill=AUX_FILL, **kw)
    want_f = ctx.slice_advanced_slab(h, w, _free_form(), fill=FILL, return_aux=True, aux_fill=AUX_FILL, **kw)
    assert (want_c[1] == AUX_FILL).any() and (want_f[1] > 0).any()
    for ts in (torch.cuda.Stream(device=dev), torch.cuda.default_stream(dev)):
        bufs = [torch.full((h * w,), FILL, dtype=torch.float32, device=dev) for _ in range(2)]
        auxs = [torch.full((h * w,), AUX_FILL, dtype=torch.int32, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            ctx.slice_slab_device(h, w, *d, orient, bufs[0].data_ptr(), auxs[0].data_ptr(), stream=vv.stream_handle(ts), **kw)
            ctx.slice_advanced_slab_device(h, w, _free_form(), bufs[1].data_ptr(), auxs[1].data_ptr(), stream=vv.stream_handle(ts), **kw)
        ts.synchronize()
        _same_pair((bufs[0].cpu().numpy(), auxs[0].cpu().numpy()), want_c, "enqueue-only, canonical")
        _same_pair((bufs[1].cpu().numpy(), auxs[1].cpu().numpy()), want_f, "enqueue-only, free-form")
    # aux = NULL: the same values, on the device (synchronous call) and on the host
    buf = torch.full((h * w,), FILL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.slice_slab_device(h, w, *d, orient, buf.data_ptr(), 0, **kw)
    _same(buf.cpu().numpy(), want_c[0], "device, no aux")
    _same(ctx.slice_advanced_slab(h, w, _free_form(), fill=FILL, **kw), want_f[0], "host, no aux")
    # a misaligned device aux
    raw = torch.zeros(h * w * 4 + 8, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        with pytest.raises(vv.VolvizError) as e:
            ctx.slice_slab_device(h, w, *d, orient, buf.data_ptr(), raw.data_ptr() + off, **kw)
        assert e.value.code == ERR_INVALID
        with pytest.raises(vv.VolvizError) as e:
            ctx.slice_advanced_slab_device(h, w, _free_form(), buf.data_ptr(), raw.data_ptr() + off, **kw)
        assert e.value.code == ERR_INVALID
    _same(buf.cpu().numpy(), want_c[0], "a refused call writes nothing")


@pytest.mark.gpu
def test_slab_errors(ctx, monkeypatch):
    _load(ctx, monkeypatch, "rand_u8")
    vol = _volume("rand_u8")
    lib, hnd = ctx.lib, ctx.h
    h, w = 9, 7
    buf = np.full(h * w, FILL, f32)
    sc = (C.c_float * 3)(1.0, 1.0, 1.0)
    tr = (C.c_float * 16)(*[float(v) for v in _free_form()])
    good = vv.vv_slab(vv.SLAB_MAX, 4, 0.5)

    def canonical(ctx_h=hnd, b=buf.ctypes.data, hh=h, ww=w, orient=vv.SAGITTAL, scale=C.byref(sc), slab=good):
        return lib.vv_slice_slab(ctx_h, b, None, hh, ww, 0.1, 0.1, 0.4, orient, scale, vv.FILTER_TEX8, C.byref(slab) if slab is not None else None, 0, None)

    def advanced(ctx_h=hnd, b=buf.ctypes.data, hh=h, ww=w, trans=C.byref(tr), scale=C.byref(sc), slab=good):
        return lib.vv_slice_advanced_slab(ctx_h, b, None, hh, ww, trans, scale, vv.FILTER_TEX8, C.byref(slab) if slab is not None else None, 0, None)

    assert canonical() == 0 and advanced() == 0
    for call in (canonical, advanced):
        assert call(ctx_h=None) == ERR_INVALID
        assert call(b=None) == ERR_INVALID
        assert call(scale=None) == ERR_INVALID
        assert call(slab=None) == ERR_INVALID
        for mode in (-1, 3, 7):
            assert call(slab=vv.vv_slab(mode, 4, 0.5)) == ERR_INVALID
        for samples in (0, -1, 1025, 1 << 20):
            assert call(slab=vv.vv_slab(vv.SLAB_MEAN, samples, 0.5)) == ERR_INVALID
        for thick in (-0.5, -1e-30, float("inf"), float("-inf"), float("nan")):
            assert call(slab=vv.vv_slab(vv.SLAB_MIN, 4, thick)) == ERR_INVALID
        for hh, ww in ((0, 5), (5, 0), (65535 * 16 + 1, 1), (1, 65535 * 16 + 1)):          # the sizes vv_slice rejects
            assert call(hh=hh, ww=ww) == ERR_INVALID
            assert lib.vv_slice(hnd, buf.ctypes.data, hh, ww, 0.0, 0.0, 0.0, vv.SAGITTAL, C.byref(sc), 0, vv.FILTER_TEX8, 0, None) == ERR_INVALID
        assert call(slab=vv.vv_slab(vv.SLAB_MAX, 1024, 0.0)) == 0                        # the ends of the valid ranges
    assert advanced(trans=None) == ERR_INVALID
    for orient in (vv.FREE_FORM, 3, -1, 17):
        assert canonical(orient=orient) == ERR_INVALID
    assert canonical(slab=vv.vv_slab(vv.SLAB_MAX, 1024, 0.0)) == 0                       # 1024 samples of one plane
    _same(buf, ctx.slice(h, w, 0.1, 0.1, 0.4, vv.SAGITTAL, fill=FILL), "thickness 0")
    with vv.Context(0) as empty:
        for name in ("slice_slab", "slice_advanced_slab"):
            with pytest.raises(vv.VolvizError) as e:
                if name == "slice_slab":
                    empty.slice_slab(h, w, 0.1, 0.1, 0.4, vv.SAGITTAL, samples=4, thickness=0.5)
                else:
                    empty.slice_advanced_slab(h, w, _free_form(), samples=4, thickness=0.5)
            assert e.value.code == ERR_NO_VOLUME
    # the context is still usable: a good call matches the model
    orient, d = CANONICAL["coronal"]
    got = ctx.slice_slab(17, 23, *d, orient, mode=vv.SLAB_MIN, samples=7, thickness=0.5, fill=FILL, return_aux=True, aux_fill=AUX_FILL)
    _same_pair(got, SM.slab_canonical(vol, 17, 23, *d, orient, SM.SLAB_MIN, 7, 0.5), "a good call after the refused ones")


@pytest.mark.gpu
def test_slab_leaves_the_context_alone(ctx, monkeypatch):
    _load(ctx, monkeypatch, "aniso")
    cam = vv.Camera.orbit(3.0, 1.0, 0.6)
    orient, d = CANONICAL["sagittal"]
    state = ctx.layout_state()
    slice_before = ctx.slice(33, 19, *d, orient, fill=FILL)
    frame_before = ctx.render(57, 43, cam, fill=1)
    state_rendered = ctx.layout_state()
    for mode, _ in MODES:
        ctx.slice_slab(33, 19, *d, orient, mode=mode, samples=16, thickness=1.4, return_aux=True)
        ctx.slice_advanced_slab(12, 40, _free_form(), mode=mode, samples=5, thickness=0.25)
    assert ctx.layout_state() == state_rendered
    _same(ctx.slice(33, 19, *d, orient, fill=FILL), slice_before, "vv_slice after slab calls")
    assert np.array_equal(ctx.render(57, 43, cam, fill=1), frame_before)
    assert ctx.layout_state() == state_rendered and state["linear"] == state_rendered["linear"]
