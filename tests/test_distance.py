"""The distance transform (vv_distance_volume) and Context.morphology against tests/distance_model.py, every word exactly.

CPU part: the header, the library and the binding export the call, the structure has the header's size, the model equals the brute-force minimum
over all (voxel, seed) pairs and np.rint(edt^2) of scipy.ndimage.distance_transform_edt, and the model's own identities hold.  GPU part: the words
equal the model on every shape, seed pattern, spacing, source, box and output mode of the issue, into a guarded device buffer prefilled with 0xA5
whose start moves by 4 bytes from call to call, and through the host path; out == labels gives the words of the separate-buffer call; whatever the
block order (VV_DISTANCE_BLOCKS), the layout, the pitch and the load path; the four morphology operations equal the model's; every error of the
rule list is refused in order; and the calls leave the context alone.

Not tested: the overlap of `out` with the context's volume allocation (no public call tells its address) and the 2^32 - 2 voxel limit (a box that
large has an extent above 2048 or a volume that is not loaded here)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import distance_model as DM
import hist_model as HM
import label_model as LM
import test_hist as TH
import volume_out as VO
import volviz_amd as vv
from volume_out import GARBAGE, GUARD

f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2
TF = TH.TF
THREADS, WAVE = 256, 64                                    # kDtThreads, kDtWave of csrc/vv_distance.hip: a wave takes a row in chunks of 64 voxels
COLS = {256: 32, 512: 16, 1024: 8, 2048: 8}                # dt_cols: lines per tile of distance_line_kernel<NCAP>, by the line's capacity
LAYOUT_KNOBS = TH.LAYOUT_KNOBS + ("VV_DERIVE_BLOCKS", "VV_LABEL_BLOCKS", "VV_DISTANCE_BLOCKS", "VV_DISTANCE_PHASES")
FG, BG = 200, 7                                            # the built volumes: a seed's byte, every other voxel's
SPACINGS = ((1, 1, 1), (1, 2, 5), (3, 1, 2))
REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _line_shapes():
    out = []
    for n in (WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1):
        out += [f"{n}x3x2", f"3x{n}x2", f"3x2x{n}"]
    return out


SHAPES = (["1x1x1", "2x1x3", "1x40x1"] + _line_shapes() + [f"{COLS[256] + d}x5x3" for d in (0, 1, -1)] +
          [f"{COLS[512] + 1}x300x2", f"{COLS[1024] + 1}x2x600", "37x21x13", "1x2048x1", "1x1x2048", "2048x1x1", f"{COLS[2048] + 1}x1x1100"])
PATTERNS = ("none", "all") + tuple(f"corner{k}" for k in range(8)) + ("centre", "ends_x", "ends_y", "ends_z", "plane_x", "plane_y", "plane_z", "gaps", "half")


def _dims(shape):
    return tuple(int(s) for s in shape.split("x"))


@functools.lru_cache(maxsize=None)
def _built(shape, pattern):
    """A u8 volume [nz, ny, nx] whose seeds (byte FG on a background of BG) form `pattern`."""
    nx, ny, nz = _dims(shape)
    v = np.full((nz, ny, nx), BG, np.uint8)
    if pattern == "all":
        v[...] = FG
    elif pattern.startswith("corner"):
        k = int(pattern[6:])
        v[(nz - 1) * (k >> 2 & 1), (ny - 1) * (k >> 1 & 1), (nx - 1) * (k & 1)] = FG
    elif pattern == "centre":
        v[nz // 2, ny // 2, nx // 2] = FG
    elif pattern.startswith("ends_"):                          # two seeds at a line's ends: the ties fall in the middle
        a = "zyx".index(pattern[5])
        at = [nz // 2, ny // 2, nx // 2]
        for e in (0, v.shape[a] - 1):
            at[a] = e
            v[tuple(at)] = FG
    elif pattern.startswith("plane_"):
        idx = [slice(None)] * 3
        idx["zyx".index(pattern[6])] = 0
        v[tuple(idx)] = FG
    elif pattern == "gaps":                                    # planes and rows without a seed between seeded ones
        v[::2, ::3, ::4] = FG
    elif pattern == "half":
        v[np.random.default_rng(nx * 31 + ny * 7 + nz).random(v.shape) < 0.5] = FG
    else:
        assert pattern == "none"
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _random(kind, p_inv):
    """70 x 40 x 20, seeds (bin 0) at probability 1 / p_inv; u8, or f32 with NaN, -Inf (bin 0 too) and +Inf (bin 255) voxels."""
    rng = np.random.default_rng(4000 + p_inv)
    shape = (20, 40, 70)
    hit = rng.random(shape) < 1.0 / p_inv
    if kind == "u8":
        v = rng.integers(1, 256, shape, dtype=np.uint8)
        v[hit] = 0
    else:
        v = (rng.random(shape, dtype=f32) * f32(0.9) + f32(0.05)).astype(f32)
        v[hit] = f32(0.001)
        flat = v.reshape(-1)
        sp = rng.choice(flat.size, 9, replace=False)
        flat[sp[:3]], flat[sp[3:6]], flat[sp[6:]] = np.nan, -np.inf, np.inf
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want_built(shape, pattern, spacing, r2=None):
    """The model's words of one built case: computed once, shared by the tests, never changed."""
    w = DM.distance(_built(shape, pattern), (FG, FG), spacing=spacing, within_r2=r2)
    w.setflags(write=False)
    return w


def _check(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (what, got.shape, want.shape, got.dtype, want.dtype)
    VO.report(got, want, DM.same(got, want), what)


def _edt2(seed, spacing):
    ndimage = pytest.importorskip("scipy.ndimage")
    if not seed.any():
        return np.full(seed.shape, DM.NONE, np.uint32)
    e = ndimage.distance_transform_edt(~seed, sampling=(spacing[2], spacing[1], spacing[0]))
    return np.rint(e * e).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_distance_call():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "volviz.h")).read(), flags=re.S)
    assert re.search(r"\bvv_distance_volume\s*\(", header), "include/volviz.h does not declare vv_distance_volume"
    lib = vv.load_library()
    assert "vv_distance_volume" in vv.EXPORTS and "vv_distance_volume" in vv._NEWER_EXPORTS and hasattr(lib, "vv_distance_volume")
    for name in ("distance", "distance_device", "morphology"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert (vv.SEED_BINS, vv.SEED_LABEL, vv.SEED_NONZERO) == (0, 1, 2) == (DM.SEED_BINS, DM.SEED_LABEL, DM.SEED_NONZERO)
    assert (vv.DIST_SQUARED, vv.DIST_WITHIN) == (0, 1)
    assert (vv.MORPH_DILATE, vv.MORPH_ERODE, vv.MORPH_OPEN, vv.MORPH_CLOSE) == (DM.DILATE, DM.ERODE, DM.OPEN, DM.CLOSE)
    assert vv.DISTANCE_MAX_EXTENT == DM.MAX_EXTENT == 2048 and vv.DISTANCE_NONE == DM.NONE
    assert re.search(r"#define\s+VV_DISTANCE_MAX_EXTENT\s+2048\b", header)


def test_structure_matches_the_header():
    d = vv.vv_distance
    assert C.sizeof(d) == 64
    assert (d.box_lo.offset, d.box_hi.offset, d.seed.offset, d.bin_lo.offset, d.bin_hi.offset, d.label.offset, d.invert.offset, d.spacing.offset,
            d.out.offset, d.within_r2.offset) == (0, 12, 24, 28, 32, 36, 40, 44, 56, 60)


@pytest.mark.parametrize("shape", [(7, 9, 13), (1, 1, 1), (3, 1, 2), (1, 11, 1), (5, 4, 3)])
def test_model_equals_the_minimum_over_all_pairs(shape):
    rng = np.random.default_rng(sum(shape))
    for p in (0.5, 0.1, 0.01, 0.0, 1.0):
        seed = rng.random(shape) < p
        for spacing in SPACINGS:
            assert np.array_equal(DM.squared(seed, spacing), DM.brute(seed, spacing)), (shape, p, spacing)


def test_model_equals_scipy():
    rng = np.random.default_rng(77)
    for spacing in SPACINGS:
        for p in (0.5, 0.02, 0.0002):
            seed = rng.random((20, 40, 70)) < p
            assert np.array_equal(DM.squared(seed, spacing), _edt2(seed, spacing)), (spacing, p)
    seed = np.zeros((258, 1, 1), bool)
    seed[0] = True
    limit = DM.squared(seed, (1, 1, 255))
    assert int(limit[-1, 0, 0]) == 65535 ** 2 == 4294836225 > 2 ** 31 and np.array_equal(limit, _edt2(seed, (1, 1, 255)))
    assert not DM.limits_ok((259, 1, 1), (1, 1, 255)) and DM.limits_ok((258, 1, 1), (1, 1, 255))
    seed = rng.random((1, 2048, 1)) < 0.003
    assert seed.any() and np.array_equal(DM.squared(seed, (1, 1, 1)), _edt2(seed, (1, 1, 1)))


def test_model_identities():
    rng = np.random.default_rng(78)
    seed = rng.random((13, 21, 37)) < 0.03
    for spacing in SPACINGS:
        d = DM.squared(seed, spacing)
        assert np.array_equal(d == 0, seed)                                  # D = 0 exactly on the seeds
        assert not DM.squared(np.ones(seed.shape, bool), spacing).any()     # all seeds: all 0
        assert (DM.squared(np.zeros(seed.shape, bool), spacing) == DM.NONE).all() and not DM.within(np.zeros(seed.shape, bool), 0xFFFFFFFE, spacing).any()
        crop = (slice(2, 11), slice(3, 17), slice(5, 30))                     # a crop of D is at most D of the crop's box (the box loses seeds)
        assert (d[crop] <= DM.squared(seed[crop], spacing)).all()
        assert np.array_equal(DM.within(seed, 0, spacing), seed.astype(np.uint32))
    blob = DM.within(seed, 9).astype(bool) & (rng.random(seed.shape) < 0.9)
    for radius in (1, 1.5, 2, 3):
        dil, ero, opn, cls = (DM.morphology(op, blob, radius).astype(bool) for op in (DM.DILATE, DM.ERODE, DM.OPEN, DM.CLOSE))
        assert (dil >= blob).all() and (blob >= ero).all() and (opn <= blob).all() and (blob <= cls).all()
        assert dil.sum() > blob.sum() > ero.sum()
    full = np.ones((5, 6, 7), bool)
    assert DM.morphology(DM.ERODE, full, 3).all(), "an erosion must not eat in from the box's faces"
    assert (DM.radius2(1.5), DM.radius2(1), DM.radius2(3), DM.radius2(2.9999)) == (2, 1, 9, 8)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _load(ctx, monkeypatch, vol):
    VO.load(ctx, monkeypatch, LAYOUT_KNOBS, vol, TF)


def _device(ctx, dev, shape, what, labels_ptr=0, **kw):
    """One call into the guarded device buffer (float32 to VolumeOut: a start that moves by 4 bytes) -> the words [bz, by, bx]."""
    got = dev.run(lambda p, cap: ctx.distance_device(p, cap, labels_ptr=labels_ptr, **kw), shape, np.float32, what)
    return got.view(np.uint32)


def _run_case(ctx, dev, what, want, host=True, labels=None, **kw):
    """One case through the device buffer and, with `host`, through host pointers (prefilled with GARBAGE or 0 in turn)."""
    import torch
    lab_t = torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).copy()).to(torch.device("cuda", 0)) if labels is not None else None
    what = f"{what} {kw}"
    _check(_device(ctx, dev, want.shape, what, labels_ptr=lab_t.data_ptr() if lab_t is not None else 0, **kw), want, what)
    if host:
        _check(ctx.distance(labels=labels, prefill=GARBAGE if dev.calls % 2 else 0, **kw), want, what + " host")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_distance_shapes(ctx, shape, monkeypatch):
    """Every seed pattern on every shape: no seed, all seeds, one at each corner, one in the centre, two at a line's ends, a plane x = 0, y = 0 or
    z = 0, seeded planes and rows with empty ones between, random seeds at 1 / 2; the three spacings in turn."""
    nx, ny, nz = _dims(shape)
    dev = VO.DeviceOut(nx * ny * nz * 4)
    seen = set()
    for k, pattern in enumerate(PATTERNS):
        vol = _built(shape, pattern)
        if vol.tobytes() in seen:                                 # (corners of a flat volume coincide)
            continue
        seen.add(vol.tobytes())
        _load(ctx, monkeypatch, vol)
        spacing = SPACINGS[k % 3]
        want = _want_built(shape, pattern, spacing)
        if pattern == "none":
            assert (want == DM.NONE).all()
        _run_case(ctx, dev, f"{shape} {pattern}", want, host=k % 2 == 0, bins=(FG, FG), spacing=spacing)
        if k % 4 == 1:
            r2 = int(want.max()) // 2 if pattern != "none" else 5
            _run_case(ctx, dev, f"{shape} {pattern}", _want_built(shape, pattern, spacing, r2), host=False, bins=(FG, FG), spacing=spacing, within=r2)


@pytest.mark.gpu
@pytest.mark.parametrize("p_inv", [2, 50, 5000])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_distance_random(ctx, kind, p_inv, monkeypatch):
    """70 x 40 x 20, random seeds at 1 / 2, 1 / 50 and 1 / 5000; the f32 volume holds NaN and -Inf (bin 0: seeds) and +Inf (bin 255)."""
    vol = _random(kind, p_inv)
    _load(ctx, monkeypatch, vol)
    dev = VO.DeviceOut(vol.size * 4)
    for spacing in SPACINGS:
        want = DM.distance(vol, (0, 0), spacing=spacing)
        assert 0 < int((want == 0).sum()) < vol.size
        if kind == "f32":
            assert (want[np.isnan(vol) | (vol == -np.inf)] == 0).all() and (want[vol == np.inf] > 0).all()
        _run_case(ctx, dev, f"random {kind} 1/{p_inv}", want, bins=(0, 0), spacing=spacing)
    if kind == "f32":
        want = DM.distance(vol, (255, 255))
        assert int((want == 0).sum()) == 3 and (want[vol == np.inf] == 0).all()
        _run_case(ctx, dev, "the +Inf voxels", want, bins=(255, 255))
        _run_case(ctx, dev, "all but the +Inf voxels", DM.distance(vol, (255, 255), invert=True), bins=(255, 255), invert=True)


@pytest.mark.gpu
def test_distance_at_the_32_bit_limit(ctx, monkeypatch):
    """1 x 1 x 258 with spacing z = 255 and a seed at z = 0: the far end is 65535^2 = 4294836225, above 2^31.  259 slices are refused."""
    vol = np.full((259, 1, 1), BG, np.uint8)
    vol[0] = FG
    _load(ctx, monkeypatch, vol)
    box = ((0, 0, 0), (1, 1, 258))
    want = DM.distance(vol, (FG, FG), spacing=(1, 1, 255), box=box)
    assert int(want[-1, 0, 0]) == 4294836225 and int(want[129, 0, 0]) == (255 * 129) ** 2 < 2 ** 31 < int(want[200, 0, 0])
    dev = VO.DeviceOut(259 * 4)
    _run_case(ctx, dev, "the limit line", want, bins=(FG, FG), spacing=(1, 1, 255), box=box)
    for r2 in (4294836225, 4294836224, 0xFFFFFFFE, 2 ** 31, 2 ** 31 - 1):
        _run_case(ctx, dev, "the limit line", DM.distance(vol, (FG, FG), spacing=(1, 1, 255), box=box, within_r2=r2), bins=(FG, FG), spacing=(1, 1, 255), box=box, within=r2)
    far =np.full((258, 1, 1), BG, np.uint8)                           # the seed at the far end: the parabola's position term is the large one
    far[257] = FG
    _load(ctx, monkeypatch, far)
    _run_case(ctx, dev, "the limit line, seed at the far end", DM.distance(far, (FG, FG), spacing=(1, 1, 255)), bins=(FG, FG), spacing=(1, 1, 255))
    _load(ctx, monkeypatch, vol)
    with pytest.raises(vv.VolvizError) as e:
        ctx.distance(bins=(FG, FG), spacing=(1, 1, 255))
    assert e.value.code == ERR_INVALID and "largest squared" in str(e.value)
    _check(ctx.distance(bins=(FG, FG), spacing=(1, 1, 254), prefill=GARBAGE), DM.distance(vol, (FG, FG), spacing=(1, 1, 254)), "259 slices at spacing 254")


@pytest.mark.gpu
def test_distance_sources(ctx, monkeypatch):
    """Bins give the seeds of ctx.label's foreground; VV_SEED_LABEL and VV_SEED_NONZERO on labels from ctx.label; invert of each; a labels input
    that is a VV_DIST_WITHIN result."""
    vol = TH._volume("aniso")
    _load(ctx, monkeypatch, vol)
    dev = VO.DeviceOut(vol.size * 4)
    for bins in ((60, 60), (80, 120)):
        labels = ctx.label(bins, 6)
        assert np.array_equal(labels != 0, LM.foreground(vol, bins))
        for invert in (False, True):
            for spacing in SPACINGS[:2]:
                want = DM.distance(vol, bins, invert=invert, spacing=spacing)
                _run_case(ctx, dev, "bins", want, bins=bins, invert=invert, spacing=spacing)
                _run_case(ctx, dev, "nonzero labels", want, labels=labels, invert=invert, spacing=spacing)       # the same seeds
            some = int(np.unique(labels[labels > 0])[-1])
            _run_case(ctx, dev, "one label", DM.distance(labels=labels, label=some, invert=invert), labels=labels, label=some, invert=invert)
            _run_case(ctx, dev, "label 0", DM.distance(labels=labels, label=0, invert=invert), labels=labels, label=0, invert=invert)
        grown = ctx.distance(bins=bins, within=4, prefill=GARBAGE)
        _check(grown, DM.distance(vol, bins, within_r2=4), "within 4")
        for invert in (False, True):
            _run_case(ctx, dev, "a WITHIN result as labels", DM.distance(labels=grown, invert=invert, spacing=(3, 1, 2)), labels=grown, invert=invert, spacing=(3, 1, 2))


@pytest.mark.gpu
def test_distance_boxes(ctx, monkeypatch):
    """Sub-boxes with a seed one voxel outside each face (not seen), boxes that start at odd offsets, one voxel, one row."""
    rng = np.random.default_rng(91)
    vol = np.full((20, 40, 70), BG, np.uint8)
    box = ((11, 7, 5), (52, 30, 16))
    (x0, y0, z0), (x1, y1, z1) = box
    for z, y, x in ((z0 - 1, 20, 30), (z1, 20, 30), (10, y0 - 1, 30), (10, y1, 30), (10, 20, x0 - 1), (10, 20, x1)):
        vol[z, y, x] = FG
    _load(ctx, monkeypatch, vol)
    dev = VO.DeviceOut(vol.size * 4)
    want = DM.distance(vol, (FG, FG), box=box)
    assert (want == DM.NONE).all(), "a seed outside the box must not be seen"
    _run_case(ctx, dev, "seeds outside every face", want, bins=(FG, FG), box=box)
    _run_case(ctx, dev, "seeds outside every face, within", DM.distance(vol, (FG, FG), box=box, within_r2=0xFFFFFFFE), bins=(FG, FG), box=box, within=0xFFFFFFFE)
    vol = vol.copy()
    vol[12, 21, 33] = FG                                           # ... and one inside
    vol[rng.random(vol.shape) < 0.001] = FG
    _load(ctx, monkeypatch, vol)
    boxes = [box, ((3, 5, 1), (70, 40, 20)), ((17, 9, 9), (18, 10, 10)), ((1, 1, 1), (69, 39, 19)), ((33, 21, 11), (34, 22, 14)), ((5, 0, 3), (6, 40, 4)), ((1, 3, 5), (66, 4, 6))]
    for k, bx in enumerate(boxes):
        spacing = SPACINGS[k % 3]
        _run_case(ctx, dev, "box", DM.distance(vol, (FG, FG), spacing=spacing, box=bx), bins=(FG, FG), spacing=spacing, box=bx)
        labels = HM.crop(vol, bx).astype(np.uint32)
        _run_case(ctx, dev, "box, labels", DM.distance(labels=labels, label=BG, spacing=spacing), labels=labels, label=BG, spacing=spacing, box=bx)


@pytest.mark.gpu
def test_distance_within_and_aliasing(ctx, monkeypatch):
    """VV_DIST_WITHIN at r^2 = 0, 1, 2, 3, 4, 9, the maximum of D and 0xFFFFFFFE; out == labels on the device and on the host gives the words of the
    separate-buffer call."""
    import torch
    tdev = torch.device("cuda", 0)
    vol = _random("u8", 50)
    _load(ctx, monkeypatch, vol)
    dev = VO.DeviceOut(vol.size * 4)
    d = DM.distance(vol, (0, 0))
    dmax = int(d.max())
    for r2 in (0, 1, 2, 3, 4, 9, dmax - 1, dmax, 0xFFFFFFFE):
        want = DM.distance(vol, (0, 0), within_r2=r2)
        assert (r2 < dmax) == (not want.all())
        _run_case(ctx, dev, "within", want, bins=(0, 0), within=r2, host=r2 in (0, 3, dmax))
    labels = ctx.label((0, 40), 6)
    lab = int(np.bincount(labels[labels > 0]).argmax())
    cases = [dict(label=None), dict(label=lab), dict(label=lab, invert=True), dict(label=None, within=5), dict(label=None, invert=True, spacing=(1, 2, 5)),
             dict(label=lab, spacing=(3, 1, 2), within=30)]
    buf = torch.full((vol.size + 2 * GUARD // 4,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    for kw in cases:
        want = DM.distance(labels=labels, label=kw.get("label"), invert=kw.get("invert", False), spacing=kw.get("spacing", (1, 1, 1)), within_r2=kw.get("within"))
        _run_case(ctx, dev, "separate buffers", want, labels=labels, **kw)
        buf.fill_(0xA5A5A5A5 - (1 << 32))
        buf[GUARD // 4:GUARD // 4 + vol.size] = torch.from_numpy(labels.reshape(-1).view(np.int32).copy()).to(tdev)
        torch.cuda.synchronize()
        p = buf.data_ptr() + GUARD
        assert ctx.distance_device(p, vol.size * 4, labels_ptr=p, **kw) == (70, 40, 20)
        raw = buf.cpu().numpy().view(np.uint32)
        assert (raw[:GUARD // 4] == 0xA5A5A5A5).all() and (raw[GUARD // 4 + vol.size:] == 0xA5A5A5A5).all(), "bytes outside the aliased buffer were written"
        _check(raw[GUARD // 4:GUARD // 4 + vol.size].reshape(want.shape), want, f"out == labels on the device {kw}")
        d = ctx._distance(None, True, kw.get("label"), kw.get("invert", False), kw.get("spacing", (1, 1, 1)), None, kw.get("within"))
        host = labels.copy()
        ctx._chk(ctx.lib.vv_distance_volume(ctx.h, C.byref(d), host.ctypes.data, host.ctypes.data, host.nbytes, 0, None))
        _check(host, want, f"out == labels on the host {kw}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["random", "gaps", "long_lines"])
def test_distance_block_order(ctx, case, monkeypatch):
    """VV_DISTANCE_BLOCKS = 1, 8 and unset: one block takes every row and tile in turn, eight share them, one block per item; the same words, and
    the same words from a second run."""
    vol = {"random": lambda: _random("u8", 50), "gaps": lambda: _built("37x21x13", "gaps"), "long_lines": lambda: _built(f"{COLS[512] + 1}x300x2", "half")}[case]()
    bins = (0, 0) if case == "random" else (FG, FG)
    _load(ctx, monkeypatch, vol)
    dev = VO.DeviceOut(vol.size * 4)
    want = DM.distance(vol, bins, spacing=(1, 2, 5))
    try:
        for blocks in ("1", "8", None):
            if blocks is None:
                monkeypatch.delenv("VV_DISTANCE_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("VV_DISTANCE_BLOCKS", blocks)
            ctx.reread_env()
            _run_case(ctx, dev, f"VV_DISTANCE_BLOCKS={blocks} {case}", want, bins=bins, spacing=(1, 2, 5))
            first, second = ctx.distance(bins=bins, spacing=(1, 2, 5), prefill=GARBAGE), ctx.distance(bins=bins, spacing=(1, 2, 5), prefill=0)
            assert first.tobytes() == second.tobytes(), "a second run differs"
            _check(ctx.morphology(vv.MORPH_CLOSE, 2, bins=bins), DM.morphology(DM.CLOSE, DM.seeds(vol, bins), 2), f"closing under VV_DISTANCE_BLOCKS={blocks}")
    finally:
        monkeypatch.delenv("VV_DISTANCE_BLOCKS", raising=False)
        ctx.reread_env()


@pytest.mark.gpu
@VO.layout_sweep
def test_distance_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume (32 bytes of zeros behind every row, with and without an extra row of zeros per slice) and the 64-bit addressing build.
    The volume holds no zero: bin 0 has no voxel unless padding is read as data."""
    with VO.layout_context(kind, nx, knobs, monkeypatch, LAYOUT_KNOBS, TF) as (c, vol):
        nz, ny, _ = vol.shape
        dev = VO.DeviceOut(vol.size * 4)
        for bins, box, spacing in (((1, 8), None, (1, 1, 1)), ((200, 255), ((1, 0, 1), (nx - 1, ny, nz - 1)), (1, 2, 5)), ((250, 255), ((3, 2, 1), (nx, ny - 1, nz)), (3, 1, 2))):
            _run_case(c, dev, f"layout {kind} {knobs}", DM.distance(vol, bins, spacing=spacing, box=box), bins=bins, spacing=spacing, box=box)
        assert (c.distance(bins=(0, 0), prefill=GARBAGE) == DM.NONE).all(), "padding was read as data"


@pytest.mark.gpu
def test_distance_load_paths_and_streams(ctx, monkeypatch):
    """A volume that came from a device buffer and one promoted by the streamed upload; then enqueue-only calls on a torch stream, synchronised by
    the stream alone."""
    import torch
    tdev = torch.device("cuda", 0)
    vol8 = np.random.default_rng(5).integers(0, 256, (13, 21, 37), dtype=np.uint8)
    dev = VO.DeviceOut(vol8.size * 4)
    for (what, loaded), spacing in zip(VO.load_paths(ctx, monkeypatch, LAYOUT_KNOBS, vol8, TF), ((1, 2, 5), (3, 1, 2))):
        _run_case(ctx, dev, what, DM.distance(loaded, (0, 3), spacing=spacing), bins=(0, 3), spacing=spacing)
    # enqueue only: the distances, a margin, and the margin's complement grown again, in place
    vol = _random("u8", 50)
    _load(ctx, monkeypatch, vol)
    n = vol.size
    ts = torch.cuda.Stream(device=tdev)
    d_t = torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    w_t = torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    torch.cuda.synchronize()
    with torch.cuda.stream(ts):
        h = vv.stream_handle(ts)
        assert ctx.distance_device(d_t.data_ptr(), n * 4, bins=(0, 0), stream=h) == (70, 40, 20)
        ctx.distance_device(w_t.data_ptr(), n * 4, bins=(0, 0), within=9, stream=h)
        ctx.distance_device(w_t.data_ptr(), n * 4, labels_ptr=w_t.data_ptr(), invert=True, within=9, stream=h)
    ts.synchronize()
    _check(d_t.cpu().numpy().view(np.uint32).reshape(vol.shape), DM.distance(vol, (0, 0)), "enqueue-only distances")
    opened_complement = DM.within(~DM.within(DM.seeds(vol, (0, 0)), 9).astype(bool), 9)
    _check(w_t.cpu().numpy().view(np.uint32).reshape(vol.shape), opened_complement, "enqueue-only composition in place")


@pytest.mark.gpu
def test_morphology_matches_the_model(ctx, monkeypatch):
    """All four operations at radius 1, 1.5, 2 and 3, from bins and from labels; ctx.mask of an opening equals the model's masked volume."""
    vol = TH._volume("aniso")
    _load(ctx, monkeypatch, vol)
    bins = (80, 120)
    seed = DM.seeds(vol, bins)
    labels = ctx.label(bins, 6)
    lab = int(np.bincount(labels[labels > 0]).argmax())
    for radius in (1, 1.5, 2, 3):
        for op in (vv.MORPH_DILATE, vv.MORPH_ERODE, vv.MORPH_OPEN, vv.MORPH_CLOSE):
            _check(ctx.morphology(op, radius, bins=bins), DM.morphology(op, seed, radius), f"morphology {op} radius {radius} of bins")
    for op in (vv.MORPH_DILATE, vv.MORPH_ERODE, vv.MORPH_OPEN, vv.MORPH_CLOSE):
        _check(ctx.morphology(op, 1.5, labels=labels, spacing=(1, 2, 5)), DM.morphology(op, seed, 1.5, (1, 2, 5)), f"morphology {op} of nonzero labels, spacing (1, 2, 5)")
        _check(ctx.morphology(op, 2, labels=labels, label=lab), DM.morphology(op, labels == lab, 2), f"morphology {op} of one label")
    box = ((3, 5, 7), (18, 30, 44))
    _check(ctx.morphology(vv.MORPH_ERODE, 2, bins=(0, 255), box=box), np.ones((37, 25, 15), np.uint32), "the erosion of a full box")
    _check(ctx.morphology(vv.MORPH_OPEN, 2, bins=bins, box=box), DM.morphology(DM.OPEN, DM.seeds(vol, bins, box=box), 2), "an opening in a box")
    opened = ctx.morphology(vv.MORPH_OPEN, 1.5, bins=bins)
    assert 0 < int(opened.sum()) <= int(seed.sum())
    for out_type in (vv.VOXEL_U8, vv.VOXEL_F32):
        got = ctx.mask(opened, vv.KEEP_FOREGROUND, fill=0.0, out_type=out_type, prefill=GARBAGE)
        want = LM.mask(vol, DM.morphology(DM.OPEN, seed, 1.5), LM.KEEP_FOREGROUND, fill=0.0, out_type=out_type)
        VO.report(got, want, LM.same(got, want), f"the mask of an opening, out_type {out_type}")
    with pytest.raises(ValueError):
        ctx.morphology(vv.MORPH_OPEN, 1, bins=bins, labels=labels)
    with pytest.raises(ValueError):
        ctx.morphology(vv.MORPH_OPEN, 1)
    with pytest.raises(ValueError):
        ctx.distance()
    with pytest.raises(ValueError):
        ctx.distance(bins=bins, labels=labels)


@pytest.mark.gpu
def test_distance_errors_and_state(ctx, monkeypatch):
    """Every refusal of the header's rule 10, the first failing rule winning; a refused call leaves GARBAGE everywhere and the context usable; the
    calls leave the volume, the table, the layout state, vv_last_frame_ms and device_bytes alone and allocate no device memory."""
    import torch
    tdev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h

    def mk(lo=(0, 0, 0), hi=(0, 0, 0), seed=vv.SEED_BINS, bin_lo=0, bin_hi=100, label=0, invert=0, spacing=(1, 1, 1), out=vv.DIST_SQUARED, r2=0):
        d = vv.vv_distance()
        d.box_lo[:], d.box_hi[:], d.spacing[:] = lo, hi, spacing
        d.seed, d.bin_lo, d.bin_hi, d.label, d.invert, d.out, d.within_r2 = seed, bin_lo, bin_hi, label, invert, out, r2
        return d

    def err():
        return lib.vv_last_error(hnd).decode()

    with vv.Context(0) as empty:                                    # before a load: behind the NULL checks, before a bad descriptor
        out = np.full(256, GARBAGE, np.uint8)
        assert lib.vv_distance_volume(empty.h, C.byref(mk(seed=9)), None, out.ctypes.data, out.nbytes, 0, None) == ERR_NO_VOLUME
        assert lib.vv_distance_volume(empty.h, C.byref(mk(seed=vv.SEED_NONZERO)), out.ctypes.data, out.ctypes.data, out.nbytes, 0, None) == ERR_NO_VOLUME
        assert lib.vv_distance_volume(empty.h, None, None, out.ctypes.data, out.nbytes, 0, None) == ERR_INVALID
        assert lib.vv_distance_volume(empty.h, C.byref(mk()), None, None, out.nbytes, 0, None) == ERR_INVALID
        assert (out == GARBAGE).all()
    # the order of the rules, on a volume one voxel longer than the longest line
    long_vol = np.full((1, 1, 2049), BG, np.uint8)
    long_vol[0, 0, 5] = FG
    _load(ctx, monkeypatch, long_vol)
    host = np.full(4 * 2049 * 2 + GUARD, GARBAGE, np.uint8)
    raw = torch.full((4 * 2049 * 2 + GUARD,), GARBAGE, dtype=torch.uint8, device=tdev)
    torch.cuda.synchronize()
    hp, dp = host.ctypes.data, raw.data_ptr()
    assert dp % 8 == 0
    short = dict(lo=(0, 0, 0), hi=(100, 1, 1))
    bad = dict(lo=(1, 0, 0), hi=(0, 0, 0), seed=7, bin_lo=9, bin_hi=3, invert=5, spacing=(0, 1, 1), out=9)
    steps = [(dict(), True, 0, 2, "lo < hi"), (dict(lo=(0, 0, 0)), True, 0, 2, "at most 2048"), (short, True, 0, 2, "seed must"),
             (dict(seed=vv.SEED_BINS), True, 0, 2, "bins must"), (dict(bin_lo=0), True, 0, 2, "labels must"), (dict(), False, 0, 2, "invert must"),
             (dict(invert=1), False, 0, 2, "spacing must"), (dict(spacing=(700, 1, 1)), False, 0, 2, "largest squared"), (dict(spacing=(600, 1, 1)), False, 0, 2, "out must"),
             (dict(out=vv.DIST_WITHIN), False, 0, 2, "capacity"), (dict(), False, 399, 2, "capacity"), (dict(), False, 400, 2, "aligned")]
    kw = dict(bad)
    for fix, with_labels, capacity, off, word in steps:
        kw.update(fix)
        assert lib.vv_distance_volume(hnd, C.byref(mk(**kw)), dp + 4096 if with_labels else None, dp + off, capacity, 1, None) == ERR_INVALID, (word, kw)
        assert word in err(), (word, err())
    assert lib.vv_distance_volume(None, C.byref(mk(**short)), None, hp, 400, 0, None) == ERR_INVALID
    assert lib.vv_distance_volume(hnd, None, None, hp, 400, 0, None) == ERR_INVALID
    assert lib.vv_distance_volume(hnd, C.byref(mk(**short)), None, None, 400, 0, None) == ERR_INVALID
    assert lib.vv_distance_volume(hnd, C.byref(mk()), None, dp, 4 * 2049, 1, None) == ERR_INVALID and "at most 2048" in err()          # extent 2049
    assert lib.vv_distance_volume(hnd, C.byref(mk()), None, hp, 4 * 2049, 0, None) == ERR_INVALID and "at most 2048" in err()
    # each rule alone, host and device agreeing
    nz_ = dict(short, seed=vv.SEED_NONZERO)

    def both(d, labels=False, capacity=400):
        rc = [lib.vv_distance_volume(hnd, C.byref(d), p + 4096 if labels else None, p, capacity, on, None) for p, on in ((hp, 0), (dp, 1))]
        assert rc[0] == rc[1], rc
        return rc[0]

    for lo, hi in (((-1, 0, 0), (5, 1, 1)), ((0, 0, 0), (2050, 1, 1)), ((0, 0, 0), (5, 2, 1)), ((3, 0, 0), (3, 1, 1)), ((1, 0, 0), (0, 0, 0))):
        assert both(mk(lo, hi)) == ERR_INVALID and "lo < hi" in err(), (lo, hi)
    for seed in (-1, 3, 99):
        assert both(mk(**dict(short, seed=seed))) == ERR_INVALID and "seed must" in err()
    for bin_lo, bin_hi in ((-1, 5), (0, 256), (7, 6)):
        assert both(mk(**dict(short, bin_lo=bin_lo, bin_hi=bin_hi))) == ERR_INVALID and "bins must" in err()
        assert both(mk(**dict(nz_, bin_lo=bin_lo, bin_hi=bin_hi)), labels=True) == 0                   # (bins are VV_SEED_BINS' alone)
    assert both(mk(**short), labels=True) == ERR_INVALID and "labels must" in err()
    for seed in (vv.SEED_LABEL, vv.SEED_NONZERO):
        assert both(mk(**dict(short, seed=seed))) == ERR_INVALID and "labels must" in err()
    for invert in (-1, 2):
        assert both(mk(**dict(short, invert=invert))) == ERR_INVALID and "invert must" in err()
    for spacing in ((0, 1, 1), (1, -1, 1), (1, 1, 0)):
        assert both(mk(**dict(short, spacing=spacing))) == ERR_INVALID and "spacing must" in err()
    for spacing in ((662, 1, 1), (2 ** 31 - 1, 1, 1)):                                                   # 662 * 99 = 65538
        assert both(mk(**dict(short, spacing=spacing))) == ERR_INVALID and "largest squared" in err()
    assert both(mk(**dict(short, spacing=(661, 2 ** 31 - 1, 2 ** 31 - 1)))) == 0                        # 661 * 99 = 65439; flat axes add nothing
    for out in (-1, 2):
        assert both(mk(**dict(short, out=out))) == ERR_INVALID and "out must" in err()
    assert both(mk(**short), capacity=399) == ERR_INVALID and "capacity" in err()
    for off in (1, 2, 3):
        assert lib.vv_distance_volume(hnd, C.byref(mk(**short)), None, dp + off, 400, 1, None) == ERR_INVALID and "aligned" in err()
        assert lib.vv_distance_volume(hnd, C.byref(mk(**nz_)), dp + 4096 + off, dp, 400, 1, None) == ERR_INVALID and "aligned" in err()
    for loff in (4, 396, -4, -396):                                 # a partial overlap of out and labels, either way round
        assert lib.vv_distance_volume(hnd, C.byref(mk(**nz_)), dp + 1024 + loff, dp + 1024, 400, 1, None) == ERR_INVALID and "overlaps labels" in err(), loff
    host[:4096 + 400] = GARBAGE
    raw.fill_(GARBAGE)
    torch.cuda.synchronize()
    for seed in (7, vv.SEED_BINS):                                  # refused calls once more, on clean buffers
        assert lib.vv_distance_volume(hnd, C.byref(mk(**dict(short, seed=seed, invert=3))), None, hp, 400, 0, None) == ERR_INVALID
        assert lib.vv_distance_volume(hnd, C.byref(mk(**dict(short, seed=seed, invert=3))), None, dp, 400, 1, None) == ERR_INVALID
    assert lib.vv_distance_volume(hnd, C.byref(mk(**nz_)), dp + 4, dp, 400, 1, None) == ERR_INVALID
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # exactly the needed capacity is enough; the longest line that is allowed
    box = ((1, 0, 0), (2049, 1, 1))
    want = DM.distance(long_vol, (FG, FG), spacing=(5, 1, 1), box=box)
    assert lib.vv_distance_volume(hnd, C.byref(mk(*box, bin_lo=FG, bin_hi=FG, spacing=(5, 1, 1))), None, hp, 2048 * 4, 0, None) == 0
    _check(host[:2048 * 4].view(np.uint32).reshape(want.shape), want, "exact capacity")
    assert (host[2048 * 4:] == GARBAGE).all()
    # the context
    vol = TH._volume("aniso")
    _load(ctx, monkeypatch, vol)
    n = vol.size
    before = VO.Untouched(ctx)
    out_t = torch.empty(n, dtype=torch.int32, device=tdev)
    lab_t = torch.ones(n, dtype=torch.int32, device=tdev)

    def calls():
        for spacing in SPACINGS:
            ctx.distance_device(out_t.data_ptr(), n * 4, bins=(60, 100), spacing=spacing)
            ctx.distance_device(out_t.data_ptr(), n * 4, labels_ptr=out_t.data_ptr(), label=0, within=7, spacing=spacing)
            ctx.distance_device(out_t.data_ptr(), n * 4, labels_ptr=lab_t.data_ptr(), invert=True)

    VO.free_memory_unchanged(calls)
    assert bool((out_t == -1).all()), "every voxel a label, inverted: no seed"
    with pytest.raises(vv.VolvizError):
        ctx.distance(bins=(300, 400))
    _check(ctx.distance(bins=(60, 100), prefill=GARBAGE), DM.distance(vol, (60, 100)), "a good call after the refused ones")
    _check(ctx.morphology(vv.MORPH_OPEN, 1, bins=(60, 100)), DM.morphology(DM.OPEN, DM.seeds(vol, (60, 100)), 1), "an opening after the refused calls")
    before.check()
