"""The roofline's three instruments -- touched_bricks, touched_lines, touched_block_lines (vv_render_options) -- and the copy builders, held to
tests/footprint_model.py: a numpy statement of what every layout holds byte for byte, which bytes a sample loads from it, and hence which 8^3
bricks and 128-byte lines the executed samples of a frame touch.  Every bitmap comparison is word-for-word equality, except where the contract
itself is a containment: the issued set (touched_lines_all = 1 and the (block, line) pairs), which depends on the samples per loop trip and on idle
lanes and is not modelled -- it must contain the compulsory set, and the pairs' lines must be exactly its set bits --, and the Phong kernel, which
marks the cache entries 1..30 of its rays instead of the executed samples and is held between two modelled sets.

  volumes   brain (tests/golden/brain_aniso_20x36x52.u8: every dimension a multiple of 4, none of 8 -- the bricked copy has its clamped extra layer in
            y and in z, the last brick column's halo is a clamped voxel) as u8 and promoted to f32; noise 41 x 13 x 9 in both types (odd dimensions:
            partial last bricks, no extra layer; f32 rows of 164 bytes: not line-sized; every value of the f32 one distinct); the f32 brain once
            more with padded pitch (VV_PITCH_FORCE=1 VV_PITCH_PAD=32 VV_PITCH_ROWS=1)
  frames    48 x 40 pixels at the default step from three cameras: along the memory axis, a side view, an oblique view
  layouts   LAYOUTS below: the knobs that force each and the code vv_debug_last_launch must report; the z-fastest and the x-pair copy serve views
            whose screen x does not run along the volume's x only, so their cases take the side and the oblique camera

The CPU half ties gathers() to pack() through the witness's corner values and shows that every case is a working detector."""
import functools
import os

import numpy as np
import pytest

import footprint_model as FM
import iso_model as IM
import mip_oracle as MO
import proj_model as PM
import volviz_amd as vv
import witness as Wt

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 48, 40
# (the axis camera looks along z from beside the centre: part of the volume's front lies outside the frame, so no bitmap is simply full)
CAMS = {"axis": vv.Camera(origin=(0.5, 0.3, -3.0), look_at=(0.5, 0.3, 0.0)), "side": vv.Camera(origin=(2.4, 0.3, 1.1), look_at=(0.0, 0.3, 1.1)),
        "oblique": vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5), "front": vv.Camera()}
VIEWS = ("axis", "side", "oblique")
PITCH_KNOBS = {"VV_PITCH_FORCE": "1", "VV_PITCH_PAD": "32", "VV_PITCH_ROWS": "1"}
_LINEAR = {"VV_BRICKED": "0", "VV_ZPAIR": "0", "VV_ZFAST": "0"}
# name -> (knobs, layout code of vv_debug_last_launch, the model's layout, cameras, the copies to read out: (code, model layout))
LAYOUTS = {
    "linear":  (_LINEAR, 0, "linear", ("axis", "side", "oblique"), ((0, "linear"),)),
    "big":     (dict(_LINEAR, VV_FORCE_BIG="1"), 1, "linear", ("axis", "side", "oblique"), ((1, "linear"),)),
    "bricked": ({"VV_BRICKED": "1", "VV_ZFAST": "0"}, 2, "bricked", ("axis", "side", "oblique"), ((2, "bricked"),)),
    "zpair":   ({"VV_BRICKED": "0", "VV_ZPAIR": "1", "VV_ZFAST": "0"}, 3, "zpair", ("axis", "side", "oblique"), ((3, "zpair"),)),
    "zfast":   ({"VV_ZFAST": "1", "VV_ZPAIR": "0"}, 4, "zfast", ("side", "oblique"), ((4, "zfast"),)),
    "xpair":   ({"VV_ZFAST": "1"}, 5, "xpair", ("side", "oblique"), ((4, "zfast"), (5, "xpair"))),
    "pitched": (dict(_LINEAR, **PITCH_KNOBS), 0, "linear", ("axis", "side", "oblique"), ((0, "linear"),)),
}
VOLUMES = ("brain_u8", "brain_f32", "noise_f32", "noise_u8")
CASES = [(v, l) for v in VOLUMES for l in ("linear", "big", "bricked", "zpair", "zfast", "xpair")] + [("brain_f32", "pitched")]
FAMILY_LAYOUTS = ("linear", "bricked", "zpair")


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name.startswith("brain"):
        v = np.fromfile(os.path.join(HERE, "golden", "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
        if name == "brain_f32":
            v = v.astype(f32) / f32(255)
    elif name == "noise_u8":
        v = np.random.default_rng(41).integers(0, 256, (9, 13, 41), dtype=np.uint8)
    else:
        assert name == "noise_f32"
        n = 41 * 13 * 9
        v = ((np.random.default_rng(13).permutation(n).astype(f32) + f32(0.5)) / f32(n)).reshape(9, 13, 41)     # every value distinct, all in (0, 1)
        assert len(np.unique(v)) == n
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


def _dims(vol):
    return vol.shape[2], vol.shape[1], vol.shape[0]


def _geom(vol, layout_name):
    """The model's geometry of a case, from the contracts alone."""
    model = LAYOUTS[layout_name][2]
    if layout_name == "pitched":
        row, sl = FM.pitched_linear(vol.dtype, _dims(vol), 32, True, 1)
        return FM.dense_geom("linear", vol.dtype, _dims(vol), row, sl)
    return FM.dense_geom(model, vol.dtype, _dims(vol))


def _cam_kw(cam):
    return dict(cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y, scale=cam.scale)


@functools.lru_cache(maxsize=None)
def _rays(dims, cam_name, step=None, slab_rows=(0, 0), shard=None, size=(W, H)):
    return PM.owned_rays(dims, size[0], size[1], step=step, slab_rows=slab_rows, shard=shard, **_cam_kw(CAMS[cam_name]))


@functools.lru_cache(maxsize=None)
def _mip_samples(dims, cam_name, step=None, slab_rows=(0, 0), shard=None, size=(W, H)):
    """Texture coordinates of every executed sample of a reducer frame that runs every ray to its end (MIP, projection, a transparent composite)."""
    R, inv_scale = _rays(dims, cam_name, step, slab_rows, shard, size)
    tex, _ = FM.reducer_samples(R, inv_scale, PM.march)
    tex.setflags(write=False)
    return tex


def _expect(tex, vol, layout_name, line_bits):
    model = LAYOUTS[layout_name][2]
    return FM.bricks(tex, _dims(vol)), FM.lines(tex, model, vol.dtype, _geom(vol, layout_name), _dims(vol), line_bits)


def _line_bits(geom):
    return geom["alloc"] // FM.LINE + 64


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the model against the witness, and every case a working detector
# ---------------------------------------------------------------------------------------------------------------------
def _probe_coordinates(n, rng):
    """~n texture coordinates in [0, 1)^3: uniform ones, the faces and corners of the cube, and coordinates on and beside texel centres."""
    one = np.nextafter(f32(1), f32(0))
    edge = np.array([0, one, f32(0.5), np.nextafter(f32(0), f32(1))], f32)
    corners = np.stack(np.meshgrid(edge, edge, edge, indexing="ij"), -1).reshape(-1, 3)
    t = rng.random((n, 3), dtype=f32)
    faces = rng.random((n // 4, 3), dtype=f32)
    faces[np.arange(len(faces)), rng.integers(0, 3, len(faces))] = rng.choice(np.array([0, one], f32), len(faces))
    return np.minimum(np.concatenate([corners, t, faces]), one).astype(f32)


@pytest.mark.parametrize("name,layout", [(v, l) for v in VOLUMES for l in FM.LAYOUTS] + [("brain_f32", "pitched")])
def test_gathers_read_the_witness_corners_out_of_pack(name, layout):
    """Reading pack(vol) at gathers() gives the eight corner values of witness._corners, for ~10^4 coordinates with the faces and corners of [0, 1)^3:
    value for value, except the weight-0 upper corners of edge samples that the contracts leave free (see `free` below).  Every load of every layout
    stays inside the allocation."""
    vol = _volume(name)
    dims = _dims(vol)
    model = "linear" if layout == "pitched" else layout
    geom = _geom(vol, layout)
    if layout == "pitched":
        assert (geom["row"], geom["slice"]) == (20 * 4 + 32, (36 + 1) * (20 * 4 + 32))
    buf = FM.pack(vol, model, geom)
    assert buf.shape == (geom["alloc"],)
    tex = _probe_coordinates(10000, np.random.default_rng(5))
    # on and next to every texel centre of each axis, too: where the base texel changes
    for a, n in enumerate(dims):
        c = ((np.arange(n, dtype=f32) + f32(0.5)) / f32(n)).astype(f32)
        extra = np.full((3 * n, 3), f32(0.37), f32)
        extra[:, a] = np.concatenate([c, np.nextafter(c, f32(0)), np.nextafter(c, f32(1))])
        tex = np.concatenate([tex, np.minimum(extra, np.nextafter(f32(1), f32(0)))])
    assert FM.in_volume(tex).all()
    axes = [Wt._axis(tex[:, a], n, Wt.FILTER_EXACT) for a, n in enumerate(dims)]
    ix, iy, iz = (ax[0] for ax in axes)
    for off, length in FM.gathers(model, vol.dtype, geom, ix, iy, iz):
        assert off.min() >= 0 and (off + length).max() <= geom["alloc"], (layout, int(off.max()), geom)
    got = FM.corners(buf, model, vol.dtype, geom, ix, iy, iz)
    want = np.stack([np.stack([np.stack(row, -1) for row in plane], -2) for plane in Wt._corners(vol, *axes)], -3)     # [n, z, y, x]
    assert got.shape == want.shape
    care = np.ones(want.shape, bool)
    for a, (lo, hi, w, _) in enumerate(axes):
        # Where the witness's two texels of an axis coincide (the coordinate lies at or beyond the first / last texel centre) the value does not depend on the
        # upper corner: the fetch clamps the coordinate, which makes the weight 0, and loads texel lo + 1 all the same.  Below the first centre that is
        # texel 1, not the witness's texel 0: free on every layout.  Beyond the last centre it is texel n: the clamped voxel again on the layouts that
        # store it (the halo and the extra layers of the bricks, the clamped records of the pair copies), anything on the linear and the z-fastest layout.
        free = (hi == lo) & ((lo == 0) | np.bool_(model in ("linear", "zfast")))
        sel = [slice(None)] * 4
        sel[3 - a] = 1                                          # axis a = x is the last of [n, z, y, x]
        care[tuple(sel)] &= ~free[:, None, None]
        assert (hi == lo).any() and (lo == dims[a] - 1).any() and (hi == lo + 1).any()
    assert care.mean() > 0.75
    assert np.array_equal(got[care], want[care]), (name, layout, int((got[care] != want[care]).sum()))
    for ax in axes:                                             # the probes reach both ends of every axis
        assert ax[0].min() == 0 and ax[0].max() == ax[1].max()


@pytest.mark.parametrize("name", VOLUMES)
def test_every_case_is_a_working_detector(name):
    """A case's compulsory line set is neither empty nor (copies of 32 KiB and more) the whole copy and differs from the set of every other layout; its
    brick set differs between the three cameras."""
    vol = _volume(name)
    dims = _dims(vol)
    brick_sets = {}
    for cam in VIEWS:
        tex = _mip_samples(dims, cam)
        assert len(tex) > 1000
        brick_sets[cam] = FM.bricks(tex, dims).tobytes()
        sets = {}
        for layout in FM.LAYOUTS + ("pitched",):
            if (layout == "pitched" and name != "brain_f32") or cam not in LAYOUTS[layout][3]:
                continue
            geom = _geom(vol, layout)
            ln = FM.line_numbers(tex, "linear" if layout == "pitched" else layout, vol.dtype, geom, dims)
            total = -(-geom["alloc"] // FM.LINE)
            # (a copy of fewer than 256 lines -- the 41 x 13 x 9 volumes' -- is touched whole by some views: a line of it spans several rows of every axis)
            assert 0 < len(ln) <= total and (len(ln) < total or total < 256) and ln.max() < total, (cam, layout, len(ln), total)
            sets[layout] = ln.tobytes()
        assert len(set(sets.values())) == len(sets), (cam, [k for k in sets])
    assert len(set(brick_sets.values())) == 3


def test_a_covering_frame_sets_every_brick_bit():
    """A frame along the memory axis that covers the volume at a fine step touches every 8^3 brick."""
    for name in ("brain_u8", "noise_f32"):
        dims = _dims(_volume(name))
        words = FM.bricks(_mip_samples(dims, "front", 1 / 128), dims)
        assert FM.bit_count(words) == FM.brick_bits(dims), (name, FM.bit_count(words), FM.brick_bits(dims))


def test_the_march_that_was_factored_out_counts_what_the_frame_counts():
    """reducer_samples over proj_model.march lists as many samples as proj_model.render executes, and the witness's `visit` as many as it counts."""
    vol = _volume("brain_u8")
    cam = CAMS["oblique"]
    tf = np.zeros(1024, f32)
    assert len(_mip_samples(_dims(vol), "oblique")) == PM.render_cam(vol, tf, W, H, cam, PM.PROJ_MAX)["count"]
    v = FM.Visit()
    _, n = Wt.render(vol, tf, W, H, visit=v, **_cam_kw(cam))
    assert n == len(v.samples()) == len(_mip_samples(_dims(vol), "oblique")) and n > 0
    assert np.array_equal(np.sort(v.samples().view(np.uint32), axis=0), np.sort(_mip_samples(_dims(vol), "oblique").view(np.uint32), axis=0))


# ---------------------------------------------------------------------------------------------------------------------
# composite, isosurface and Phong frames on the CPU: the samples, and that each case is real
# ---------------------------------------------------------------------------------------------------------------------
ERT_THRESHOLD = 0.9


def _opaque_table():
    """Opaque from index 40 on: rays end where they meet tissue."""
    tf = np.zeros((256, 4), f32)
    tf[40:] = (0.8, 0.7, 0.6, 0.6)
    return tf.reshape(1024)


def _faint_table():
    """Tissue at an opacity no ray accumulates to the threshold: a Phong frame shades its samples and runs every ray to its end."""
    tf = np.zeros((256, 4), f32)
    tf[40:] = (0.8, 0.7, 0.6, 0.004)
    return tf.reshape(1024)


@functools.lru_cache(maxsize=None)
def _composite_visit(name, cam_name, ert_mode, phong=False):
    vol = _volume(name)
    v = FM.Visit()
    _, n = Wt.render(vol, _faint_table() if phong else _opaque_table(), W, H, visit=v, ert_threshold=ERT_THRESHOLD, ert_mode=ert_mode, phong=phong, **_cam_kw(CAMS[cam_name]))
    assert n == len(v.samples())
    return v


@functools.lru_cache(maxsize=None)
def _iso_case(name, cam_name):
    """(level, iso_model's frame, the executed samples up to and including the hit, the six gradient positions of every hit)"""
    vol = _volume(name)
    cam = CAMS[cam_name]
    tf = np.zeros(1024, f32)
    mx = PM.render_cam(vol, tf, W, H, cam, PM.PROJ_MAX)
    reach = mx["index"][mx["n"] > 0]
    level = max(int(np.median(reach)), 1)                     # about half of the rays that cross the volume reach it
    iso = IM.render_cam(vol, tf, W, H, cam, level)
    R, inv_scale = _rays(_dims(vol), cam_name)
    ordinal = iso["hit"][R["y"], R["x"], 3].astype(np.int64)
    found = iso["index"][R["y"], R["x"]] >= level
    tex, _ = FM.reducer_samples(R, inv_scale, PM.march, np.where(found, ordinal, -1))
    assert len(tex) == iso["count"]
    share = found.sum() / max((mx["n"][R["y"], R["x"]] > 0).sum(), 1)
    assert 0.25 <= share <= 0.75, share
    t_hit = Wt._to_tex(iso["hit"][R["y"], R["x"], :3][found], inv_scale)
    grad = []
    for a, n in enumerate(_dims(vol)):
        h = f32(1) / f32(n)
        for s in (h, -h):
            g = t_hit.copy(); g[:, a] = t_hit[:, a] + s
            grad.append(g)
    return level, iso, tex, np.concatenate(grad)


@pytest.mark.parametrize("name", ("brain_u8", "brain_f32"))
def test_family_cases_are_real(name):
    """The composite case ends rays early -- strictly fewer samples and a strictly smaller brick set than the MIP frame, in both ERT modes --; the
    isosurface case stops about half of the rays; the Phong bracket is tight: its two bounds differ by less than a quarter of the lower one."""
    vol = _volume(name)
    dims = _dims(vol)
    for cam in ("oblique",):
        full = _mip_samples(dims, cam)
        for mode in (Wt.ERT_REFERENCE, Wt.ERT_TRUE):
            s = _composite_visit(name, cam, mode).samples()
            assert 0 < len(s) < len(full)
            a, b = FM.bricks(s, dims), FM.bricks(full, dims)
            assert FM.contains(b, a) and FM.bit_count(a) < FM.bit_count(b), (FM.bit_count(a), FM.bit_count(b))
        _, _, tex, grad = _iso_case(name, cam)
        assert 0 < len(tex) < len(full) and len(grad) > 0
        for layout in FAMILY_LAYOUTS:
            geom = _geom(vol, layout)
            bits = _line_bits(geom)
            (b_lo, l_lo), (b_hi, l_hi) = FM.phong_bounds(_composite_visit(name, cam, Wt.ERT_REFERENCE, True), layout, vol.dtype, geom, dims, bits)
            assert FM.contains(b_hi, b_lo) and FM.contains(l_hi, l_lo)
            for lo, hi in ((b_lo, b_hi), (l_lo, l_hi)):
                assert 0 < FM.bit_count(lo) and (FM.bit_count(hi) - FM.bit_count(lo)) * 4 < FM.bit_count(lo), (layout, FM.bit_count(lo), FM.bit_count(hi))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
GUARD_WORDS, GUARD = 4, 0x5A5A5A5A
PAIRS_LOG2 = 18


class _Instruments:
    """Device buffers for one instrumented frame: the brick bitmap, the line bitmap of `line_bits` bits, optionally the (block, line) table; each
    bitmap is followed by guard words that must come back untouched."""
    def __init__(self, dims, line_bits, pairs=False):
        import torch
        dev = torch.device("cuda", 0)
        self.bw, self.lw, self.line_bits = (FM.brick_bits(dims) + 31) // 32, (line_bits + 31) // 32, line_bits
        self.bricks = torch.full((self.bw + GUARD_WORDS,), GUARD, dtype=torch.int32, device=dev); self.bricks[:self.bw] = 0
        self.lines = torch.full((self.lw + GUARD_WORDS,), GUARD, dtype=torch.int32, device=dev); self.lines[:self.lw] = 0
        self.pairs = torch.zeros(1 << PAIRS_LOG2, dtype=torch.int64, device=dev) if pairs else None
        torch.cuda.synchronize()

    def options(self, lines_all=False, **kw):
        return vv.make_options(count_samples=True, touched_bricks=self.bricks.data_ptr(), touched_lines=self.lines.data_ptr(), touched_line_bits=self.line_bits,
                               touched_lines_all=lines_all, touched_block_lines=self.pairs.data_ptr() if self.pairs is not None else 0,
                               touched_block_lines_log2=PAIRS_LOG2 if self.pairs is not None else 0, **kw)

    def read(self):
        import torch
        torch.cuda.synchronize()
        b = self.bricks.cpu().numpy().view(np.uint32); l = self.lines.cpu().numpy().view(np.uint32)
        assert (b[self.bw:] == GUARD).all() and (l[self.lw:] == GUARD).all(), "guard words behind a bitmap were written"
        p = self.pairs.cpu().numpy().view(np.uint64) if self.pairs is not None else None
        return b[:self.bw].copy(), l[:self.lw].copy(), p


def _same_words(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(got)} words differ ({FM.bit_count(got)} bits set, {FM.bit_count(want)} expected), first word {int(bad[0])}: "
                           f"{int(got[bad[0]]):#010x} vs {int(want[bad[0]]):#010x}")


def _load(ctx, name, layout_name, tf=None):
    """Loads the volume (inside MO.knobs: the knobs of the case are read at the load)."""
    vol = _volume(name)
    ctx.load_volume(vol, np.zeros(1024, f32) if tf is None else tf)
    return vol


def _check_layout(ctx, layout_name, what):
    assert ctx.last_launch()["layout"] == LAYOUTS[layout_name][1], (what, ctx.last_launch())


@pytest.mark.gpu
@pytest.mark.parametrize("name,layout_name", CASES)
def test_copies_equal_pack(ctx, name, layout_name):
    """Every layout the case samples, read out of HBM, equals pack() byte for byte over the whole allocation -- halo voxels, clamped extra layers,
    clamped records and zero padding included.  Exempt, by formula (footprint_model.pair_padding): the one padding record that ends each row of a u8
    pair copy whose fast dimension is even, which no gather reads and the contract leaves unspecified."""
    knobs, code, _, cams, copies = LAYOUTS[layout_name]
    with MO.knobs(ctx, knobs):
        vol = _load(ctx, name, layout_name)
        ctx.render_mip(W, H, CAMS[cams[-1]])                                   # (builds the copy)
        _check_layout(ctx, layout_name, (name, layout_name))
        for read_code, model in copies:
            raw, g = ctx.read_layout(read_code)
            want_geom = _geom(vol, layout_name) if model == LAYOUTS[layout_name][2] else FM.dense_geom(model, vol.dtype, _dims(vol))
            slice_bytes = g["slice"] * 64 if model == "bricked" else g["slice"]
            assert (g["alloc_bytes"], g["row"], slice_bytes) == (want_geom["alloc"], want_geom["row"], want_geom["slice"]), (model, g, want_geom)
            assert (g["nx"], g["ny"], g["nz"]) == _dims(vol) and g["voxel_type"] == (vv.VOXEL_F32 if vol.dtype == np.float32 else vv.VOXEL_U8)
            want = FM.pack(vol, model, want_geom)
            care = np.ones(len(want), bool)
            for a, b in FM.pair_padding(model, vol.dtype, _dims(vol), want_geom):
                care[a:b] = False
            bad = np.flatnonzero((raw != want) & care)
            assert len(bad) == 0, f"{name} {model}: {len(bad)} bytes differ, first at {int(bad[0])}: {int(raw[bad[0]])} vs {int(want[bad[0]])}"
        # a layout that is not resident reports 0 bytes; bad arguments are errors
        if layout_name == "linear":
            assert ctx.read_layout(2)[1]["alloc_bytes"] == 0 and ctx.read_layout(2)[0].size == 0
            with pytest.raises(vv.VolvizError):
                ctx.read_layout(6)
            geom = np.zeros(8, np.uint64); small = np.zeros(16, np.uint8)
            assert ctx.lib.vv_debug_read_layout(ctx.h, 0, geom.ctypes.data, small.ctypes.data, small.size) == -1 and int(geom[0]) == len(raw)
            assert ctx.lib.vv_debug_read_layout(None, 0, geom.ctypes.data, small.ctypes.data, small.size) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("name,layout_name", CASES)
def test_mip_frame_instruments(ctx, name, layout_name):
    """A MIP frame's instruments on every layout, from every camera the layout serves: touched_bricks and the compulsory touched_lines equal the model
    word for word; the issued bitmap contains the compulsory one; the (block, line) table's distinct lines are exactly the issued bitmap's set bits, its
    block ids lie in 1..grid, and there are at least as many pairs as lines; under an odd touched_line_bits below the layout's size the bits below
    the limit equal the model's, nothing at or beyond it is set and the guard words stay untouched."""
    knobs, code, model, cams, _ = LAYOUTS[layout_name]
    vol = _volume(name)
    dims = _dims(vol)
    geom = _geom(vol, layout_name)
    bits = _line_bits(geom)
    with MO.knobs(ctx, knobs):
        _load(ctx, name, layout_name)
        for cam_name in cams:
            cam = CAMS[cam_name]
            what = f"{name} {layout_name} {cam_name}"
            tex = _mip_samples(dims, cam_name)
            want_bricks, want_lines = _expect(tex, vol, layout_name, bits)
            ins = _Instruments(dims, bits)
            ctx.render_mip(W, H, cam, options=ins.options())
            _check_layout(ctx, layout_name, what)
            assert ctx.last_sample_count() == len(tex), what
            got_bricks, got_lines, _ = ins.read()
            print(f"{what}: samples {len(tex)}, bricks {FM.bit_count(got_bricks)} / {FM.bit_count(want_bricks)} of {FM.brick_bits(dims)}, "
                  f"compulsory lines {FM.bit_count(got_lines)} / {FM.bit_count(want_lines)} of {geom['alloc'] // 128}")
            _same_words(got_bricks, want_bricks, what + ": touched_bricks")
            _same_words(got_lines, want_lines, what + ": touched_lines")
            # the issued set and the per-block table
            ins = _Instruments(dims, bits, pairs=True)
            ctx.render_mip(W, H, cam, options=ins.options(lines_all=True))
            _check_layout(ctx, layout_name, what)
            lay = ctx.last_launch()
            _, issued, table = ins.read()
            assert FM.contains(issued, want_lines), what + ": the issued set does not contain the compulsory one"
            keys = table[table != 0]
            assert len(keys) == len(np.unique(keys)) and len(keys) * 4 <= len(table), (what, len(keys))
            line_of, block_of = (keys & np.uint64((1 << 36) - 1)).astype(np.int64), (keys >> np.uint64(36)).astype(np.int64)
            _same_words(FM._words(np.unique(line_of), bits), issued, what + ": lines of touched_block_lines against the issued bitmap")
            assert line_of.max() < bits
            blk_w, blk_h = 1 << lay["blk_log2w"], 256 >> lay["blk_log2w"]
            grid = (-(-H // blk_h) + 7) // 8 * 8 * -(-W // blk_w)              # vv_tiles.h grid_blocks: whole rounds of 8 strips of blocks
            print(f"{what}: issued lines {FM.bit_count(issued)}, pairs {len(keys)}, blocks {len(np.unique(block_of))}, highest block id {int(block_of.max())} of {grid}")
            assert block_of.min() >= 1 and block_of.max() <= grid, (what, int(block_of.min()), int(block_of.max()), grid)
            assert len(keys) >= FM.bit_count(issued)
            # an odd limit inside the layout
            limit = int(np.median(FM.line_numbers(tex, model, vol.dtype, geom, dims))) | 1     # (half of the touched lines lie below it)
            ins = _Instruments(dims, limit)
            ctx.render_mip(W, H, cam, options=ins.options())
            _, clipped, _ = ins.read()
            want_clipped = FM.lines(tex, model, vol.dtype, geom, dims, limit)
            assert 0 < FM.bit_count(want_clipped) < FM.bit_count(want_lines)
            _same_words(clipped, want_clipped, what + f": touched_lines under touched_line_bits = {limit}")


def _family_frame(ctx, kind, cam, ins, **kw):
    """One instrumented frame of a kernel family into scratch images; returns the family code vv_debug_last_launch must report."""
    o = ins.options(**kw.pop("okw", {}))
    if kind == "mip":
        ctx.render_mip(W, H, cam, options=o); return 2
    if kind in ("composite", "phong"):
        ctx.render(W, H, cam, phong=kind == "phong", options=o); return int(kind == "phong")
    if kind == "iso":
        ctx.render_iso(W, H, cam, kw["level"], options=o); return 3
    ctx.render_projection(W, H, cam, kw["mode"], options=o); return 4


@pytest.mark.gpu
@pytest.mark.parametrize("layout_name", FAMILY_LAYOUTS)
@pytest.mark.parametrize("name", ("brain_u8", "brain_f32"))
def test_other_families_instruments(ctx, name, layout_name):
    """The other kernel families on the linear, the bricked and the z-pair layout, oblique camera.  A transparent composite and the MIN / MEAN projections
    mark what the MIP frame marks.  An opaque composite that ends rays early marks the witness's executed samples, in both ERT modes.  An isosurface frame
    marks the samples up to and including the hit; its six gradient gathers mark nothing under touched_lines_all = 0 and are present under 1.  A Phong
    frame lies between the model of its executed samples and that of every entry 1..30 of the chunks its rays begin."""
    knobs, code, model, _, _ = LAYOUTS[layout_name]
    cam_name = "oblique"
    cam = CAMS[cam_name]
    vol = _volume(name)
    dims = _dims(vol)
    geom = _geom(vol, layout_name)
    bits = _line_bits(geom)
    mip_want = _expect(_mip_samples(dims, cam_name), vol, layout_name, bits)

    def frame(kind, what, lines_all=False, tf=None, **kw):
        if tf is not None:
            ctx.set_transfer_function(tf)
        ins = _Instruments(dims, bits)
        okw = dict(kw.pop("okw", {}), lines_all=lines_all)
        family = _family_frame(ctx, kind, cam, ins, okw=okw, **kw)
        lay = ctx.last_launch()
        assert lay["layout"] == code and lay["phong"] == family, (what, lay)
        b, l, _ = ins.read()
        return b, l, ctx.last_sample_count()

    with MO.knobs(ctx, knobs):
        _load(ctx, name, layout_name)
        # transparent composite, MIN and MEAN projections: the MIP frame's bitmaps
        for kind, kw in (("composite", dict(okw=dict(ert_threshold=2.0))), ("proj", dict(mode=vv.PROJ_MIN)), ("proj", dict(mode=vv.PROJ_MEAN)), ("mip", {})):
            what = f"{name} {layout_name} {kind} {kw}"
            b, l, n = frame(kind, what, tf=np.zeros(1024, f32), **kw)
            assert n == len(_mip_samples(dims, cam_name)), what
            _same_words(b, mip_want[0], what + ": touched_bricks"); _same_words(l, mip_want[1], what + ": touched_lines")
        # opaque composite: rays end early
        for mode in (vv.ERT_REFERENCE, vv.ERT_TRUE):
            what = f"{name} {layout_name} opaque composite ert_mode {mode}"
            tex = _composite_visit(name, cam_name, mode).samples()
            want = _expect(tex, vol, layout_name, bits)
            b, l, n = frame("composite", what, tf=_opaque_table(), okw=dict(ert_threshold=ERT_THRESHOLD, ert_mode=mode))
            print(f"{what}: samples {n} / {len(tex)}, bricks {FM.bit_count(b)} / {FM.bit_count(want[0])}, lines {FM.bit_count(l)} / {FM.bit_count(want[1])}")
            assert n == len(tex), what
            _same_words(b, want[0], what + ": touched_bricks"); _same_words(l, want[1], what + ": touched_lines")
        # isosurface
        level, iso, tex, grad = _iso_case(name, cam_name)
        what = f"{name} {layout_name} iso level {level}"
        want = _expect(tex, vol, layout_name, bits)
        b, l, n = frame("iso", what, level=level)
        print(f"{what}: samples {n} / {len(tex)}, bricks {FM.bit_count(b)} / {FM.bit_count(want[0])}, lines {FM.bit_count(l)} / {FM.bit_count(want[1])}")
        assert n == len(tex) == iso["count"], what
        _same_words(b, want[0], what + ": touched_bricks"); _same_words(l, want[1], what + ": touched_lines (the gradient gathers mark nothing)")
        grad_lines = FM._words(FM.line_numbers(grad, model, vol.dtype, geom, dims), bits)      # (positions outside the volume are gathered too, but their lines are not modelled)
        assert np.any(grad_lines & ~want[1]), what + ": the gradient positions add no line: the case shows nothing"
        b, l, n = frame("iso", what, lines_all=True, level=level)
        assert FM.contains(l, want[1]) and FM.contains(l, grad_lines), what + ": issued set without the gradient gathers' lines"
        # Phong
        what = f"{name} {layout_name} phong"
        visit = _composite_visit(name, cam_name, Wt.ERT_REFERENCE, True)
        lo, hi = FM.phong_bounds(visit, model, vol.dtype, geom, dims, bits)
        b, l, n = frame("phong", what, tf=_faint_table(), okw=dict(ert_threshold=ERT_THRESHOLD))
        print(f"{what}: samples {n} / {len(visit.samples())}, bricks {FM.bit_count(lo[0])} <= {FM.bit_count(b)} <= {FM.bit_count(hi[0])}, "
              f"lines {FM.bit_count(lo[1])} <= {FM.bit_count(l)} <= {FM.bit_count(hi[1])}")
        assert n == len(visit.samples()), what
        assert FM.contains(b, lo[0]) and FM.contains(hi[0], b), what + ": touched_bricks outside the bracket"
        assert FM.contains(l, lo[1]) and FM.contains(hi[1], l), what + ": touched_lines outside the bracket"


@pytest.mark.gpu
@pytest.mark.parametrize("rows_kw", [dict(shard=(4, 2, 1)), dict(slab_rows=(2, 5))], ids=["shard-1-of-2", "slab-rows-2-4"])
def test_only_owned_rows_are_marked(ctx, rows_kw):
    """A sharded frame (shard_count = 2, bands of 4 slab rows) and one with slab_row_begin / _end mark the samples of the rows they own only: the model
    over those rays, exactly, and strictly less than the whole frame's.  48 x 120 pixels: 9 slab rows, of which the shard owns 4..7."""
    name, layout_name, cam_name, size = "brain_f32", "bricked", "oblique", (48, 120)
    knobs, code, model, _, _ = LAYOUTS[layout_name]
    vol = _volume(name)
    dims = _dims(vol)
    geom = _geom(vol, layout_name)
    bits = _line_bits(geom)
    tex = _mip_samples(dims, cam_name, None, rows_kw.get("slab_rows", (0, 0)), rows_kw.get("shard"), size)
    whole = _expect(_mip_samples(dims, cam_name, size=size), vol, layout_name, bits)
    want = _expect(tex, vol, layout_name, bits)
    assert 0 < FM.bit_count(want[0]) < FM.bit_count(whole[0]) and 0 < FM.bit_count(want[1]) < FM.bit_count(whole[1])
    with MO.knobs(ctx, knobs):
        _load(ctx, name, layout_name)
        ins = _Instruments(dims, bits)
        ctx.render_mip(size[0], size[1], CAMS[cam_name], options=ins.options(**rows_kw))
        _check_layout(ctx, layout_name, rows_kw)
        assert ctx.last_sample_count() == len(tex)
        b, l, _ = ins.read()
        print(f"{rows_kw}: samples {len(tex)}, bricks {FM.bit_count(b)} / {FM.bit_count(want[0])} (whole frame {FM.bit_count(whole[0])}), lines {FM.bit_count(l)} / {FM.bit_count(want[1])} ({FM.bit_count(whole[1])})")
        _same_words(b, want[0], f"{rows_kw}: touched_bricks"); _same_words(l, want[1], f"{rows_kw}: touched_lines")
