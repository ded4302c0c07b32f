"""Every kernel family held to its host model where the addressing changes: volumes whose sampled layout passes 2^32 bytes (64-bit slice bases), volumes
whose 32-bit offsets reach [2^31, 2^32) (the band a sign extension would break), u8 pair copies at the top of their 32-bit range and just beyond it
(refused), and three-slice volumes whose slice pitch lies at and just below 2^24 bytes (the second clause of VolumeView::big, which protects the 24-bit
multiply of the slice index).  Noise volumes (`_noise_parts`): a voxel read from the wrong address almost surely differs.  Every comparison is exact.

  volume             shape, type             what it is for                                            limit   builds forced (layout code unshaded / Phong)
  f32_above          1280^3 f32, 8.4 GB      f32 beyond 4 GiB (rows of 5 KiB: re-pitched)              2^32    linear 1/1, bricked 2/2, z-pair 3/3, z-fastest 4/4
  u8_above           1792 x 1792 x 2304 u8   u8 beyond 4 GiB and 2^32 voxels; pair copies refused      2^32    linear 1/1, bricked 2/2, z-fastest 4/4; z-pair -> 1/1, x-pair -> 4/4
  f32_band           960^3 f32, 3.5 GB       32-bit offsets in [2^31, 2^32)                            2^31    linear 0/1, bricked 2/2, z-pair 3/3, z-fastest 4/4
  u8_pair_refused    1536^3 u8, 3.6 GB       pair copies would pass 4 GiB: refused, next layout        2^31    linear 0/1, bricked 2/2, z-fastest 4/4; z-pair -> 0/1, x-pair -> 4/4
  thin_{at,below}    1000 x 4195|4194 x 3    slice pitch 16 780 000 / 16 776 000 bytes around 2^24     2^24    linear 1/1 | 0/0, bricked, z-pair, z-fastest, x-pair 5/4
    _{f32,u8}        (u8: 4000 voxels a row)
  u8_pair_top        1280^3 u8, 2.1 GB       pair copies of 4.2 GB: offsets up to the top of 32 bits   2^31    z-pair 3/3, x-pair 5/4, bricked 2/2 (its linear layout ends below
                                                                                                               2^31: the slice, slab and histogram kernels have nothing to show on it)

What keeps a comparison from passing vacuously is computed from the models alone, before the kernel runs (`_decided`, `_crossing`): the voxel that
decides each compared pixel -- the isosurface hit's position, the sample whose ordinal the projection record names (the MIP frame: the same sample), the
slice pixel's own position -- and hence its offset in the sampled layout; at least 10 % of the compared pixels are decided beyond the limit, 10 % below it,
and they hold at least 20 distinct values.  Mean projections and composited frames cross the whole volume: at least 30 % of their samples lie beyond the
limit.  The shares are taken over the images a family compares on one build (two cameras: one enters the volume at high z and x, the other at low
addresses).  Offsets: exact in the linear layout; in a copy, whose order follows z (bricked, z-pair) or x (z-fastest, x-pair), proportional along that axis.

The volume-to-volume families (derive, stencil, resample, label and mask; helpers in addressing_volumes.py) read the linear layout only and are held three ways:

  test                                         what it runs                                                              what a bug would be
  test_derive / _stencil / _resample /         the histogram's four boxes on every volume but u8_pair_top: below the     a source address formed in 32 bits, sign-extended,
    _label_and_mask                            limit, across it inside a row, across it over a slice boundary, ending   or with a 24-bit multiply of the slice index
                                               at the last voxel; device output with guard bytes, host path once
  test_volume_outputs_beyond_4_gib             f32_above, u8_above: the whole volume derived, filtered, resampled into   an output offset (`dst`, `first` / `plane`, `at`)
                                               8.4 / 7.4 GB; three slabs against the models, the copying calls against   or a grid-stride item counter in 32 bits
                                               the regenerated source byte for byte; grid caps of 4096 blocks
  test_label_box_of_more_than_2_to_31_voxels   2047 x 2049 x 1023 u8, sparse foreground, against a sparse model that     a signed compare, atomicMin or division of a
                                               the CPU half ties to label_model; then a mask into 17 GB of f32           voxel index; `i0 * 4` in 32 bits

The voxel that decides an output voxel of a straddling box is the source voxel (label and mask), the cell's first voxel (derive), the centre voxel
(stencil), the lower corner of the sample position (resample); the same thresholds hold over the two straddling boxes together, with 20 distinct labels
under connectivity 6 (under 26 a foreground share of 0.3 ... 0.6 is one component almost surely: there the records compared, label, size and masked
voxel, are what is distinct).  The rotation of the resampled boxes leaves the box's centre where it is: vv_resample_matrix's `centre` is where the grid's
centre lands, so it is handed c + A (1/2 - c).  The mask's `fill` is in storage units (rule M2): 0.25 on a u8 volume is 0.25 / 255 in an f32 output.

The CPU half holds the same conditions for the thin volumes and shows once that the models notice the bugs this module is for (a slice pitch multiplied
in 24 bits; an offset taken modulo 2^32; one sign-extended from 32 bits): profiles/addressing_sensitivity.txt.  For every volume it asserts the boxes'
properties and the shares from the layout alone, and it ties the sparse label model to label_model on the wide box's structures at 63 x 41 x 39."""
import functools
import os
import re
import time
from types import SimpleNamespace

import numpy as np
import pytest

import addressing_volumes as AV
import hist_model as HM
import iso_model as IM
import label_model as LM
import mip_oracle as MO
import oracle_lib as O
import proj_model as PM
import slab_model as SM
import volume_out as VO
import volviz_amd as vv
import witness as Wt

f32 = np.float32
REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FILL = 0x5A
SEED = 11
W, H, STEP = 99, 71, 1 / 64                                     # the MIP, isosurface and projection frames
CW, CH, CSTEP, CBAND = 200, 113, 1 / 128, (3, 5)                # the composited frames: slab rows 3 and 4 of 9 (the image centre)
CAM_HI = vv.Camera.orbit(3.0, 1.0, 0.6)                         # (2.08, 1.62, 1.43): rays enter at high x, y and z
CAM_LO = vv.Camera.orbit(3.0, np.pi - 1.0, 0.6 + np.pi)         # the opposite corner: rays enter at low addresses
CAMS = (("hi", CAM_HI), ("lo", CAM_LO))
LEVEL_NEAR = 128                                                # the noise's median: hits among a ray's first samples
WIDE_FG = 200                                                   # the wide label box: foreground byte on a background of 0 (test_label.py's FG)

# build -> (knobs, vv_prepare_layouts bit, the copies it samples (vv_layout_state), the axis its offsets follow: 2 = z, 0 = x)
BUILDS = {
    "linear":  ({"VV_BRICKED": "0", "VV_ZPAIR": "0", "VV_ZFAST": "0"}, 0, (), 2),
    "bricked": ({"VV_BRICKED": "1", "VV_ZFAST": "0"}, vv.LAYOUT_BRICKED, ("bricked",), 2),
    "zpair":   ({"VV_BRICKED": "0", "VV_ZPAIR": "1", "VV_ZFAST": "0"}, vv.LAYOUT_ZPAIR, ("zpair",), 2),
    "zfast":   ({"VV_ZFAST": "1", "VV_ZPAIR": "0"}, vv.LAYOUT_ZFAST, ("zfast",), 0),
    "xpair":   ({"VV_ZFAST": "1"}, vv.LAYOUT_ZFAST, ("zfast", "xpair"), 0),
}
LIN_BIG, LIN_32, LIN_32_PHONG_BIG = (1, 1), (0, 0), (0, 1)      # (Phong frames of volumes beyond 1 GiB take the 64-bit build by policy)


def _spec(dims, dtype, limit, linear, builds, refused=()):
    """builds: build -> (layout code unshaded, layout code Phong); refused: the copies vv_layout_state must report absent after they were asked for."""
    return SimpleNamespace(dims=dims, dtype=dtype, limit=limit, big=linear[0] == 1, builds=dict(linear=linear, **builds), refused=refused)


_COPIES = dict(bricked=(2, 2), zpair=(3, 3), zfast=(4, 4))
_THIN = dict(_COPIES, xpair=(5, 4))
SPECS = {
    "thin_at_f32":     _spec((1000, 4195, 3), "f32", 1 << 24, LIN_BIG, _THIN),
    "thin_below_f32":  _spec((1000, 4194, 3), "f32", 1 << 24, LIN_32, _THIN),
    "thin_at_u8":      _spec((4000, 4195, 3), "u8", 1 << 24, LIN_BIG, _THIN),
    "thin_below_u8":   _spec((4000, 4194, 3), "u8", 1 << 24, LIN_32, _THIN),
    "f32_band":        _spec((960, 960, 960), "f32", 1 << 31, LIN_32_PHONG_BIG, _COPIES),
    "u8_pair_refused": _spec((1536, 1536, 1536), "u8", 1 << 31, LIN_32_PHONG_BIG, dict(bricked=(2, 2), zfast=(4, 4), zpair=LIN_32_PHONG_BIG, xpair=(4, 4)), ("zpair", "xpair")),
    "f32_above":       _spec((1280, 1280, 1280), "f32", 1 << 32, LIN_BIG, _COPIES),
    "u8_above":        _spec((1792, 1792, 2304), "u8", 1 << 32, LIN_BIG, dict(bricked=(2, 2), zfast=(4, 4), zpair=LIN_BIG, xpair=(4, 4)), ("zpair", "xpair")),
    "u8_pair_top":     _spec((1280, 1280, 1280), "u8", 1 << 31, LIN_32_PHONG_BIG, dict(bricked=(2, 2), zpair=(3, 3), xpair=(5, 4))),
}
SPECS["u8_pair_top"].builds.pop("linear")                       # 2.1 GB: its linear layout ends below 2^31
NAMES = list(SPECS)
LINEAR_NAMES = NAMES[:-1]                                       # the volumes whose linear layout passes their limit (the same order: one load per volume)
THIN = NAMES[:4]


# ---------------------------------------------------------------------------------------------------------------------
# the models' side: rays, deciding voxels, shares
# ---------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _voxel(t, n):
    """The lower texel of texture coordinate t on an axis of n voxels."""
    return np.clip(np.floor(np.nan_to_num(np.asarray(t, np.float64)) * n - 0.5), 0, n - 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _rays(w, h, cam_name, step):
    """The owned rays of a frame as the models set them up (witness.py): a dict of flat arrays."""
    cam = dict(CAMS)[cam_name]
    R = Wt.frame_rays(w, h)
    front, back = Wt.analytic_endpoints(w, h, R["x"], R["y"], cam.origin, cam.look(), cam.up, cam.fov_y, cam.scale)
    Wt.setup(R, front, back, cam.origin, np.full(3, step, f32), Wt.SLICE_NONE, (.5, .5, .5, 0, 0, 1))
    return {k: v[R["owned"]] for k, v in R.items()}


def _sample_positions(R, ordinal, chunk):
    """Cube-space position [n, 3] of each ray's `ordinal`-th executed sample (1-based; chunks of `chunk` samples restart from origin + dir * dist)."""
    o = np.asarray(ordinal, np.int64) - 1
    d = R["dist0"].astype(np.float64) + (o // chunk) * chunk * R["sstep"].astype(np.float64)
    return R["origin"] + R["dir"] * d[:, None] + R["sdir"] * ((o % chunk) + 1)[:, None]


def _decided(coord, first_beyond, records, what):
    """Section 3 of the module's contract for pixels decided by one voxel: `coord` their voxel index along the layout's axis, `records` what is compared there."""
    coord = np.asarray(coord); records = np.asarray(records).reshape(len(coord), -1)
    assert len(coord) >= 200, f"{what}: {len(coord)} decided pixels only"
    beyond = coord >= first_beyond
    share = float(beyond.mean())
    distinct = len(np.unique(records[beyond], axis=0)) if beyond.any() else 0
    assert 0.10 <= share <= 0.90, f"{what}: {share:.3f} of the compared pixels are decided beyond the limit"
    assert distinct >= 20 and len(np.unique(records[~beyond], axis=0)) >= 20, f"{what}: {distinct} distinct values beyond the limit"
    return share, distinct


def _crossing(dims, axis, first_beyond, cams_e, w, h, step, chunk, what):
    """... for frames whose rays cross the whole volume: the share of the executed samples inside the volume that lie beyond the limit.
    cams_e: (camera name, executed samples per pixel [h, w]) per compared image."""
    inside = beyond = 0
    for cam_name, e in cams_e:
        R = _rays(w, h, cam_name, step)
        n = e[R["y"], R["x"]]
        for k in range(1, int(n.max()) + 1):
            p = _sample_positions(R, np.full(len(n), k), chunk)
            ok = (k <= n) & np.all((p >= 0) & (p < 1), axis=-1)
            inside += int(ok.sum())
            beyond += int((ok & (_voxel(p[:, axis], dims[axis]) >= first_beyond)).sum())
    share = beyond / max(inside, 1)
    assert inside >= 10000 and share >= 0.30, f"{what}: {share:.3f} of {inside} samples lie beyond the limit"
    return share


def _high_level(M):
    """An isosurface level most rays reach only deep inside: the 30th percentile of the frame's maxima."""
    return int(np.percentile(M[M > 0], 30))


class Models:
    """The host models of one volume, each computed once and shared by the tests and builds that need it."""

    def __init__(self, host, tf):
        self.host, self.tf, self.dims = host, tf, host.shape[::-1]
        self.cache = {}

    def get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def proj(self, cam_name, mode):
        return self.get(("proj", cam_name, mode), lambda: PM.render_cam(self.host, self.tf, W, H, dict(CAMS)[cam_name], mode, step=STEP, fill=FILL))

    def mip(self, cam_name):
        cam = dict(CAMS)[cam_name]
        return self.get(("mip", cam_name), lambda: (MO.sweep(self.host, W, H, cam, options_kw=dict(step=STEP)),
                                                    MO.written_mask(self.host, W, H, cam, options=vv.make_options(step=STEP)),
                                                    MO.executed_samples(self.host, W, H, cam, options_kw=dict(step=STEP))))

    def iso(self, cam_name, level):
        return self.get(("iso", cam_name, level), lambda: IM.render_cam(self.host, self.tf, W, H, dict(CAMS)[cam_name], level, step=STEP, fill=FILL))

    def levels(self):
        return LEVEL_NEAR, _high_level(np.where(self.proj("hi", PM.PROJ_MAX)["written"], self.proj("hi", PM.PROJ_MAX)["index"], 0))

    def composite(self, cam_name, phong):
        def make():
            want = np.zeros((CH, CW, 4), np.uint8)
            _, n = O.render(self.host, self.tf, CW, CH, dict(CAMS)[cam_name], phong=phong, options=vv.make_options(step=CSTEP, slab_rows=CBAND), out=want)
            return want, n
        return self.get(("composite", cam_name, phong), make)

    # ---- the conditions of one family on one layout (axis, first voxel index beyond the limit) ----
    def extremum_condition(self, mode, axis, first_beyond, what):
        """MAX / MIN (and the MIP frame, whose maximum is PROJ_MAX's): the sample the record's ordinal names."""
        coord, rec = [], []
        for cam_name, _ in CAMS:
            m = self.proj(cam_name, mode)
            R = _rays(W, H, cam_name, STEP)
            stat = m["stat"][R["y"], R["x"]]
            ok = stat[:, 1] > 0
            p = _sample_positions({k: v[ok] for k, v in R.items()}, stat[ok, 0], PM.SAMPLES)
            coord.append(_voxel(p[:, axis], self.dims[axis])); rec.append(np.column_stack([stat[ok], m["index"][R["y"], R["x"]][ok]]))
        return _decided(np.concatenate(coord), first_beyond, np.concatenate(rec), what)

    def crossing_condition(self, axis, first_beyond, what):
        return _crossing(self.dims, axis, first_beyond, [(c, self.proj(c, PM.PROJ_MEAN)["e"]) for c, _ in CAMS], W, H, STEP, PM.SAMPLES, what)

    def iso_condition(self, level, axis, first_beyond, what):
        coord, rec = [], []
        for cam_name, _ in CAMS:
            m = self.iso(cam_name, level)
            ok = m["written"] & (m["hit"][..., 3] > 0)
            coord.append(_voxel(m["hit"][ok][:, axis], self.dims[axis])); rec.append(m["hit"][ok].view(np.uint32))
        return _decided(np.concatenate(coord), first_beyond, np.concatenate(rec), what)

    def composite_condition(self, axis, first_beyond, what):
        """Every sample of the band's rays between the ray's ends (early termination only shortens a ray that entered on the side named by its camera)."""
        rows = slice(CBAND[0] * 14, CBAND[1] * 14)
        cams_e = []
        for cam_name, _ in CAMS:
            R = _rays(CW, CH, cam_name, CSTEP)
            e = np.zeros((CH, CW), np.int64)
            with np.errstate(all="ignore"):
                n = np.where(R["dead"], 0, np.ceil((R["upper"] - R["dist0"]) / R["sstep"])).astype(np.int64)
            e[R["y"], R["x"]] = np.where((R["y"] >= rows.start) & (R["y"] < rows.stop), n, 0)
            cams_e.append((cam_name, e))
        return _crossing(self.dims, axis, first_beyond, cams_e, CW, CH, CSTEP, Wt.CHUNK, what)


# ---- slices and slabs: the images compared, and each pixel's own position ----
FREE_FORM = (0.3, 0.3, 0.3, 0.4, -0.7, 1.1)
SLICES = (("sagittal-high", vv.SAGITTAL, (0.0, 0.0, 0.93)), ("sagittal-low", vv.SAGITTAL, (0.0, 0.0, 0.2)), ("coronal", vv.CORONAL, (0.97, 0.0, 0.0)),
          ("horizontal", vv.HORIZONTAL, (0.0, 0.99, 0.0)), ("free", None, None))
SH, SW = 96, 96
SLAB_K, SLAB_THICK = 7, 0.04                                    # 7 samples: one group of four and a remainder of three


def _slice_coords(view):
    """Texture coordinates [SH, SW, 3] of the pixels of one slice image (witness.slice_canonical / slice_advanced at scale 1) and which lie inside."""
    _, orient, d = view
    u = (np.arange(SW, dtype=f32) / f32(SW))[None, :] + np.zeros((SH, 1), f32)
    w = (np.arange(SH, dtype=f32) / f32(SH))[:, None] + np.zeros((1, SW), f32)
    zero = np.zeros((SH, SW), f32)
    if orient is None:
        t = O.slice_matrix(*FREE_FORM).reshape(16)
        p = np.stack([t[4 * r] * u + t[4 * r + 1] * w + t[4 * r + 2] * f32(0.5) + t[4 * r + 3] for r in range(3)], axis=-1)
    else:
        pos = {vv.SAGITTAL: [u, w, zero], vv.HORIZONTAL: [w, zero, u], vv.CORONAL: [zero, w, u]}[orient]
        p = np.stack([pos[c] + f32(d[c]) for c in range(3)], axis=-1)
    return p, Wt._in_bounds(p)


def _slice_condition(host, images, first_beyond_z, what):
    """images: (view, the model's image [SH * SW]) per compared image; each pixel is decided at its own position."""
    coord, rec = [], []
    for view, img in images:
        p, ok = _slice_coords(view)
        vals = np.asarray(img).reshape(SH, SW)[ok]                 # (SH == SW: the buffer's stride is the image's)
        assert len(np.unique(vals)) >= 20, f"{what} {view[0]}: a flat image"
        coord.append(_voxel(p[ok][:, 2], host.shape[0])); rec.append(vals.view(np.uint32))
    return _decided(np.concatenate(coord), first_beyond_z, np.concatenate(rec), what)


def _slice_images(host, filt):
    out = []
    for view in SLICES:
        _, orient, d = view
        img = O.slice_advanced(host, SH, SW, O.slice_matrix(*FREE_FORM), filter=filt, fill=-1.0) if orient is None else \
            O.slice(host, SH, SW, *d, orientation=orient, filter=filt, fill=-1.0)
        out.append((view, img))
    return out


def _slab_images(host, filt, mode):
    out = []
    for view in SLICES:
        _, orient, d = view
        pair = SM.slab_advanced(host, SH, SW, O.slice_matrix(*FREE_FORM), mode, SLAB_K, SLAB_THICK, filt=filt) if orient is None else \
            SM.slab_canonical(host, SH, SW, *d, orient, mode, SLAB_K, SLAB_THICK, filt=filt)
        out.append((view, pair))
    return out


def _first_beyond_linear(limit, slice_bytes):
    """The first slice most of which lies beyond `limit` in a linear layout of this slice pitch ((z + 1/2) * pitch >= limit)."""
    return max(-(-(2 * limit - slice_bytes) // (2 * slice_bytes)), 0)


def _first_beyond(limit, layout_bytes, n):
    """... in a copy of `layout_bytes` whose order follows an axis of n voxels: proportional."""
    return -(-limit * n // layout_bytes)


# ---------------------------------------------------------------------------------------------------------------------
# CPU half: the thin volumes' preconditions, and the sensitivity of the models to the bugs this module is for
# ---------------------------------------------------------------------------------------------------------------------
def _noise_parts(dims):
    """(z0, z1, seed) of the noise volumes a volume is made of.  The generator hashes the voxel's linear index as a 32-bit number: a volume of more
    than 2^32 voxels would repeat itself after 2^32 of them, and a u8 voxel read through an offset taken modulo 2^32 would hold the right value.  Such a
    volume is therefore two volumes of different seeds, one behind the other in z (profiles/addressing_sensitivity.txt shows that this is noticed)."""
    nx, ny, nz = dims
    if nx * ny * nz <= 1 << 32:
        return [(0, nz, SEED)]
    assert nx * ny * (nz // 2) <= 1 << 32
    return [(0, nz // 2, SEED), (nz // 2, nz, SEED + 1)]


def _host_noise(name):
    s = SPECS[name]
    nx, ny, nz = s.dims
    v = np.empty((nz, ny, nx), np.uint8)
    for z0, z1, seed in _noise_parts(s.dims):
        v[z0:z1] = O.noise_u8(nx, ny, z1 - z0, seed)            # == vv_generate_noise_u8 (test_noise_generator_matches_oracle)
    if s.dtype == "f32":
        v = v.astype(f32) / f32(255)                            # == vv_promote_u8_to_f32
    return np.ascontiguousarray(v)


@functools.lru_cache(maxsize=None)
def _thin_models(name):
    return Models(_host_noise(name), _table())


def _table(seed=7):
    """Colours outside [0, 1] too (the conversions clamp); opacities small enough that the composited rays cross the volume."""
    tf = np.random.default_rng(seed).uniform(-0.3, 1.4, 1024).astype(f32)
    tf[3::4] *= f32(0.03)
    return tf


def _dense_slice_bytes(name):
    s = SPECS[name]
    return s.dims[0] * s.dims[1] * (4 if s.dtype == "f32" else 1)


def _ray_family_conditions(models, axis, first_beyond, what, composite=True):
    out = {}
    for mode, mname in ((PM.PROJ_MAX, "max / mip"), (PM.PROJ_MIN, "min")):
        out[mname] = models.extremum_condition(mode, axis, first_beyond, f"{what} {mname}")
    out["mean"] = models.crossing_condition(axis, first_beyond, f"{what} mean")
    for level in models.levels():
        out[f"iso {level}"] = models.iso_condition(level, axis, first_beyond, f"{what} iso level {level}")
    if composite:
        out["composite"] = models.composite_condition(axis, first_beyond, f"{what} composite")
    return out


@pytest.mark.parametrize("name", THIN)
def test_thin_volume_preconditions(name):
    """The slice pitch lies where the name says, and the linear layout's conditions hold from the models alone."""
    s = SPECS[name]
    pitch = _dense_slice_bytes(name)
    assert (pitch >= 1 << 24) == s.big and abs(pitch - (1 << 24)) < 4096 and s.dims[2] == 3
    M = _thin_models(name)
    first = _first_beyond_linear(s.limit, pitch)
    assert first == 1                                           # slices 1 and 2 of 3: at 2^24, the other one 1216 bytes below it
    print(name, _ray_family_conditions(M, 2, first, name))
    for filt in (vv.FILTER_TEX8, vv.FILTER_EXACT):
        print(name, filt, _slice_condition(M.host, _slice_images(M.host, filt), first, f"{name} slices filter {filt}"))
        for mode in SM.MODES:
            _slice_condition(M.host, [(v, pair[0]) for v, pair in _slab_images(M.host, filt, mode)], first, f"{name} slabs mode {mode} filter {filt}")


def _misread(host, pitch_of, offset_of, pitches=None):
    """The volume a kernel would see whose byte offset of voxel (z, y, x) is offset_of(z * pitch_of(slice pitch) + y * row + x * size): offsets that
    fall outside the volume read 0.  pitches: (row, slice) pitch in bytes of a re-pitched layout (its padding holds zeros); None: the dense one."""
    nz, ny, nx = host.shape
    size = host.itemsize
    row, slice_bytes = pitches or (nx * size, ny * nx * size)
    flat, out = host.ravel(), np.empty(host.shape, host.dtype)
    in_slice = (np.arange(ny, dtype=np.int64)[:, None] * row + np.arange(nx, dtype=np.int64)[None, :] * size).ravel()
    for z in range(nz):                                         # (a slice at a time: the volumes of several GB too)
        off = offset_of(z * pitch_of(slice_bytes) + in_slice)
        sz, rem = np.divmod(off, slice_bytes)
        sy, sx = np.divmod(rem, row)
        sx //= size
        ok = (off >= 0) & (sz < nz) & (sy < ny) & (sx < nx)
        out[z] = np.where(ok, flat[np.where(ok, (sz * ny + sy) * nx + sx, 0)], host.dtype.type(0)).reshape(ny, nx)
    return out


def _differing(a, b, mask=None):
    d = np.asarray(a) != np.asarray(b)
    d = d.reshape(d.shape[0], d.shape[1], -1).any(axis=-1) if d.ndim > 2 else d
    return int(d[mask].sum() if mask is not None else d.sum()), int(mask.sum() if mask is not None else d.size)


def _sensitivity(name, bug, good, bad):
    """Per image kind: on how many compared pixels the models of the misread volume differ from those of the volume."""
    rows = []
    for cam_name, _ in CAMS:
        for mode, mname in ((PM.PROJ_MAX, "max"), (PM.PROJ_MIN, "min"), (PM.PROJ_MEAN, "mean")):
            a, b = good.proj(cam_name, mode), bad.proj(cam_name, mode)
            rows.append((f"projection {mname} record, camera {cam_name}",) + _differing(a["stat"], b["stat"], a["written"]))
        a, b = good.proj(cam_name, PM.PROJ_MAX), bad.proj(cam_name, PM.PROJ_MAX)
        rows.append((f"mip index, camera {cam_name}",) + _differing(a["index"], b["index"], a["written"]))
        for level in good.levels():
            a, b = good.iso(cam_name, level), bad.iso(cam_name, level)
            rows.append((f"iso level {level} hit record, camera {cam_name}",) + _differing(a["hit"].view(np.uint32), b["hit"].view(np.uint32), a["written"]))
        for phong in (False, True):
            a, b = good.composite(cam_name, phong)[0], bad.composite(cam_name, phong)[0]
            band = np.zeros((CH, CW), bool); band[CBAND[0] * 14:CBAND[1] * 14, :CW - 1] = True
            rows.append((f"composite{' phong' if phong else ''} rgba, camera {cam_name}",) + _differing(a, b, band))
    for (view, a), (_, b) in zip(_slice_images(good.host, vv.FILTER_TEX8), _slice_images(bad.host, vv.FILTER_TEX8)):
        rows.append((f"slice {view[0]}",) + _differing(a.view(np.uint32), b.view(np.uint32), _slice_coords(view)[1].ravel()))
    for (view, a), (_, b) in zip(_slab_images(good.host, vv.FILTER_TEX8, SM.SLAB_MEAN), _slab_images(bad.host, vv.FILTER_TEX8, SM.SLAB_MEAN)):
        rows.append((f"slab mean {view[0]}",) + _differing(a[0].view(np.uint32), b[0].view(np.uint32), _slice_coords(view)[1].ravel()))
    ha, hb = (sum(HM.histogram(m.host[z:z + 64]).counts for z in range(0, m.host.shape[0], 64)) for m in (good, bad))      # (64 slices at a time)
    rows.append(("histogram bins",) + (int((ha != hb).sum()), 256))
    return [(name, bug) + r for r in rows] + _volume_call_sensitivity(name, bug, good.host, bad.host)


def _volume_call_sensitivity(name, bug, good_host, bad_host):
    """One row per volume-to-volume family: on how many output voxels of its calls on the two straddling boxes the models of the two volumes differ."""
    V = _layout_only(name)
    rows = []
    for family in AV.FAMILIES:
        boxes = _family_boxes(V, family)
        differ = of = 0
        for bname in AV.STRADDLING:
            for case in AV.cases(family, bname, int(good_host.dtype == np.float32)):
                a, b = (AV.records(family, AV.want(family, case, h, boxes[bname]), h, boxes[bname]) for h in (good_host, bad_host))
                d = _differing(a[:, None, :], b[:, None, :])    # (per output voxel)
                differ, of = differ + d[0], of + d[1]
        rows.append((name, bug, f"{family}, straddling boxes", differ, of))
    return rows


def _write_sensitivity(rows, path):
    lines = ["On how many of the compared pixels (bins, output voxels) the host models of a misread volume differ from the models of the volume itself: what the",
             "comparisons of tests/test_addressing.py would report if a kernel read its voxels through the offset named.  Written by",
             "tests/test_addressing.py::test_models_notice_a_misread_volume (thin volumes) and, for the volumes of several GB, by the same functions",
             "run once by hand (_sensitivity_of_big_volumes).  Offsets outside the volume read 0.  The low sagittal images of the large volumes lie",
             "wholly below the limit and are read correctly: 0 by construction (they are the compared pixels decided below the limit).  The rows of the",
             "volume-to-volume families count the output voxels of all their calls on the two boxes that straddle the limit, in the library's pitches.", "",
             "volume".ljust(18) + "bug".ljust(38) + "image".ljust(46) + "differ".rjust(9) + "of".rjust(9)]
    lines += [r[0].ljust(18) + r[1].ljust(38) + r[2].ljust(46) + str(r[3]).rjust(9) + str(r[4]).rjust(9) for r in rows]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _read_sensitivity(path):
    if not os.path.exists(path):
        return []
    rows = [re.split(r"\s{2,}", l.strip()) for l in open(path).read().splitlines()]
    return [(r[0], r[1], r[2], int(r[3]), int(r[4])) for r in rows if len(r) == 5 and r[0] in SPECS and r[3].isdigit() and r[4].isdigit()]


SENSITIVITY_FILE = os.path.join(REPO, "profiles", "addressing_sensitivity.txt")
MUL24 = ("slice pitch multiplied in 24 bits", lambda pitch: pitch & 0xFFFFFF, lambda off: off)
MOD32 = ("offset modulo 2^32", lambda pitch: pitch, lambda off: off & 0xFFFFFFFF)
SIGN32 = ("offset sign-extended from 32 bits", lambda pitch: pitch, lambda off: np.where(off & 0x80000000, (off & 0xFFFFFFFF) - (1 << 32), off & 0xFFFFFFFF))


@pytest.mark.parametrize("name", ["thin_at_f32", "thin_at_u8"])
def test_models_notice_a_misread_volume(name):
    """A slice pitch at 2^24 multiplied as a 24-bit value: every image kind of the module differs on at least the share of pixels the conditions ask
    for (10 % of the pixels decided by one voxel, 30 % of those that cross the volume).  The thin rows of profiles/addressing_sensitivity.txt."""
    good = _thin_models(name)
    bad = Models(_misread(good.host, MUL24[1], MUL24[2]), good.tf)
    assert not np.array_equal(bad.host[1], good.host[1]) and np.array_equal(bad.host[0], good.host[0])
    rows = _sensitivity(name, MUL24[0], good, bad)
    for r in rows:
        print(*r)
        need = 0.30 if ("mean" in r[2] or "composite" in r[2]) else 0.10
        assert r[3] >= need * r[4], r
    try:                                                        # the thin rows replace their earlier version; the big volumes' rows stay
        keep = _read_sensitivity(SENSITIVITY_FILE)
        _write_sensitivity(sorted([k for k in keep if k[0] != name] + rows, key=lambda r: (NAMES.index(r[0]), r[1])), SENSITIVITY_FILE)
    except (OSError, ValueError):
        pass                                                    # a read-only checkout: the assertions above are the test


def _sensitivity_of_big_volumes(names=("f32_band", "u8_pair_refused", "f32_above", "u8_above"), volume_calls_only=False):
    """The rows of the volumes of several GB (minutes of host time and 20 GB of host memory: run by hand, `python -c "import test_addressing as t;
    t._sensitivity_of_big_volumes()"` from tests/): offsets modulo 2^32 on the volumes beyond 4 GiB, offsets sign-extended from 32 bits on the band volumes.
    volume_calls_only: the rows of the volume-to-volume families alone, the others kept as the file has them."""
    keep = _read_sensitivity(SENSITIVITY_FILE)
    for name in names:
        good = Models(_host_noise(name), _table())
        bug = MOD32 if SPECS[name].limit == 1 << 32 else SIGN32
        bad = None if volume_calls_only else Models(_misread(good.host, bug[1], bug[2]), good.tf)
        if volume_calls_only:
            V = _layout_only(name)                              # (these boxes lie where the library's layout passes the limit: its pitches)
            bad = Models(_misread(good.host, bug[1], bug[2], (V.row_bytes, V.slice_bytes)), good.tf)
            rows = _volume_call_sensitivity(name, bug[0], good.host, bad.host)
            keep = [k for k in keep if k[0] != name or k[2] not in [r[2] for r in rows]] + rows
        else:
            keep = [k for k in keep if k[0] != name] + _sensitivity(name, bug[0], good, bad)
        _write_sensitivity(sorted(keep, key=lambda r: (NAMES.index(r[0]), r[1])), SENSITIVITY_FILE)


# ---- the volume-to-volume families (derive, stencil, resample, label and mask): boxes, deciding voxels, conditions ----
def _layout_only(name):
    """What _hist_boxes and the conditions need of a Loaded, from the spec alone: the pitches by the re-pitch rule Loaded.__init__ states."""
    s = SPECS[name]
    dtype = np.float32 if s.dtype == "f32" else np.uint8
    row, slice_bytes = AV.pitches(s.dims, np.dtype(dtype).itemsize)
    return SimpleNamespace(name=name, spec=s, models=SimpleNamespace(host=np.empty((0, 0, 0), dtype)), row_bytes=row, slice_bytes=slice_bytes)


def _layout(V):
    return AV.Layout(V.spec.dims, V.models.host.itemsize, V.row_bytes, V.slice_bytes, V.spec.limit)


def _family_boxes(V, family):
    """_hist_boxes, grown where the family needs it; each keeps the property it is named for."""
    L, out = _layout(V), {}
    for bname, box in _hist_boxes(V).items():
        out[bname] = AV.family_box(family, box, V.spec.dims)
        assert AV.box_property(bname, out[bname], L, V.spec.dims), (V.name, family, bname, out[bname])
    return out


def _share_conditions(V, family):
    """From the layout alone: of the output voxels of the two straddling boxes together, 10 % to 90 % are decided beyond the limit."""
    L, out = _layout(V), {}
    for what, off in AV.shares(family, _family_boxes(V, family), L):
        share = float((off >= L.limit).mean())
        assert len(off) >= 200 and 0.10 <= share <= 0.90, f"{V.name} {what}: {share:.3f} of {len(off)} output voxels are decided beyond the limit"
        out[what] = round(share, 3)
    return out


def _volume_call_plan(V, family, host):
    """Every call of one family on one volume with the model's output, and the module's conditions on the two straddling boxes asserted from the models
    and the layout alone: [namespace(bname, box, k, case, want)]."""
    L, boxes = _layout(V), _family_boxes(V, family)
    src_type = int(host.dtype == np.float32)
    plan = [SimpleNamespace(bname=bname, box=box, k=k, case=case, want=AV.want(family, case, host, box))
            for bname, box in boxes.items() for k, case in enumerate(AV.cases(family, bname, src_type, other_type=bname == "inside a row"))]
    labels = []
    for k, case in enumerate(AV.cases(family, "across slices", src_type)):
        items = [p for p in plan if p.bname in AV.STRADDLING and p.k == k]
        assert [p.bname for p in items] == list(AV.STRADDLING)
        off, rec = [], []
        for p in items:
            o, ok = AV.deciding(family, p.case, p.box, L)
            assert o.shape == (p.want[0] if family == "label and mask" else p.want).shape
            off.append(o[ok]); rec.append(AV.records(family, p.want, host, p.box)[ok.ravel()])
        what = f"{V.name} {family} {({k_: v for k_, v in case.items() if k_ != 'taps'})}"
        print(what, _decided(np.concatenate(off), L.limit, np.concatenate(rec), what))
        if family == "label and mask":
            labels.append(len(np.unique(np.concatenate([p.want[0][p.want[0] > 0] for p in items]))))
    if family == "label and mask":
        # 20 distinct labels across both sides.  Under 26 a foreground share of 0.3 ... 0.6 lies at three to six times the percolation threshold
        # (0.097): nearly all of it is one component whatever the noise, so the count is asserted under 6 and the 26 run must have fewer components.
        assert labels[0] >= 20 and 1 <= labels[1] < labels[0], (V.name, labels)
        for p in plan:
            share = p.want[2].foreground / p.want[0].size
            assert 0.3 <= share <= 0.6, (V.name, p.bname, share)
    return plan


def test_volume_call_boxes_and_shares():
    """Every volume whose linear layout passes its limit, without voxel data: the boxes have the properties they are named for and the deciding voxels
    of the straddling boxes lie on both sides of the limit, for each of the four families."""
    assert [n for n in NAMES if n not in LINEAR_NAMES] == ["u8_pair_top"]
    s = SPECS["u8_pair_top"]
    assert AV.pitches(s.dims, 1)[1] * s.dims[2] < s.limit           # nothing of its linear layout lies beyond the limit: no box can straddle it
    for name in LINEAR_NAMES:
        V = _layout_only(name)
        assert (V.slice_bytes * V.spec.dims[2] > 1 << 32 or V.slice_bytes >= 1 << 24) == V.spec.big, name
        for family in AV.FAMILIES:
            print(name, family, _share_conditions(V, family))


@pytest.mark.parametrize("family", AV.FAMILIES)
@pytest.mark.parametrize("name", THIN)
def test_thin_volume_call_preconditions(name, family):
    """The full conditions of the four families' comparisons on the thin volumes, from the models alone."""
    _volume_call_plan(_layout_only(name), family, _thin_models(name).host)


@pytest.mark.parametrize("connectivity", LM.CONNECTIVITIES)
def test_sparse_label_model_is_the_label_model(connectivity):
    """The wide label box's structures in a 63 x 41 x 39 volume: the sparse model over the coordinate list equals label_model.label."""
    dims = AV.SMALL["dims"]
    idx, parts = AV.wide_foreground(**AV.SMALL)
    vol = np.zeros(dims[::-1], np.uint8)
    vol.ravel()[idx] = WIDE_FG
    labels, sizes, stats = LM.label(vol, (WIDE_FG, WIDE_FG), connectivity)
    got = AV.sparse_label(idx, dims, connectivity)
    assert np.array_equal(got[0], labels.ravel()[idx]) and np.array_equal(got[1], sizes.ravel()[idx]), connectivity
    assert got[2] == (stats.foreground, stats.components, stats.largest_size, stats.largest_label, stats.reserved)
    assert int(labels.astype(bool).sum()) == len(idx) and int(sizes.astype(bool).sum()) == stats.components
    _wide_conditions(idx, parts, got, AV.SMALL["half"], AV.SMALL["stairs"], connectivity)


def _wide_conditions(idx, parts, model, half, stairs, connectivity):
    """What the wide label box must show before a kernel runs: `stairs` expected labels above `half` (the staircase's voxels under 6; the loop's under
    every connectivity), a component with members on both sides of `half` whose label is tiny, a unique largest component."""
    labels, sizes, stats = model
    high = labels[labels.astype(np.int64) - 1 >= half]           # (a label is an index + 1)
    assert len(high) >= stairs and len(np.unique(high)) >= (stairs if connectivity == 6 else 2), (connectivity, len(high), len(np.unique(high)))
    loop = labels[np.isin(idx, parts["loop"])]
    assert len(np.unique(loop)) == 1 and int(loop[0]) == int(parts["loop"].min()) + 1 > half
    wire = labels[np.isin(idx, parts["wire"])]
    assert len(np.unique(wire)) == 1 and int(wire[0]) - 1 < idx[-1] >> 8
    members = idx[labels == wire[0]]
    assert members.min() < half <= members.max() and members.max() == idx[-1]
    assert int((sizes == stats[2]).sum()) == 1 and stats[3] == int(wire[0])
    st = labels[np.isin(idx, parts["stairs"])]
    assert len(np.unique(st)) == {6: stairs, 18: stairs // 2, 26: 1}[connectivity]


# ---------------------------------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------------------------------
class Loaded:
    """One volume on the device and on the host, with what the library reports about its layouts."""

    def __init__(self, ctx, name):
        import torch
        self.ctx, self.name, self.spec = ctx, name, SPECS[name]
        nx, ny, nz = self.spec.dims
        n = nx * ny * nz
        dev = torch.device("cuda", 0)
        free_b, total_b = torch.cuda.mem_get_info(dev)
        if total_b < 100 * 2 ** 30:                              # (test_c5_streamed_2048_phong's guard: only a physically smaller GPU model skips)
            pytest.skip(f"device has {total_b / 2 ** 30:.0f} GiB in all: not an MI355X-class GPU")
        assert free_b >= 60 * 2 ** 30, f"the addressing volumes need 60 GiB of free HBM, the device reports {free_b / 2 ** 30:.1f} of {total_b / 2 ** 30:.0f} GiB free"
        self.tf = _table()
        t0 = time.time()
        with MO.knobs(ctx, {}):
            v8 = torch.empty(n, dtype=torch.uint8, device=dev)
            for z0, z1, seed in _noise_parts(self.spec.dims):
                ctx.generate_noise_device(v8.data_ptr() + z0 * ny * nx, nx, ny, z1 - z0, seed)
            v = v8
            if self.spec.dtype == "f32":
                v = torch.empty(n, dtype=torch.float32, device=dev)
                ctx.promote_device(v8.data_ptr(), v.data_ptr(), n)
            ctx.load_volume_device(v.data_ptr(), vv.VOXEL_F32 if self.spec.dtype == "f32" else vv.VOXEL_U8, nx, ny, nz, self.tf)
            torch.cuda.synchronize()
            self.counts8 = np.zeros(256, np.uint64)             # torch.bincount of the u8 device tensor, a slab at a time
            for a in range(0, n, 1 << 28):
                self.counts8 += torch.bincount(v8[a:a + (1 << 28)], minlength=256).cpu().numpy().astype(np.uint64)
            self.range8 = (int(v8.min()), int(v8.max()))
            host = v.cpu().numpy().reshape(nz, ny, nx)
            del v, v8
            torch.cuda.empty_cache()
        host.setflags(write=False)
        self.models = Models(host, self.tf)
        # the linear layout as the library holds it: nz slices + one slice + two rows + 4 KiB; rows of a multiple of 1 KiB are re-pitched by 32 bytes,
        # with one more row if the slice would still be a multiple of 4 KiB (1280 f32 voxels a row; test_padded_pitch_layout's formula)
        size = host.itemsize
        self.row_bytes = nx * size + (32 if nx * size % 1024 == 0 else 0)
        rows = ny + (1 if self.row_bytes != nx * size and ny * self.row_bytes % 4096 == 0 else 0)
        linear = ctx.device_bytes()[0]
        assert linear == ctx.layout_state()["linear"] and (linear - 2 * self.row_bytes - 4096) % (nz + 1) == 0, (linear, self.spec.dims)
        self.slice_bytes = (linear - 2 * self.row_bytes - 4096) // (nz + 1)
        assert self.slice_bytes == rows * self.row_bytes, (self.slice_bytes, self.spec.dims)
        self.linear_bytes = self.slice_bytes * nz
        print(f"{name}: generated, loaded and downloaded in {time.time() - t0:.1f} s; linear layout {self.linear_bytes} bytes, slice pitch {self.slice_bytes}")

    def free(self):
        with MO.knobs(self.ctx, {}):
            self.ctx.load_volume(np.zeros((4, 4, 4), np.uint8), self.tf)    # frees the volume and its copies for the tests that follow

    def prepare(self, build):
        """Inside MO.knobs(ctx, BUILDS[build][0]), before any frame: builds (or is refused) the copies of `build`, asserts their residency as the table
        says and that at least 30 % of the sampled layout lies beyond the limit; returns (axis, first voxel index beyond the limit along it)."""
        env, bit, copies, axis = BUILDS[build]
        s = self.spec
        if bit:
            self.ctx.prepare_layouts(bit)
        state = self.ctx.layout_state()
        for c in copies:
            assert (state[c] > 0) == (c not in s.refused), f"{self.name} {build}: copy {c} holds {state[c]} bytes"
        sampled = [c for c in copies if c not in s.refused]
        if build == "xpair" and "xpair" in s.refused:
            axis = 0                                            # the z-fastest copy serves the frame
        elif build == "zpair" and "zpair" in s.refused:
            sampled = []                                        # the linear layout does
        layout_bytes = state[sampled[-1]] if sampled else self.linear_bytes
        if build == "linear" or not sampled:
            assert (self.linear_bytes > 1 << 32 or self.slice_bytes >= 1 << 24) == s.big
            first = _first_beyond_linear(s.limit, self.slice_bytes)
        else:
            first = _first_beyond(s.limit, layout_bytes, s.dims[axis])
        share = 1.0 - s.limit / layout_bytes
        assert share >= 0.30, f"{self.name} {build}: {share:.3f} of the sampled layout's {layout_bytes} bytes lie beyond {s.limit}"
        if sampled and sampled[-1] in ("zpair", "xpair") and s.dtype == "u8":
            assert layout_bytes < 1 << 32                       # the u8 pair sampler's 32-bit offsets
        return axis, first

    def check_launch(self, build, phong, what):
        """After an instrumented frame: the layout the frame sampled and the waves-per-copy counters."""
        lay = self.ctx.last_launch()
        code = self.spec.builds[build][1 if phong == 1 else 0]
        assert lay["layout"] == code and lay["phong"] == phong, (what, lay, code)
        counters = self.ctx.debug_counters()
        assert (counters[2] > 0) == (code == 2) and (counters[3] > 0) == (code in (3, 5)), (what, code, [int(c) for c in counters[:4]])


@pytest.fixture(scope="module")
def vol(request, ctx):
    v = None
    try:
        v = Loaded(ctx, request.param)
        yield v
    finally:
        if v is not None:
            v.free()
        else:
            with MO.knobs(ctx, {}):
                ctx.load_volume(np.zeros((4, 4, 4), np.uint8), _table())


def _each_build(V, family):
    """(build, axis, first voxel beyond the limit) under the build's knobs, copies prepared."""
    for build in V.spec.builds:
        if build == "xpair" and family == "phong":
            continue                                            # Phong frames never take the x-pair copy (the z-fastest build serves them, covered under its own name)
        with MO.knobs(V.ctx, BUILDS[build][0]):
            axis, first = V.prepare(build)
            yield build, axis, first


@pytest.mark.gpu
@pytest.mark.parametrize("vol", NAMES, indirect=True)
def test_mip(vol):
    V, ctx, Mo = vol, vol.ctx, vol.models
    for build, axis, first in _each_build(V, "mip"):
        what = f"{V.name} {build} mip"
        print(what, Mo.extremum_condition(PM.PROJ_MAX, axis, first, what))
        for cam_name, cam in CAMS:
            M, written, n_want = Mo.mip(cam_name)
            MO.assert_not_vacuous(M, what)
            assert np.array_equal(np.where(written, M, 0), np.where(written, Mo.proj(cam_name, PM.PROJ_MAX)["index"], 0)), what      # the deciding samples are PROJ_MAX's
            MO.assert_frame(ctx, M, written, V.tf, FILL, W, H, cam, f"{what} camera {cam_name}", options=vv.make_options(step=STEP))
            MO.assert_frame(ctx, M, written, V.tf, FILL, W, H, cam, f"{what} camera {cam_name} counted", options=vv.make_options(step=STEP, count_samples=True))
            assert ctx.last_sample_count() == n_want, what
            V.check_launch(build, 2, what)


@pytest.mark.gpu
@pytest.mark.parametrize("vol", NAMES, indirect=True)
def test_iso(vol):
    V, ctx, Mo = vol, vol.ctx, vol.models
    levels = Mo.levels()
    assert levels[1] > levels[0], levels
    for build, axis, first in _each_build(V, "iso"):
        for level in levels:
            what = f"{V.name} {build} iso level {level}"
            print(what, Mo.iso_condition(level, axis, first, what))
            for cam_name, cam in CAMS:
                m = Mo.iso(cam_name, level)
                got = ctx.render_iso(W, H, cam, level, fill=FILL, return_index=True, return_hit=True, options=vv.make_options(step=STEP, count_samples=True))
                _same(got[1], m["index"], f"{what} camera {cam_name}: index image")
                _same(got[2], m["hit"], f"{what} camera {cam_name}: hit records")
                _same(got[0], m["rgba"], f"{what} camera {cam_name}: rgba")
                assert ctx.last_sample_count() == m["count"], what
                V.check_launch(build, 3, what)
        near, deep = (np.median(Mo.iso("hi", l)["hit"][..., 3][Mo.iso("hi", l)["hit"][..., 3] > 0]) for l in levels)
        assert deep > near, (near, deep)                   # the high level's hits lie deeper along the rays


@pytest.mark.gpu
@pytest.mark.parametrize("vol", NAMES, indirect=True)
def test_projection(vol):
    V, ctx, Mo = vol, vol.ctx, vol.models
    for build, axis, first in _each_build(V, "proj"):
        for mode, mname in ((PM.PROJ_MAX, "max"), (PM.PROJ_MIN, "min"), (PM.PROJ_MEAN, "mean")):
            what = f"{V.name} {build} projection {mname}"
            print(what, Mo.crossing_condition(axis, first, what) if mode == PM.PROJ_MEAN else Mo.extremum_condition(mode, axis, first, what))
            for cam_name, cam in CAMS:
                m = Mo.proj(cam_name, mode)
                got = ctx.render_projection(W, H, cam, mode, fill=FILL, return_index=True, return_stat=True, options=vv.make_options(step=STEP, count_samples=True))
                _same(got[2], m["stat"], f"{what} camera {cam_name}: record image")
                _same(got[1], m["index"], f"{what} camera {cam_name}: index image")
                _same(got[0], m["rgba"], f"{what} camera {cam_name}: rgba")
                assert ctx.last_sample_count() == m["count"], what
                V.check_launch(build, 4, what)


@pytest.mark.gpu
@pytest.mark.parametrize("phong", [False, True], ids=["unshaded", "phong"])
@pytest.mark.parametrize("vol", NAMES, indirect=True)
def test_composite(vol, phong):
    """march_kernel / march_phong_kernel: a band of slab rows of the frame against the oracle, and the band's executed-sample count."""
    V, ctx, Mo = vol, vol.ctx, vol.models
    rows = slice(CBAND[0] * 14, CBAND[1] * 14)
    for build, axis, first in _each_build(V, "phong" if phong else "march"):
        what = f"{V.name} {build} composite phong={phong}"
        print(what, Mo.composite_condition(axis, first, what))
        for cam_name, cam in CAMS:
            want, n_band = Mo.composite(cam_name, phong)
            assert (want[rows][..., 3] > 0).mean() > 0.2 and len(np.unique(want[rows].reshape(-1, 4), axis=0)) >= 20, what
            full = ctx.render(CW, CH, cam, phong=phong, options=vv.make_options(step=CSTEP, count_samples=True))
            n_full = ctx.last_sample_count()
            V.check_launch(build, int(phong), what)
            _same(full[rows], want[rows], f"{what} camera {cam_name}: the band of the whole frame")
            got = np.zeros_like(full)
            ctx.render(CW, CH, cam, phong=phong, options=vv.make_options(step=CSTEP, slab_rows=CBAND, count_samples=True), out=got)
            _same(got[rows], want[rows], f"{what} camera {cam_name}: the band alone")
            assert ctx.last_sample_count() == n_band and 0 < n_band < n_full, (what, ctx.last_sample_count(), n_band, n_full)


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [vv.FILTER_TEX8, vv.FILTER_EXACT], ids=["tex8", "exact"])
@pytest.mark.parametrize("vol", LINEAR_NAMES, indirect=True)
def test_slices_and_slabs(vol, filt):
    """slice_kernel and slab_kernel (both sample the linear layout and pick their addressing from VolumeView::big at run time)."""
    V, ctx, host = vol, vol.ctx, vol.models.host
    with MO.knobs(ctx, {}):
        _, first = V.prepare("linear")
        images = V.models.get(("slices", filt), lambda: _slice_images(host, filt))
        print(V.name, "slices", _slice_condition(host, images, first, f"{V.name} slices filter {filt}"))
        for view, want in images:
            _, orient, d = view
            got = ctx.slice_advanced(SH, SW, O.slice_matrix(*FREE_FORM), filter=filt, fill=-1.0) if orient is None else \
                ctx.slice(SH, SW, *d, orientation=orient, filter=filt, fill=-1.0)
            _same(got, want, f"{V.name} slice {view[0]} filter {filt}")
        for mode in SM.MODES:
            slabs = V.models.get(("slabs", filt, mode), lambda: _slab_images(host, filt, mode))
            _slice_condition(host, [(v, pair[0]) for v, pair in slabs], first, f"{V.name} slabs mode {mode} filter {filt}")
            for view, want in slabs:
                _, orient, d = view
                kw = dict(mode=mode, samples=SLAB_K, thickness=SLAB_THICK, filter=filt, fill=-3.0, return_aux=True, aux_fill=-7)
                got = ctx.slice_advanced_slab(SH, SW, O.slice_matrix(*FREE_FORM), **kw) if orient is None else ctx.slice_slab(SH, SW, *d, orient, **kw)
                _same(got[0], want[0], f"{V.name} slab {view[0]} mode {mode} filter {filt}: values")
                _same(got[1], want[1], f"{V.name} slab {view[0]} mode {mode} filter {filt}: aux")


def _hist_same(got, want, what):
    bad = np.flatnonzero(np.asarray(got.counts, np.uint64) != want.counts)
    assert len(bad) == 0, f"{what}: {len(bad)} bins differ, first {bad[0]}: {got.counts[bad[0]]} vs {want.counts[bad[0]]}"
    assert got.voxels == want.voxels == int(want.counts.sum()) and got.nan_voxels == want.nan_voxels, (what, got.voxels, want.voxels, got.nan_voxels)
    for a, b in ((got.vmin, want.vmin), (got.vmax, want.vmax)):
        assert np.asarray(a, f32).reshape(1).view(np.uint32)[0] == np.asarray(b, f32).reshape(1).view(np.uint32)[0], (what, a, b)


def _hist_boxes(V):
    """A box wholly below the limit, one that straddles it inside a row, one that straddles it across a slice boundary, one that ends at the last voxel."""
    nx, ny, nz = V.spec.dims
    size = V.models.host.itemsize
    z, rem = divmod(V.spec.limit, V.slice_bytes)
    y, x = rem // V.row_bytes, (rem % V.row_bytes) // size
    assert 0 < z < nz or (z == 0 and V.spec.big), (z, y, x)
    clip = lambda lo, hi, n: (max(min(lo, n - 1), 0), max(min(hi, n), max(min(lo, n - 1), 0) + 1))
    boxes = {"below": ((0, 0, 0), (40, 10, min(8, max(z, 1)))),
             "inside a row": tuple(zip(clip(x - 20, x + 20, nx), clip(y - 3, y + 4, ny), clip(z - 2, z + 3, nz))),
             "across slices": ((5, 5, max(z - 1, 0)), (45, 15, min(z + 2, nz))),
             "last voxel": ((nx - 40, ny - 10, max(nz - 8, min(z + 1, nz - 1))), (nx, ny, nz))}
    off = lambda p: p[2] * V.slice_bytes + p[1] * V.row_bytes + p[0] * size
    last = lambda b: off((b[1][0] - 1, b[1][1] - 1, b[1][2] - 1))
    if z > 0:
        assert last(boxes["below"]) < V.spec.limit
    for k in ("inside a row", "across slices"):
        assert off(boxes[k][0]) < V.spec.limit <= last(boxes[k]), (k, boxes[k])
    assert off(boxes["last voxel"][0]) >= V.spec.limit and boxes["last voxel"][1] == (nx, ny, nz)
    return boxes


@pytest.mark.gpu
@pytest.mark.parametrize("vol", LINEAR_NAMES, indirect=True)
def test_histogram(vol):
    V, ctx, host = vol, vol.ctx, vol.models.host
    nx, ny, nz = V.spec.dims
    if host.dtype == np.uint8:
        whole = SimpleNamespace(counts=V.counts8, voxels=host.size, nan_voxels=0, vmin=f32(V.range8[0]), vmax=f32(V.range8[1]))
    else:                                                       # u8 / 255 promoted: the u8 counts through the model's bin of the 256 values v / 255
        values = np.arange(256, dtype=f32) / f32(255)
        counts = np.zeros(256, np.uint64)
        np.add.at(counts, HM.bins(values), V.counts8)
        whole = SimpleNamespace(counts=counts, voxels=host.size, nan_voxels=0, vmin=values[V.range8[0]], vmax=values[V.range8[1]])
    assert int(V.counts8.sum()) == nx * ny * nz and (V.counts8 > 0).sum() >= 100
    try:
        for blocks in (None, "1", "7"):
            with MO.knobs(ctx, {}):
                if blocks is not None:
                    os.environ["VV_HIST_BLOCKS"] = blocks
                ctx.reread_env()
                _, _ = V.prepare("linear")
                _hist_same(ctx.histogram(prefill=0xA5), whole, f"{V.name} whole volume VV_HIST_BLOCKS={blocks}")
                for bname, box in _hist_boxes(V).items():
                    _hist_same(ctx.histogram(box, prefill=0xA5), HM.histogram(host, box), f"{V.name} box {bname} {box} VV_HIST_BLOCKS={blocks}")
                os.environ.pop("VV_HIST_BLOCKS", None)
    finally:
        os.environ.pop("VV_HIST_BLOCKS", None)
        ctx.reread_env()


@pytest.mark.gpu
def test_histogram_counts_more_than_2_to_32_voxels_of_one_value(ctx):
    """2048 x 2048 x 1025 zeros under VV_HIST_BLOCKS=1: launch_hist must not go down to so few blocks that a 32-bit sub-counter wraps."""
    import torch
    nx, ny, nz = 2048, 2048, 1025
    assert nx * ny * nz > 1 << 32
    tf = _table()
    try:
        with MO.knobs(ctx, {}):
            z = torch.zeros(nx * ny * nz, dtype=torch.uint8, device=torch.device("cuda", 0))
            ctx.load_volume_device(z.data_ptr(), vv.VOXEL_U8, nx, ny, nz, tf)
            torch.cuda.synchronize()
            del z
            torch.cuda.empty_cache()
            os.environ["VV_HIST_BLOCKS"] = "1"
            ctx.reread_env()
            h = ctx.histogram(prefill=0xA5)
            assert int(h.counts[0]) == nx * ny * nz == h.voxels and int(h.counts[1:].sum()) == 0 and h.vmin == 0 and h.vmax == 0 and h.nan_voxels == 0
    finally:
        os.environ.pop("VV_HIST_BLOCKS", None)
        with MO.knobs(ctx, {}):
            ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)


# ---------------------------------------------------------------------------------------------------------------------
# the volume-to-volume families: source addresses beyond the limits (boxes), outputs beyond 2^32 bytes, a label box of more than 2^31 voxels
# ---------------------------------------------------------------------------------------------------------------------
def _report(family, got, want, what):
    VO.report(got, want, AV.same(family, got, want), what)


def _device_and_host(ctx, family, p, dims):
    """(device call(ptr, capacity) -> (bx, by, bz), host call() -> array) of one planned call of derive, stencil or resample."""
    c = p.case
    if family == "derive":
        kw = dict(box=p.box, factor=c["factor"], mode=c["mode"], out_type=c["out_type"])
        return (lambda ptr, cap: ctx.derive_device(ptr, cap, **kw)), (lambda: ctx.derive(prefill=VO.GARBAGE, **kw))
    if family == "stencil":
        kw = dict(box=p.box, out_type=c["out_type"], radius=c.get("radius", (0, 0, 0)), taps=c.get("taps"))
        return (lambda ptr, cap: ctx.stencil_device(ptr, cap, c["kind"], **kw)), (lambda: ctx.stencil(c["kind"], prefill=VO.GARBAGE, **kw))
    assert family == "resample"
    matrix = None
    if c["rotated"]:
        matrix = vv.resample_matrix(AV.EULER, 1.0, AV.rotation_centre(p.box, dims))
        assert matrix.tobytes() == AV.rotation(p.box, dims).tobytes(), "vv_resample_matrix is not the model's matrix"
    kw = dict(matrix=matrix, filter=c["filter"], fill=0.0, box=p.box)
    return (lambda ptr, cap: ctx.resample_device(ptr, cap, dims, **kw)), (lambda: ctx.resample(dims, prefill=VO.GARBAGE, **kw))


def _volume_calls(V, family):
    """derive, stencil or resample on the four boxes of one volume: every planned call into the guarded device buffer, and through the host path
    once per call kind on the box that straddles the limit inside a row."""
    ctx, host = V.ctx, V.models.host
    with MO.knobs(ctx, {}):
        V.prepare("linear")
        plan = V.models.get(("volume calls", family), lambda: _volume_call_plan(V, family, host))
        dev = VO.DeviceOut(max(p.want.nbytes for p in plan))
        for p in plan:
            what = f"{V.name} {family} box {p.bname} {p.box} {({k: v for k, v in p.case.items() if k != 'taps'})}"
            device_call, host_call = _device_and_host(ctx, family, p, V.spec.dims)
            _report(family, dev.run(device_call, p.want.shape, p.want.dtype.type, what), p.want, what + " (device)")
            if p.bname == "inside a row" and (family != "derive" or p.case["mode"] == 0):
                _report(family, host_call(), p.want, what + " (host)")


@pytest.mark.gpu
@pytest.mark.parametrize("vol", LINEAR_NAMES, indirect=True)
def test_derive(vol):
    """derive_kernel: vector loads (factor 1 from a 16-voxel boundary) and the generic path, source addresses on both sides of the limit."""
    _volume_calls(vol, "derive")


@pytest.mark.gpu
@pytest.mark.parametrize("vol", LINEAR_NAMES, indirect=True)
def test_stencil(vol):
    """stencil_sep_kernel, the median and the gradient magnitude; the boxes `below` and `last voxel` clamp at the volume's first and last slice."""
    _volume_calls(vol, "stencil")


@pytest.mark.gpu
@pytest.mark.parametrize("vol", LINEAR_NAMES, indirect=True)
def test_resample(vol):
    """resample_kernel on the volume's own grid, identity and a small rotation about the box's centre, TEX8 / EXACT / NEAREST: the 32-bit offsets
    (with the 24-bit slice multiply) below the limits of VolumeView::big, the 64-bit slice bases beyond them."""
    assert max(vol.spec.dims) <= 16384
    _volume_calls(vol, "resample")


def _guarded_words(torch, n):
    """n uint32 words on the device between two guards of 16 words, everything 0xA5A5A5A5: (tensor, pointer of the words)."""
    t = torch.full((n + 32,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=torch.device("cuda", 0))
    return t, t.data_ptr() + 64


def _words(t, n, what):
    raw = t.cpu().numpy().view(np.uint32)
    assert (raw[:16] == 0xA5A5A5A5).all() and (raw[16 + n:] == 0xA5A5A5A5).all(), f"words outside the output were written ({what})"
    return raw[16:16 + n].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("vol", LINEAR_NAMES, indirect=True)
def test_label_and_mask(vol):
    """label_local_kernel and the merge phases read `src` on both sides of the limit; mask_kernel is fed the labels and sizes the call left on the device."""
    import torch
    V, ctx, host = vol, vol.ctx, vol.models.host
    family = "label and mask"
    with MO.knobs(ctx, {}):
        V.prepare("linear")
        plan = V.models.get(("volume calls", family), lambda: _volume_call_plan(V, family, host))
        dev = VO.DeviceOut(max(p.want[0].size for p in plan) * 4)
        for p in plan:
            labels, sizes, stats = p.want
            n, conn, bins = labels.size, p.case["connectivity"], AV.label_bins(host, p.box)
            what = f"{V.name} label box {p.bname} {p.box} bins {bins} connectivity {conn}"
            lab_t, lab_p = _guarded_words(torch, n)
            siz_t, siz_p = _guarded_words(torch, n)
            st_t = torch.full((6,), -1, dtype=torch.int64, device=torch.device("cuda", 0))
            torch.cuda.synchronize()
            assert ctx.label_device(lab_p, n * 4, bins, conn, p.box, sizes_ptr=siz_p, stats_ptr=st_t.data_ptr() + 8) == labels.shape[::-1]
            _report(family, _words(lab_t, n, what).reshape(labels.shape), labels, what + ": labels")
            _report(family, _words(siz_t, n, what).reshape(labels.shape), sizes, what + ": sizes")
            st = st_t.cpu().numpy()
            got = vv.LabelStats.from_bytes(st[1:5].tobytes())
            assert st[0] == -1 and st[5] == -1 and (got.foreground, got.components, got.largest_size, got.largest_label, got.reserved) == \
                (stats.foreground, stats.components, stats.largest_size, stats.largest_label, 0), (what, got, stats)
            for mc in AV.mask_cases():
                want = AV.want_mask(host, labels, sizes, p.box, mc)
                mwhat = f"{what}: mask {mc}"
                got = dev.run(lambda ptr, cap: ctx.mask_device(ptr, cap, lab_p, mc["keep"], min_size=mc["min_size"], sizes_ptr=siz_p, fill=mc["fill"], box=p.box,
                                                               out_type=mc["out_type"]), want.shape, want.dtype.type, mwhat)
                _report(family, got, want, mwhat)
            if p.bname == "inside a row":
                got = ctx.label(bins, conn, p.box, sizes=True, stats=True, prefill=VO.GARBAGE)
                _report(family, got[0], labels, what + ": host labels")
                _report(family, got[1], sizes, what + ": host sizes")
                assert (got[2].foreground, got[2].components, got[2].largest_size, got[2].largest_label) == (stats.foreground, stats.components, stats.largest_size, stats.largest_label)
                mc = AV.mask_cases()[3]
                _report(family, ctx.mask(got[0], mc["keep"], min_size=mc["min_size"], sizes=got[1], fill=mc["fill"], box=p.box, out_type=mc["out_type"], prefill=VO.GARBAGE),
                        AV.want_mask(host, labels, sizes, p.box, mc), what + ": host mask")


OUT_GUARD = 64                                                  # the DeviceOut rule by hand: 0xA5 everywhere before a call, 64 bytes on either side of the output


class _BigOut:
    """A device buffer for outputs of several GB: nothing of its size ever goes to the host."""

    def __init__(self, torch, nbytes):
        self.torch, self.nbytes = torch, nbytes
        self.buf = torch.empty(nbytes + 2 * OUT_GUARD, dtype=torch.uint8, device=torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr() + OUT_GUARD
        assert self.ptr % 16 == 0

    def run(self, call, nbytes, dims, what):
        """call(ptr, capacity) -> the output's (mx, my, mz), complete on return; the bytes before and behind the output keep 0xA5."""
        assert nbytes <= self.nbytes
        self.buf.fill_(VO.GARBAGE)
        self.torch.cuda.synchronize()
        assert tuple(call(self.ptr, nbytes)) == tuple(dims), what
        self.torch.cuda.synchronize()
        tail = self.buf[OUT_GUARD + nbytes:]
        assert bool((self.buf[:OUT_GUARD] == VO.GARBAGE).all()) and all(bool((tail[a:a + (1 << 30)] == VO.GARBAGE).all()) for a in range(0, tail.numel(), 1 << 30)), \
            f"bytes outside the output were written ({what})"

    def slices(self, z0, z1, dims, dtype):
        """Output slices z0 .. z1 - 1 of an output of `dims` on the host."""
        sb = dims[0] * dims[1] * np.dtype(dtype).itemsize
        return self.buf[OUT_GUARD + z0 * sb:OUT_GUARD + z1 * sb].cpu().numpy().view(dtype).reshape(z1 - z0, dims[1], dims[0])

    def tensor(self, nbytes, torch_dtype):
        return self.buf[OUT_GUARD:OUT_GUARD + nbytes].view(torch_dtype)


def _output_slabs(dims, itemsize):
    """(z0, z1) of the three compared slabs of an output of `dims`: its first three slices, three slices around output byte 2^32, its last three; from
    the arithmetic: the middle slab's bytes straddle 2^32 and the last slab ends at the output's last byte."""
    mx, my, mz = dims
    sb = mx * my * itemsize
    assert sb * mz > 1 << 32 and mz >= 6
    zc = min(max((1 << 32) // sb - 1, 0), mz - 3)
    slabs = ((0, 3), (zc, zc + 3), (mz - 3, mz))
    assert slabs[1][0] * sb < 1 << 32 < slabs[1][1] * sb and slabs[2][1] * sb == sb * mz and slabs[0][1] * sb < 1 << 32
    return slabs


@pytest.mark.gpu
@pytest.mark.parametrize("vol", ["f32_above", "u8_above"], indirect=True)
def test_volume_outputs_beyond_4_gib(vol):
    """The whole volume derived, filtered and resampled into outputs of more than 2^32 bytes: derive's `dst`, stencil_item's `first` / `plane`, resample's
    `at`.  (a) three slabs of each output against the model of the slab; (b) the calls that copy by contract -- derive at factor 1, a separable pass of
    radius 0, NEAREST under the identity -- against the source regenerated on the device, every byte; (c) the guard bytes; (d) derive and the stencils
    once more under a grid cap of 4096 blocks: their grid-stride loops then carry the item counters past 2^32 bytes."""
    import torch
    V, ctx, host = vol, vol.ctx, vol.models.host
    dims = nx, ny, nz = V.spec.dims
    n, size = nx * ny * nz, host.itemsize
    own = int(host.dtype == np.float32)
    assert n * size > 1 << 32
    taps1 = AV.StM.taps(AV.StM.BINOMIAL, 1)
    rot = vv.resample_matrix(AV.EULER, 1.0, (0.5, 0.5, 0.5))
    assert rot.tobytes() == AV.RM.matrix(AV.EULER, 1.0, (0.5, 0.5, 0.5)).tobytes()
    zbox = lambda s, z_off=0: ((0, 0, s[0] + z_off), (nx, ny, s[1] + z_off))
    sep = dict(kind=AV.StM.SEPARABLE, radius=(1, 1, 1), taps=taps1, out_type=own)
    med = dict(kind=AV.StM.MEDIAN, out_type=own)
    # name -> (device call, the model of an output slab (z0, z1), output dims, output dtype)
    calls = {
        "derive": (lambda p, cap: ctx.derive_device(p, cap, None, 1, AV.DM.MEAN, own), lambda s: AV.DM.derive(host, zbox(s), 1, AV.DM.MEAN, own), dims, host.dtype),
        "separable": (lambda p, cap: ctx.stencil_device(p, cap, sep["kind"], None, own, sep["radius"], taps1), lambda s: AV.want("stencil", sep, host, zbox(s)), dims, host.dtype),
        "median": (lambda p, cap: ctx.stencil_device(p, cap, med["kind"], None, own), lambda s: AV.want("stencil", med, host, zbox(s)), dims, host.dtype),
        "resample": (lambda p, cap: ctx.resample_device(p, cap, dims, rot, AV.RM.TEX8, 0.0, own), lambda s: AV.RM.resample(host, dims, rot, AV.RM.TEX8, 0.0, own, zbox(s)),
                     dims, host.dtype),
    }
    if not own:                                                 # u8 -> f32 of the last slices: an output just above 2^32 bytes
        zr = (1 << 32) // (nx * ny * 4) + 1
        assert (zr - 1) * nx * ny * 4 <= 1 << 32 < zr * nx * ny * 4 <= n and zr < nz
        calls["derive u8 -> f32"] = (lambda p, cap: ctx.derive_device(p, cap, zbox((nz - zr, nz)), 1, AV.DM.MEAN, AV.DM.F32),
                                     lambda s: AV.DM.derive(host, zbox(s, nz - zr), 1, AV.DM.MEAN, AV.DM.F32), (nx, ny, zr), np.dtype(np.float32))
    copies = {"derive": calls["derive"][0], "separable, radius 0": lambda p, cap: ctx.stencil_device(p, cap, AV.StM.SEPARABLE, None, own, (0, 0, 0)),
              "nearest, identity": lambda p, cap: ctx.resample_device(p, cap, dims, None, AV.RM.NEAREST, 0.0, own)}
    with MO.knobs(ctx, {}):
        V.prepare("linear")
        out = _BigOut(torch, n * size)
        wants = {name: [V.models.get(("outputs", name, s), lambda: c[1](s)) for s in _output_slabs(c[2], c[3].itemsize)] for name, c in calls.items()}

        def slabs_match(name, what):
            _, _, odims, dtype = calls[name]
            for s, want in zip(_output_slabs(odims, dtype.itemsize), wants[name]):
                got = out.slices(s[0], s[1], odims, dtype)
                assert len(np.unique(want)) >= 20, (what, s)
                VO.report(got, want, AV.DM.same(got, want), f"{V.name} {what}: output slices {s}")

        for name, (call, _, odims, dtype) in calls.items():
            out.run(call, odims[0] * odims[1] * odims[2] * dtype.itemsize, odims, f"{V.name} {name}")
            slabs_match(name, name)
        try:                                                    # (d)
            os.environ["VV_DERIVE_BLOCKS"] = os.environ["VV_STENCIL_BLOCKS"] = "4096"
            ctx.reread_env()
            for name in ("derive", "separable", "median"):
                out.run(calls[name][0], n * size, dims, f"{V.name} {name} under a grid cap of 4096")
                slabs_match(name, name + " under a grid cap of 4096")
        finally:
            os.environ.pop("VV_DERIVE_BLOCKS", None)
            os.environ.pop("VV_STENCIL_BLOCKS", None)
            ctx.reread_env()
        # (b) the source as Loaded made it, in a scratch tensor; the copies against it, 64 slices at a time
        tdev = torch.device("cuda", 0)
        src = torch.empty(n, dtype=torch.uint8, device=tdev)
        for z0, z1, seed in _noise_parts(dims):
            ctx.generate_noise_device(src.data_ptr() + z0 * ny * nx, nx, ny, z1 - z0, seed)
        if own:
            v8, src = src, torch.empty(n, dtype=torch.float32, device=tdev)
            ctx.promote_device(v8.data_ptr(), src.data_ptr(), n)
            torch.cuda.synchronize()
            del v8
        torch.cuda.synchronize()
        src = src.view(torch.int32) if own else src
        assert bool((src[:nx * ny] == torch.from_numpy(np.ascontiguousarray(host[0]).view(np.int32 if own else np.uint8).ravel().copy()).to(tdev)).all()), "the regenerated source"
        step = 64 * nx * ny
        for name, call in copies.items():
            out.run(call, n * size, dims, f"{V.name} {name}")
            got = out.tensor(n * size, torch.int32 if own else torch.uint8)
            bad = [a // (nx * ny) for a in range(0, n, step) if not torch.equal(got[a:a + step], src[a:a + step])]
            assert not bad, f"{V.name} {name}: the output is not the source in the slices from {bad[:8]} on (64 at a time; {len(bad)} such runs)"
        del src, out
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_label_box_of_more_than_2_to_31_voxels(ctx):
    """2047 x 2049 x 1023 voxels, a sparse foreground (addressing_volumes.wide_foreground): vv_label_volume's 32-bit parent pointers, its unsigned
    atomicMin, the division of indices in label_flatten_kernel and the stats key with indices and labels at and above 2^31, against the sparse model;
    then vv_mask_volume into 17 GB of f32.  Everything volume-sized stays on the device."""
    import torch
    dims = nx, ny, nz = AV.WIDE_DIMS
    n = nx * ny * nz
    assert 1 << 31 < n <= (1 << 32) - 2 and all(d % t for d, t in zip(dims, (16, 8, 8))) and (1 << 31) // (nx * ny) == 512
    tdev = torch.device("cuda", 0)
    free_b, total_b = torch.cuda.mem_get_info(tdev)
    if total_b < 100 * 2 ** 30:                                  # (Loaded's rule: only a physically smaller GPU model skips)
        pytest.skip(f"device has {total_b / 2 ** 30:.0f} GiB in all: not an MI355X-class GPU")
    assert free_b >= 60 * 2 ** 30, f"the wide label box needs 60 GiB of free HBM, the device reports {free_b / 2 ** 30:.1f} of {total_b / 2 ** 30:.0f} GiB free"
    idx, parts = AV.wide_foreground(**AV.WIDE)
    assert idx[-1] == n - 1 > (1 << 32) - (1 << 24)
    models = {conn: AV.sparse_label(idx, dims, conn) for conn in (6, 26)}
    for conn, m in models.items():
        _wide_conditions(idx, parts, m, AV.WIDE["half"], AV.WIDE["stairs"], conn)
    tf = _table()
    chunk = 64 * nx * ny                                        # 64 slices at a time: every torch call sees fewer than 2^31 elements
    cuts = np.searchsorted(idx, np.arange(0, n + chunk, chunk))
    at = [(a, torch.from_numpy(idx[cuts[i]:cuts[i + 1]] - a).to(tdev)) for i, a in enumerate(range(0, n, chunk))]       # per chunk: its foreground, relative

    def gathered(t):
        return torch.cat([t[a:a + chunk][rel] for a, rel in at]).cpu().numpy().view(np.uint32)

    def nonzero(t):
        return sum(int(torch.count_nonzero(t[a:a + chunk])) for a, _ in at)

    try:
        with MO.knobs(ctx, {}):
            v = torch.zeros(n, dtype=torch.uint8, device=tdev)
            for a, rel in at:
                v[a:a + chunk][rel] = WIDE_FG
            assert nonzero(v) == len(idx)
            ctx.load_volume_device(v.data_ptr(), vv.VOXEL_U8, nx, ny, nz, tf)
            torch.cuda.synchronize()
            del v
            torch.cuda.empty_cache()
            garbage = 0xA5A5A5A5 - (1 << 32)
            lab_t = torch.empty(n + 32, dtype=torch.int32, device=tdev)
            for blocks, conn in ((None, 6), (None, 26), ("4096", 6), ("4096", 26)):
                labels, sizes, stats = models[conn]
                what = f"connectivity {conn} VV_LABEL_BLOCKS={blocks}"
                if blocks is not None:
                    os.environ["VV_LABEL_BLOCKS"] = blocks
                ctx.reread_env()
                siz_t = torch.empty(n + 32, dtype=torch.int32, device=tdev)
                st_t = torch.full((6,), -1, dtype=torch.int64, device=tdev)
                lab_t.fill_(garbage); siz_t.fill_(garbage)
                torch.cuda.synchronize()
                lab, siz = lab_t[16:16 + n], siz_t[16:16 + n]
                assert ctx.label_device(lab.data_ptr(), n * 4, (WIDE_FG, WIDE_FG), conn, sizes_ptr=siz.data_ptr(), stats_ptr=st_t.data_ptr() + 8) == dims
                torch.cuda.synchronize()
                for t in (lab_t, siz_t):
                    assert bool((t[:16] == garbage).all()) and bool((t[16 + n:] == garbage).all()), f"words outside the output were written ({what})"
                assert nonzero(lab) == len(idx) and nonzero(siz) == stats[1], (what, nonzero(lab), nonzero(siz), stats)
                got_l, got_s = gathered(lab), gathered(siz)
                bad = np.flatnonzero(got_l != labels)
                assert len(bad) == 0, f"{what}: {len(bad)} labels differ, first at index {idx[bad[0]]}: {got_l[bad[0]]} vs {labels[bad[0]]}"
                bad = np.flatnonzero(got_s != sizes)
                assert len(bad) == 0, f"{what}: {len(bad)} sizes differ, first at index {idx[bad[0]]}: {got_s[bad[0]]} vs {sizes[bad[0]]}"
                st = st_t.cpu().numpy()
                got = vv.LabelStats.from_bytes(st[1:5].tobytes())
                assert st[0] == -1 and st[5] == -1 and (got.foreground, got.components, got.largest_size, got.largest_label, got.reserved) == stats, (what, got, stats)
                os.environ.pop("VV_LABEL_BLOCKS", None)
                if blocks is None and conn == 6:                 # the mask, fed the labels and sizes of this call (under 6 the staircase's voxels are components of one)
                    wire = int(labels[np.searchsorted(idx, parts["wire"][0])])
                    assert wire == stats[3]
                    count = np.bincount(np.searchsorted(idx, labels.astype(np.int64) - 1), minlength=len(idx))      # per listed voxel: its component's size
                    comp = count[np.searchsorted(idx, labels.astype(np.int64) - 1)]
                    keeps = (("KEEP_LABEL", dict(keep=vv.KEEP_LABEL, label=wire), labels == wire), ("KEEP_MIN_SIZE", dict(keep=vv.KEEP_MIN_SIZE, min_size=2), comp >= 2))
                    out_t = torch.empty(n + 32, dtype=torch.float32, device=tdev)
                    kept_bits = LM.copy_stage(np.full(1, WIDE_FG, np.uint8), LM.F32).view(np.uint32)[0]         # 200 / 255 as binary32
                    fill_bits = int(LM.fill_stage(0.25, np.uint8, LM.F32).reshape(1).view(np.uint32)[0])          # rule M2: the fill is in storage units, 0.25 / 255
                    assert kept_bits == (np.float32(WIDE_FG) / np.float32(255)).view(np.uint32) and fill_bits == int((np.float32(0.25) / np.float32(255)).view(np.uint32))
                    for kname, kw, keep in keeps:
                        assert 0 < keep.sum() < len(idx), kname
                        out_t.view(torch.int32).fill_(garbage)
                        torch.cuda.synchronize()
                        o = out_t[16:16 + n]
                        assert ctx.mask_device(o.data_ptr(), n * 4, lab.data_ptr(), sizes_ptr=siz.data_ptr(), fill=0.25, out_type=vv.VOXEL_F32, **kw) == dims
                        torch.cuda.synchronize()
                        ob = out_t.view(torch.int32)
                        assert bool((ob[:16] == garbage).all()) and bool((ob[16 + n:] == garbage).all()), f"words outside the mask output were written ({kname})"
                        ob = ob[16:16 + n]
                        other = sum(int(torch.count_nonzero(ob[a:a + chunk] != fill_bits)) for a, _ in at)
                        got_o = gathered(ob)
                        assert other == int(keep.sum()) and np.array_equal(got_o, np.where(keep, kept_bits, np.uint32(fill_bits))), \
                            (kname, other, int(keep.sum()), [hex(v) for v in got_o[:4]], [hex(int(v)) for v in ob[:4].cpu().numpy().view(np.uint32)])
                    del out_t, o, ob
                del siz_t, siz
                torch.cuda.empty_cache()
    finally:
        os.environ.pop("VV_LABEL_BLOCKS", None)
        with MO.knobs(ctx, {}):
            ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)
