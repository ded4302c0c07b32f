"""Projection frames (vv_render_projection) against tests/proj_model.py, the numpy statement of the contract in include/volviz.h.

The model is itself held to what exists: its MAX index image is the witness's MIP image, its executed count the witness's and the
oracle's, and single rays are restated once more in plain Python, sample by sample.  Every comparison below is exact and no pixel
is excluded."""
import ctypes as C
import functools
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest

import mip_oracle as MO
import oracle_lib as O
import proj_model as PM
import volviz_amd as vv
import witness as Wt
from test_mip_geometry import RECT_CAMS, RECT_OFF_SCREEN, RECT_SIZES, _rect_volume

HERE = os.path.dirname(os.path.abspath(__file__))
CAM_A = vv.Camera.orbit(3.0, 1.0, 0.6)
CAM_B = vv.Camera.orbit(1.2, 1.3, 2.0)
CAMS = {"camA": CAM_A, "camB": CAM_B}
CUT = dict(point=(.5, .5, .5), normal=(.3, .2, 1.))            # mip_oracle's / test_mip's cut plane
LAYOUT_KNOBS = ("VV_BRICKED", "VV_ZPAIR", "VV_ZFAST", "VV_FORCE_BIG", "VV_UNROLL")
ENVS = ({}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}, {"VV_ZFAST": "1"}, {"VV_FORCE_BIG": "1"}, {"VV_UNROLL": "2"})      # test_iso.py's knob sets
ZFAST_ONLY = {"VV_ZFAST": "1", "VV_ZPAIR": "0"}            # the z-fastest build itself: VV_ZFAST=1 alone takes the x-pair copy built from it
FILL = 0x5A
ANISO_SCALE = (1.57, 1.0, 1.0)
ERR_INVALID, ERR_NO_VOLUME = -1, -2                        # include/volviz.h: vv_status
MODES = (PM.PROJ_MAX, PM.PROJ_MIN, PM.PROJ_MEAN)
MODE_IDS = ("max", "min", "mean")


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name == "brain64":
        v = O.draw_default_brain(64, 64, 64)
    elif name == "noise_u8":
        v = O.noise_u8(48, 40, 56, 3)
    elif name == "aniso":
        v = np.fromfile(os.path.join(HERE, "golden", "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
    elif name == "probe":                                   # uniform bytes: every ray's minimum, mean and maximum lie far apart
        v = np.random.default_rng(3).integers(0, 256, (56, 40, 48), np.uint8)
    elif name == "blocks":                                  # constant blocks: samples of exactly 255 and exactly 0 inside the volume (the early drop of MAX / MIN)
        v = O.noise_u8(48, 40, 56, 3).copy()
        v[8:30, 6:30, 8:40] = 255
        v[36:52, :, :] = 0
    else:
        assert name == "noise_f32"
        v = np.ascontiguousarray((O.noise_u8(40, 40, 40, 5).astype(np.float32) / np.float32(255)) ** 2, np.float32)
    v.setflags(write=False)
    return v


def _scaled(cam, scale):
    return vv.Camera(origin=cam.origin, look_at=cam.look_at, up=cam.up, fov_y=cam.fov_y, scale=scale)


def _colour_table(seed=7):
    # entries outside [0, 1] too: the conversion clamps
    return np.random.default_rng(seed).uniform(-0.3, 1.4, 1024).astype(np.float32)


def _freeze(m):
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def _model(vol, tf, W, H, cam, mode, *, stype=vv.SLICE_NONE, step=None, filt=vv.FILTER_TEX8, images=None, slab_rows=(0, 0), shard=None,
           fill=FILL):
    return PM.render_cam(vol, tf, W, H, cam, mode, slice_type=stype, plane=(*CUT["point"], *CUT["normal"]), step=step, filt=filt,
                         images=images, slab_rows=slab_rows, shard=shard, fill=fill)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _same_triple(got, m, what):
    rgba, idx, stat = got
    _same(idx, m["index"], f"{what}: index image")
    _same(stat, m["stat"], f"{what}: stat records")
    _same(rgba, m["rgba"], f"{what}: rgba")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_projection():
    for name in ("render_projection", "render_projection_device"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert "vv_render_projection" in vv.EXPORTS and hasattr(vv.load_library(), "vv_render_projection")
    assert (vv.PROJ_MAX, vv.PROJ_MIN, vv.PROJ_MEAN) == (0, 1, 2) == MODES


# test_iso.py's 8 frames (4 volumes x 2 cameras, 99 x 71), and the uniform-bytes volume under the first camera
CPU_FRAMES = [(v, c) for v in ("noise_u8", "brain64", "noise_f32", "aniso") for c in ("camA", "camB")] + [("probe", "camA")]
CPU_IDS = [f"{v}-{c}" for v, c in CPU_FRAMES]
CPU_W, CPU_H = 99, 71


def _cpu_cam(name, cam_id):
    return _scaled(CAMS[cam_id], ANISO_SCALE) if name == "aniso" else CAMS[cam_id]


@functools.lru_cache(maxsize=None)
def _cpu_frame(name, cam_id):
    """The three 99 x 71 frames of the model (MAX, MIN, MEAN): computed once, shared, read-only."""
    vol = _volume(name)
    cam = _cpu_cam(name, cam_id)
    tf = _colour_table()
    return vol, cam, tf, tuple(_freeze(_model(vol, tf, CPU_W, CPU_H, cam, mode, fill=0)) for mode in MODES)


@pytest.mark.parametrize("name,cam_id", CPU_FRAMES, ids=CPU_IDS)
def test_model_max_is_the_mip_frame_and_counts_agree(name, cam_id):
    vol, cam, tf, (mx, mn, me) = _cpu_frame(name, cam_id)
    rgba, M, count = Wt.render(vol, tf, CPU_W, CPU_H, cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y, scale=cam.scale, mip=True)
    n_oracle = MO.executed_samples(vol, CPU_W, CPU_H, cam)
    print(f"{name} {cam_id}: model count {mx['count']}, witness {count}, oracle {n_oracle}")
    _same(mx["index"], M, "the model's MAX index image against the witness's MIP image")
    _same(mx["rgba"], rgba, "the model's MAX rgba against the witness's MIP rgba")
    for m in (mx, mn, me):
        assert m["count"] == count == n_oracle == int(m["e"].sum())
        assert np.array_equal(m["e"], mx["e"]) and np.array_equal(m["n"], mx["n"]) and np.array_equal(m["written"], mx["written"])
        _same(m["stat"][..., 1], mx["n"].astype(np.uint32), "the second word is n")
    assert not mx["written"][-1].any() and not mx["written"][:, -1].any() and mx["written"][:-1, :-1].all()


@pytest.mark.parametrize("name,cam_id", CPU_FRAMES, ids=CPU_IDS)
def test_model_invariants(name, cam_id):
    _, _, tf, (mx, mn, me) = _cpu_frame(name, cam_id)
    e, n = mx["e"], mx["n"]
    has = n > 0
    assert (n <= e).all() and (e[~mx["written"]] == 0).all()
    s = me["stat"][..., 0].astype(np.int64)
    assert (s <= 255 * n).all()
    vmax, vmin, vmean = (m["index"].astype(np.int64) for m in (mx, mn, me))
    assert (vmin[has] <= vmean[has]).all() and (vmean[has] <= vmax[has]).all()
    for m in (mx, mn):
        o = m["stat"][..., 0].astype(np.int64)
        assert (o[has] >= 1).all() and (o[has] <= e[has]).all()
    for m in (mx, mn, me):
        assert (m["index"][~has] == 0).all() and (m["stat"][..., 0][~has] == 0).all()
        _same(m["rgba"][m["written"]], MO.rgba_of(tf, m["index"])[m["written"]], "rgba is the table's entry v, converted")
    share = has.sum() / mx["written"].sum()
    print(f"{name} {cam_id}: n > 0 on {share:.3f} of the written pixels")
    assert share >= 0.25


def test_model_frames_are_not_vacuous():
    """Conditions on the model alone, over the CPU frames taken together: every class of pixel the contract distinguishes is there."""
    outside_only = partly = all_inside = tied = differ = between = 0
    for name, cam_id in CPU_FRAMES:
        (mx, mn, me) = _cpu_frame(name, cam_id)[3]
        e, n = mx["e"], mx["n"]
        outside_only += int(((e > 0) & (n == 0)).sum())
        partly += int(((n > 0) & (n < e)).sum())
        all_inside += int(((n == e) & (e > 0)).sum())
        tied += int((mx["ties"] > 1).sum()) + int((mn["ties"] > 1).sum())
        differ += int((mx["index"] != mn["index"]).sum())
        between += int(((me["index"] != mx["index"]) & (me["index"] != mn["index"])).sum())
    print(f"e > 0 = n: {outside_only}, 0 < n < e: {partly}, n = e > 0: {all_inside}, tied extrema: {tied}, MIN != MAX: {differ}, MEAN apart: {between}")
    assert min(outside_only, partly, all_inside, tied, differ, between) > 0
    mn, me = _cpu_frame("probe", "camA")[3][1:]
    assert len(np.unique(mn["index"])) >= 100 and len(np.unique(me["index"])) >= 100


# ---- single rays once more, in plain Python: binary32 by numpy scalars, the fused multiply-add by exact rationals ----
def _round32(x):
    """A rational to the nearest binary32 (ties to even), returned as np.float32."""
    if x == 0:
        return np.float32(0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    ex = x.numerator.bit_length() - x.denominator.bit_length() - 24
    while x >= Fraction(2) ** (ex + 24):
        ex += 1
    while x < Fraction(2) ** (ex + 23):
        ex -= 1
    ex = max(ex, -149)
    q = x / Fraction(2) ** ex
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m % 2 == 1):
        m += 1
    return np.float32(sign * m * 2.0 ** ex)


def _fma(a, b, c):
    return _round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _scalar_index(vol, t, filt):
    """(k, inside) of one sample at texture coordinates t = (tx, ty, tz), np.float32 each."""
    one, zero = np.float32(1), np.float32(0)
    inside = all(zero <= c < one for c in t)
    dims = vol.shape[::-1]
    lo, hi, w = [], [], []
    for c, n in zip(t, dims):
        xb = _fma(c, np.float32(n), np.float32(-0.5))
        fl = np.floor(xb)
        wt = np.float32(xb - fl)
        if filt == vv.FILTER_TEX8:
            wt = np.float32(round(float(wt) * 256.0)) * np.float32(1.0 / 256.0)        # (round: ties to even)
        i = int(fl)
        lo.append(min(max(i, 0), n - 1)); hi.append(min(max(i + 1, 0), n - 1)); w.append(wt)
    def vox(z, y, x):
        return np.float32(vol[z, y, x])
    def lerp(wt, a, b):
        return _fma(wt, np.float32(b - a), a)
    lz = []
    for z in (lo[2], hi[2]):
        ly = [lerp(w[0], vox(z, y, lo[0]), vox(z, y, hi[0])) for y in (lo[1], hi[1])]
        lz.append(lerp(w[1], ly[0], ly[1]))
    L = lerp(w[2], lz[0], lz[1])
    if vol.dtype != np.uint8:
        L = np.float32(255) * L
    k = int(min(float(L), 255.0)) if L > 0 else 0
    return (k if inside else 0), inside


def _scalar_ray(vol, ray, inv_scale, filt):
    """(k, counted) of every executed sample of one ray, in march order."""
    if ray["dead"] or ray["cut"]:
        return []
    out = []
    dist, upper, sstep = ray["dist0"], ray["upper"], ray["sstep"]
    thirty = np.float32(30)
    while dist < upper:
        p = [np.float32(ray["origin"][a] + np.float32(ray["dir"][a] * dist)) for a in range(3)]
        for i in range(1, 31):
            p = [np.float32(p[a] + ray["sdir"][a]) for a in range(3)]
            if np.float32(np.float32(np.float32(i) * sstep) + dist) > upper:
                break
            t = [_fma(np.float32(p[a] - np.float32(0.5)), inv_scale[a], np.float32(0.5)) for a in range(3)]
            out.append(_scalar_index(vol, t, filt))
        dist = np.float32(dist + np.float32(sstep * thirty))
    return out


@pytest.mark.parametrize("name,cam_id", CPU_FRAMES, ids=CPU_IDS)
def test_model_against_single_rays_in_plain_python(name, cam_id):
    vol, cam, _, models = _cpu_frame(name, cam_id)
    W, H = CPU_W, CPU_H
    R = Wt.frame_rays(W, H)
    front, back = Wt.analytic_endpoints(W, H, R["x"], R["y"], cam.origin, cam.look(), cam.up, cam.fov_y, cam.scale, 0.0, False)
    nz, ny, nx = vol.shape
    Wt.setup(R, front, back, cam.origin, np.float32(1) / np.array([nx, ny, nz], np.float32), Wt.SLICE_NONE, (.5, .5, .5, 0, 0, 1))
    inv_scale = np.float32(1) / np.asarray(cam.scale, np.float32)
    owned = np.flatnonzero(R["owned"])
    e_img = models[0]["e"]
    marching = owned[e_img[R["y"][owned], R["x"][owned]] > 0]
    rng = np.random.default_rng(20)
    picks = list(rng.choice(marching, 36, replace=False)) + list(rng.choice(owned, 8, replace=False))
    # ... and rays the model says execute samples but count none, where the frame has them
    lost = marching[models[0]["n"][R["y"][marching], R["x"][marching]] == 0]
    picks += list(lost[:4])
    assert len(picks) >= 40
    for j in picks:
        ray = {k: R[k][j] for k in ("origin", "dir", "sdir", "sstep", "upper", "dist0", "dead", "cut")}
        samples = _scalar_ray(vol, ray, inv_scale, vv.FILTER_TEX8)
        y, x = int(R["y"][j]), int(R["x"][j])
        inside = [k for k, c in samples if c]
        e, n = len(samples), len(inside)
        assert (e, n) == (int(e_img[y, x]), int(models[0]["n"][y, x])), (name, cam_id, x, y)
        for mode, m in zip(MODES, models):
            if n == 0:
                want = (0, 0, 0)
            elif mode == PM.PROJ_MEAN:
                s = sum(inside)
                want = ((2 * s + n) // (2 * n), s, n)
            else:
                v = max(inside) if mode == PM.PROJ_MAX else min(inside)
                ordinal = next(i + 1 for i, (k, c) in enumerate(samples) if c and k == v)
                assert samples[ordinal - 1] == (v, True) and 1 <= ordinal <= e
                want = (v, ordinal, n)
            got = (int(m["index"][y, x]), int(m["stat"][y, x, 0]), int(m["stat"][y, x, 1]))
            assert got == want, f"{name} {cam_id} pixel ({x}, {y}) mode {mode}: model {got}, single ray {want}"


def test_mean_rounds_half_up():
    assert PM.mean_half_up([0, 1, 3, 5, 255 * 7, 10], [0, 2, 2, 2, 7, 4]).tolist() == [0, 1, 2, 3, 255, 3]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _set_env(monkeypatch, env):
    for k in LAYOUT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _forced_layout(env, default):
    if env.get("VV_ZFAST") == "1":
        return 4 if env.get("VV_ZPAIR") == "0" else 5
    for knob, code in (("VV_BRICKED", 2), ("VV_ZPAIR", 3), ("VV_FORCE_BIG", 1)):
        if env.get(knob) == "1":
            return code
    return default


def _proj(ctx, W, H, cam, mode, fill=FILL, **kw):
    return ctx.render_projection(W, H, cam, mode, fill=fill, return_index=True, return_stat=True, **kw)


# (name, volume, camera, W, H, filter, step, envs, the layout the policy itself picks (None: forced layouts are not checked)): both voxel types, both
# filters, a non-unit object scale, non-default steps, a width of 1 mod 14
PARITY = [
    ("u8-tex8",        "noise_u8",  CAM_A, 99, 71, vv.FILTER_TEX8,  None,   ENVS + (ZFAST_ONLY,), 0),
    ("f32-exact",      "noise_f32", CAM_B, 99, 71, vv.FILTER_EXACT, None,   ENVS + (ZFAST_ONLY,), 0),
    ("blocks-1mod14",  "blocks",    CAM_A, 85, 57, vv.FILTER_TEX8,  None,   ENVS + (ZFAST_ONLY,), 0),
    ("f32-axis-step-scale", "noise_f32", vv.Camera(origin=(0.0, 0.0, -3.0), scale=(1.0, 0.8, 1.2)), 90, 67, vv.FILTER_TEX8, 1 / 50,
     ({}, {"VV_ZPAIR": "1"}, {"VV_ZPAIR": "0", "VV_FORCE_BIG": "1"}, {"VV_ZPAIR": "0", "VV_UNROLL": "2"}, {"VV_BRICKED": "1"}, ZFAST_ONLY), None),
    ("u8-axis-exact",  "noise_u8",  vv.Camera(origin=(0.3, 0.2, -3.0)), 86, 57, vv.FILTER_EXACT, (1 / 40, 1 / 70, 1 / 33), ({}, {"VV_ZPAIR": "0"}, {"VV_FORCE_BIG": "1", "VV_ZPAIR": "0"}), None),
    ("aniso-scale",    "aniso",     _scaled(CAM_A, ANISO_SCALE), 99, 71, vv.FILTER_TEX8, None, ENVS + (ZFAST_ONLY,), None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_projection_matches_model_on_every_build(ctx, case, mode, monkeypatch):
    """All three images against the model on every layout build with both trip lengths; an instrumented frame holds the same images and counts
    the model's executed samples; without a stat image (MAX / MIN may then drop rays early) the other two are the same; MAX is the MIP frame."""
    _, name, cam, W, H, filt, step, envs, policy_layout = case
    vol = _volume(name)
    okw = dict(filter=filt)
    if step is not None:
        okw["step"] = step
    tf = _colour_table()
    m = _model(vol, tf, W, H, cam, mode, step=step, filt=filt)
    has = m["n"] > 0
    print(f"{case[0]} mode {mode}: n > 0 on {int(has.sum())} pixels, model count {m['count']}, {len(np.unique(m['index'][has]))} values")
    # (the minimum over a phantom with an empty background is 0 wherever n > 0: there the ordinals carry the variety)
    assert has.sum() >= 0.25 * m["written"].sum()
    assert len(np.unique(m["index"][has])) >= 20 or (mode == PM.PROJ_MIN and len(np.unique(m["stat"][..., 0][has])) >= 15)
    assert (m["index"][~m["written"]] == FILL).all() and m["written"][:-1, :-1].all() and m["written"].sum() == (W - 1) * (H - 1)
    if name == "blocks" and mode != PM.PROJ_MEAN:
        assert (m["index"][has] == (255 if mode == PM.PROJ_MAX else 0)).sum() >= 100, "no ray reaches the value at which the early drop fires"
    layouts = set()
    for env in envs:
        for unroll in ((env["VV_UNROLL"],) if "VV_UNROLL" in env else ("2", "3")):
            full = dict(env, VV_UNROLL=unroll)
            _set_env(monkeypatch, full)
            ctx.load_volume(vol, tf)                    # (the knobs are read at volume load)
            got = _proj(ctx, W, H, cam, mode, options=vv.make_options(**okw))
            lay = ctx.last_launch()
            _same_triple(got, m, f"{case[0]} mode {mode} {full}")
            assert lay["phong"] == 4, lay                 # a projection launch was reported
            assert lay["unroll"] == int(unroll), lay
            layouts.add(lay["layout"])
            if policy_layout is not None:
                assert lay["layout"] == _forced_layout(env, policy_layout), (env, lay)
            counted = _proj(ctx, W, H, cam, mode, options=vv.make_options(count_samples=True, **okw))
            n = ctx.last_sample_count()
            _same_triple(counted, m, f"{case[0]} mode {mode} {full}, instrumented")
            assert n == m["count"], f"{case[0]} mode {mode} {full}: {n} samples counted, the model executes {m['count']}"
            rgba, idx = ctx.render_projection(W, H, cam, mode, fill=FILL, return_index=True, options=vv.make_options(**okw))
            _same(idx, m["index"], f"{case[0]} mode {mode} {full}, no stat image: index image")
            _same(rgba, m["rgba"], f"{case[0]} mode {mode} {full}, no stat image: rgba")
            if mode == PM.PROJ_MAX:
                mip_rgba, mip_idx = ctx.render_mip(W, H, cam, fill=FILL, return_index=True, options=vv.make_options(**okw))
                _same(idx, mip_idx, f"{case[0]} {full}: VV_PROJ_MAX index image against vv_render_mip's")
                _same(rgba, mip_rgba, f"{case[0]} {full}: VV_PROJ_MAX rgba against vv_render_mip's")
    if policy_layout is not None:
        assert layouts == {0, 1, 2, 3, 4, 5}, layouts           # every kernel build, for this voxel type


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_projection_cut_plane(ctx, mode, monkeypatch):
    vol = _volume("brain64")
    tf = _colour_table(11)
    W, H = 99, 71
    frames = {}
    for stype in (vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT):
        sp = vv.make_slice_params(stype, **CUT)
        m = _model(vol, tf, W, H, CAM_A, mode, stype=stype, fill=3)
        assert (m["n"] > 0)[m["written"]].mean() >= 0.10
        for env in ({}, {"VV_BRICKED": "1"}, {"VV_FORCE_BIG": "1"}):
            _set_env(monkeypatch, env)
            ctx.load_volume(vol, tf)
            got = _proj(ctx, W, H, CAM_A, mode, fill=3, slice=sp, options=vv.make_options(count_samples=True))
            _same_triple(got, m, f"slice type {stype} {env}")
            assert ctx.last_sample_count() == m["count"]
        frames[stype] = (got, m)
    for a, b in zip(frames[vv.SLICE_PLANE][0], frames[vv.SLICE_NONE][0]):
        _same(a, b, "SLICE_PLANE marches as SLICE_NONE")
    cut, none = frames[vv.SLICE_PLANE_CUT][1], frames[vv.SLICE_NONE][1]
    assert cut["count"] < none["count"] and not np.array_equal(cut["stat"], none["stat"])
    assert ((cut["e"] == 0) & (none["e"] > 0)).any(), "no ray takes the cut plane's early return"


@pytest.mark.gpu
def test_projection_image_ray_source(ctx, monkeypatch):
    """End points read from first-pass images at 3 x the frame (point-sampled, UNORM8)."""
    _set_env(monkeypatch, {})
    vol = _volume("noise_u8")
    tf = _colour_table(5)
    ctx.load_volume(vol, tf)
    W, H = 90, 62
    front, back = ctx.first_pass(3 * W, 3 * H, CAM_B)
    of, ob = O.first_pass(CAM_B, 3 * W, 3 * H)
    assert np.array_equal(front, of) and np.array_equal(back, ob)
    rays = vv.image_rays(front, back)
    for mode in MODES:
        m = _model(vol, tf, W, H, CAM_B, mode, images=(front, back), fill=0xEE)
        assert (m["n"] > 0).mean() >= 0.25 and m["count"] == MO.executed_samples(vol, W, H, CAM_B, rays=rays)
        for r in (rays, vv.image_rays(front, back, hint=CAM_B)):
            got = _proj(ctx, W, H, CAM_B, mode, fill=0xEE, rays=r, options=vv.make_options(count_samples=True))
            _same_triple(got, m, f"image rays, mode {mode}")
            assert ctx.last_sample_count() == m["count"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_projection_shards_and_slab_rows(ctx, mode, monkeypatch):
    """Rows of other shards and outside the slab-row window keep the fill in all three images; the shards' union is the whole frame."""
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = _colour_table(3)
    ctx.load_volume(vol, tf)
    W, H = 57, 141                                   # 11 slab rows: bands of 4 -> 3 bands
    whole = _model(vol, tf, W, H, CAM_A, mode, fill=0x77)
    full = _proj(ctx, W, H, CAM_A, mode, fill=0x77)
    _same_triple(full, whole, "unsharded")
    union = [np.full_like(a, 0) for a in full]
    for a in union:
        a.view(np.uint8)[...] = 0x77
    covered = np.zeros((H, W), bool)
    for i in range(2):
        m = _model(vol, tf, W, H, CAM_A, mode, shard=(4, 2, i), fill=0x77)
        assert m["written"].any() and not (m["written"] & covered).any()
        got = _proj(ctx, W, H, CAM_A, mode, fill=0x77, options=vv.make_options(shard=(4, 2, i)))
        _same_triple(got, m, f"shard {i} of 2")
        for u, g in zip(union, got):
            u[m["written"]] = g[m["written"]]
        covered |= m["written"]
    assert np.array_equal(covered, whole["written"])
    for u, f, what in zip(union, full, ("rgba", "index image", "stat records")):
        _same(u, f, f"union of 2 shards: {what}")
    m = _model(vol, tf, W, H, CAM_A, mode, slab_rows=(2, 7), fill=0x11)
    assert m["written"][28:98, :-1].all() and m["written"].sum() == 70 * (W - 1)
    got = _proj(ctx, W, H, CAM_A, mode, fill=0x11, options=vv.make_options(slab_rows=(2, 7)))
    _same_triple(got, m, "slab rows 2..7")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 29), (31, 1)])
def test_projection_frames_one_pixel_wide_or_high(ctx, W, H, monkeypatch):
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = _colour_table(13)
    ctx.load_volume(vol, tf)
    cam = vv.Camera(origin=(0.2, 0.1, -3.0))
    for mode in MODES:
        m = _model(vol, tf, W, H, cam, mode)
        assert m["written"][:H - 1 if H > 1 else 1, :W - 1 if W > 1 else 1].all() and m["written"].sum() == max(W - 1, 1) * max(H - 1, 1)     # the lone column / row is written, but for its last pixel
        assert (m["n"] > 0).any()
        got = _proj(ctx, W, H, cam, mode, options=vv.make_options(count_samples=True))
        _same_triple(got, m, f"{W} x {H} mode {mode}")
        assert ctx.last_sample_count() == m["count"] > 0
        _same_triple(_proj(ctx, W, H, cam, mode), m, f"{W} x {H} mode {mode}, uninstrumented")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_projection_output_subsets_device_outputs_and_instruments(ctx, mode, monkeypatch):
    import torch
    _set_env(monkeypatch, {})
    vol = _volume("blocks")
    tf = _colour_table(4)
    ctx.load_volume(vol, tf)
    W, H = 96, 71
    m = _model(vol, tf, W, H, CAM_B, mode, fill=0x42)
    want = (m["rgba"], m["index"], m["stat"])
    names = ("rgba", "index image", "stat records")
    assert (m["n"] > 0).mean() >= 0.25 and len(np.unique(np.ascontiguousarray(m["stat"][m["n"] > 0]).view(np.uint64))) >= 15
    lib, h = ctx.lib, ctx.h
    sp = vv.make_slice_params(); cp = CAM_B.params(W, H); rs = vv.analytic_rays(CAM_B)
    # every non-empty subset of the three outputs, host buffers
    for r in (1, 2, 3):
        for subset in itertools.combinations(range(3), r):
            bufs = [np.full((H, W, 4), 0x42, np.uint8), np.full((H, W), 0x42, np.uint8), np.full((H, W, 8), 0x42, np.uint8).view(np.uint32)]
            ptrs = [bufs[i].ctypes.data if i in subset else None for i in range(3)]
            assert lib.vv_render_projection(h, W, H, C.byref(sp), C.byref(cp), C.byref(rs), None, mode, ptrs[0], ptrs[1], ptrs[2], 0, None) == 0
            for i in subset:
                _same(bufs[i], want[i], f"outputs {[names[j] for j in subset]}: {names[i]}")
    # device pointers, enqueue-only on a torch stream and synchronous; every subset once more
    dev = torch.device("cuda", 0)
    for ts in (torch.cuda.Stream(device=dev), torch.cuda.default_stream(dev)):
        for r in (1, 2, 3):
            for subset in itertools.combinations(range(3), r):
                d = [torch.full((H, W, 4), 0x42, dtype=torch.uint8, device=dev), torch.full((H, W), 0x42, dtype=torch.uint8, device=dev),
                     torch.full((H, W, 8), 0x42, dtype=torch.uint8, device=dev)]
                ptrs = [d[i].data_ptr() if i in subset else 0 for i in range(3)]
                torch.cuda.synchronize()
                with torch.cuda.stream(ts):
                    ctx.render_projection_device(W, H, CAM_B, mode, *ptrs, stream=vv.stream_handle(ts))
                ts.synchronize()
                got = [d[0].cpu().numpy(), d[1].cpu().numpy(), d[2].cpu().numpy().view(np.uint32)]
                for i in range(3):
                    _same(got[i], want[i] if i in subset else np.full_like(want[i].view(np.uint8), 0x42).view(want[i].dtype),
                          f"device outputs {[names[j] for j in subset]}: {names[i]}")
    d_stat = torch.full((H, W, 8), 0x42, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.render_projection_device(W, H, CAM_B, mode, 0, 0, d_stat.data_ptr())
    _same(d_stat.cpu().numpy().view(np.uint32), want[2], "stat records alone, device, the context's stream")
    # instrumented frames: the same three images, the model's executed count
    nb = [(s + 7) // 8 for s in vol.shape]
    bricks = torch.zeros((nb[0] * nb[1] * nb[2] + 31) // 32, dtype=torch.int32, device=dev)
    lines = torch.zeros(4096, dtype=torch.int32, device=dev)
    for okw in (dict(count_samples=True), dict(touched_bricks=bricks.data_ptr()),
                dict(touched_lines=lines.data_ptr(), touched_line_bits=4096 * 32, touched_lines_all=True)):
        _same_triple(_proj(ctx, W, H, CAM_B, mode, fill=0x42, options=vv.make_options(**okw)), m, f"instrumented {sorted(okw)}")
        assert ctx.last_sample_count() == m["count"]
    assert int(bricks.count_nonzero()) > 0 and int(lines.count_nonzero()) > 0
    assert ctx.last_frame_ms() > 0.0


@pytest.mark.gpu
def test_projection_leaves_the_context_alone_and_reports_errors(ctx, monkeypatch):
    import torch
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    W, H = 99, 71
    want_mip = ctx.render_mip(W, H, CAM_A, fill=1, return_index=True)

    def still_usable():
        got = ctx.render_mip(W, H, CAM_A, fill=1, return_index=True)
        _same(got[0], want_mip[0], "vv_render_mip after the call: rgba")
        _same(got[1], want_mip[1], "vv_render_mip after the call: index image")

    for phong in (False, True):
        before = ctx.render(W, H, CAM_A, phong=phong, fill=1)
        want, _ = O.render(vol, tf, W, H, CAM_A, phong=phong, fill=1)
        assert np.array_equal(before, want)
        state = ctx.layout_state()
        for mode in MODES:
            _proj(ctx, W, H, CAM_A, mode)
            ctx.render_projection(W, H, CAM_B, mode, slice=vv.make_slice_params(vv.SLICE_PLANE_CUT, **CUT), options=vv.make_options(count_samples=True))
        assert ctx.layout_state() == state
        after = ctx.render(W, H, CAM_A, phong=phong, fill=1)
        assert np.array_equal(after, before), f"phong={phong}"          # the volume and the table are the ones loaded
    lib, h = ctx.lib, ctx.h
    sp = vv.make_slice_params(); cp = CAM_A.params(W, H); rs = vv.analytic_rays(CAM_A)
    out = np.zeros((H, W, 4), np.uint8)
    args = dict(ctx=h, slice=C.byref(sp), cam=C.byref(cp), rays=C.byref(rs))
    for missing in ("ctx", "slice", "cam", "rays"):
        a = dict(args); a[missing] = None
        assert lib.vv_render_projection(a["ctx"], W, H, a["slice"], a["cam"], a["rays"], None, 0, out.ctypes.data, None, None, 0, None) == ERR_INVALID, missing
        still_usable()
    for mode in (-1, 3, 255):
        with pytest.raises(vv.VolvizError) as e:
            ctx.render_projection(W, H, CAM_A, mode)
        assert e.value.code == ERR_INVALID
        still_usable()
    with pytest.raises(vv.VolvizError) as e:
        ctx.render_projection_device(W, H, CAM_A, vv.PROJ_MIN, 0, 0, 0)
    assert e.value.code == ERR_INVALID
    still_usable()
    d_stat = torch.zeros(W * H * 8 + 16, dtype=torch.uint8, device=torch.device("cuda", 0))
    with pytest.raises(vv.VolvizError) as e:
        ctx.render_projection_device(W, H, CAM_A, vv.PROJ_MEAN, 0, 0, d_stat.data_ptr() + 4)
    assert e.value.code == ERR_INVALID
    still_usable()
    with vv.Context(0) as empty:
        with pytest.raises(vv.VolvizError) as e:
            empty.render_projection(W, H, CAM_A, vv.PROJ_MAX)
        assert e.value.code == ERR_NO_VOLUME
    still_usable()
    m = _model(vol, tf, W, H, CAM_A, PM.PROJ_MIN)
    _same_triple(_proj(ctx, W, H, CAM_A, PM.PROJ_MIN), m, "a projection frame after the failed calls")
    assert np.array_equal(ctx.render(W, H, CAM_A, fill=1), O.render(vol, tf, W, H, CAM_A, fill=1)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the screen rectangle and the fill beside it (fill_outside_kernel, shared with the MIP and isosurface frames): test_mip_geometry's frames
# ---------------------------------------------------------------------------------------------------------------------
RECT_CIS = (0, 1, RECT_OFF_SCREEN)               # cube partly off the left edge, partly off the bottom, wholly off the screen
RECT_MIN_COUNTED_SHARE = {0: 0.25, 1: 0.03}      # n > 0, of the (W-1) x (H-1) pixels; the model gives 0.260 and 0.0354
RECT_MIN_VALUES = 50                             # distinct v among those pixels, in every mode; the model's minimum is 55


def _rect_calls(H):
    return [{}, {"shard": (4, 2, 0)}, {"shard": (4, 2, 1)}] + ([{"slab_rows": (1, 3)}] if H >= 43 else [])


@functools.lru_cache(maxsize=None)
def _rect_frames(ci, mode):
    """(W, H, table, calls, the model's frame for each call) of one rectangle camera and mode: computed once, shared, read-only."""
    W, H = RECT_SIZES[ci]
    tf = _colour_table(17)
    assert (PM.rgba_of(tf, 0) != FILL).all()                    # the fill kernel's RGBA differs from the fill byte in every channel
    calls = _rect_calls(H)
    return W, H, tf, calls, [_freeze(_model(_rect_volume(), tf, W, H, RECT_CAMS[ci], mode, **kw)) for kw in calls]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("ci", RECT_CIS)
def test_projection_screen_rectangle_preconditions(ci, mode):
    """What keeps test_projection_screen_rectangle_and_fill from passing on an empty frame (the models alone)."""
    W, H, _, calls, models = _rect_frames(ci, mode)
    whole = models[0]
    assert whole["written"][:-1, :-1].all() and whole["written"].sum() == (W - 1) * (H - 1)
    counted = whole["written"] & (whole["n"] > 0)
    share = counted.sum() / ((W - 1) * (H - 1))
    values = len(np.unique(whole["index"][counted]))
    print(f"camera {ci} {W}x{H} mode {mode}: n > 0 on {share:.4f} of the written pixels, {values} distinct v")
    if ci == RECT_OFF_SCREEN:
        assert not counted.any()                  # every pixel is the fill kernel's
    else:
        assert share >= RECT_MIN_COUNTED_SHARE[ci], f"camera {ci}: n > 0 on {share:.4f} of the pixels only"
        assert values >= RECT_MIN_VALUES, f"camera {ci} mode {mode}: {values} distinct v only"
        assert 2 * (whole["written"] & ~counted).sum() > whole["written"].sum()       # more than half of the written pixels are the fill's (n == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("ci", RECT_CIS)
def test_projection_screen_rectangle_and_fill(ctx, ci, mode):
    """proj_kernel covers the tiles under the volume's screen rectangle, fill_outside_kernel writes n = 0 (v = 0, table entry 0, {0, 0}) beside it:
    whole frames, both shards of two, a row range, and the same frames with the rectangle switched off -- all equal to the model, bit for bit."""
    vol, cam = _rect_volume(), RECT_CAMS[ci]
    W, H, tf, calls, models = _rect_frames(ci, mode)
    frames = {}
    for rect in (None, "0"):
        with MO.knobs(ctx, {} if rect is None else {"VV_RECT": rect}):
            ctx.load_volume(vol, tf)
            for k, kw in enumerate(calls):
                frames[rect, k] = _proj(ctx, W, H, cam, mode, options=vv.make_options(**kw))
                _same_triple(frames[rect, k], models[k], f"camera {ci} {W}x{H} mode {mode} VV_RECT={rect} {kw}")
                assert ctx.last_launch()["phong"] == 4
    for k in range(len(calls)):
        for a, b in zip(frames[None, k], frames["0", k]):
            _same(a, b, f"camera {ci} mode {mode} {calls[k]}: with and without the rectangle")
