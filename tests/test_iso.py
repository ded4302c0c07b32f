"""Isosurface frames (vv_render_iso) against tests/iso_model.py, the numpy statement of the contract in include/volviz.h.

The model is itself held to the compositing oracle: under a table that is opaque from `level` upwards and true early
termination, one oracle frame shows which pixels hit, the hit's index (in the red byte) and the executed samples.  Every
comparison below is exact -- floats as their uint32 patterns -- and no pixel is excluded."""
import functools
import os

import numpy as np
import pytest

import iso_model as IM
import mip_oracle as MO
import oracle_lib as O
import volviz_amd as vv
import witness as Wt
from test_mip_geometry import RECT_CAMS, RECT_OFF_SCREEN, _rect_case, _rect_volume

HERE = os.path.dirname(os.path.abspath(__file__))
CAM_A = vv.Camera.orbit(3.0, 1.0, 0.6)
CAM_B = vv.Camera.orbit(1.2, 1.3, 2.0)
CAMS = {"camA": CAM_A, "camB": CAM_B}
CUT = dict(point=(.5, .5, .5), normal=(.3, .2, 1.))            # mip_oracle's / test_mip's cut plane
LAYOUT_KNOBS = ("VV_BRICKED", "VV_ZPAIR", "VV_ZFAST", "VV_FORCE_BIG", "VV_UNROLL")
ENVS = ({}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}, {"VV_ZFAST": "1"}, {"VV_FORCE_BIG": "1"}, {"VV_UNROLL": "2"})
ZFAST_ONLY = {"VV_ZFAST": "1", "VV_ZPAIR": "0"}            # the z-fastest build itself: VV_ZFAST=1 alone takes the x-pair copy built from it
FILL = 0x5A
ANISO_SCALE = (1.57, 1.0, 1.0)
ERR_INVALID, ERR_NO_VOLUME = -1, -2                        # include/volviz.h: vv_status


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name == "brain64":
        v = O.draw_default_brain(64, 64, 64)
    elif name == "brain128":
        v = O.draw_default_brain(128, 128, 128)
    elif name == "noise_u8":
        v = O.noise_u8(48, 40, 56, 3)
    elif name == "aniso":
        v = np.fromfile(os.path.join(HERE, "golden", "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
    else:
        assert name == "noise_f32"
        v = np.ascontiguousarray((O.noise_u8(40, 40, 40, 5).astype(np.float32) / np.float32(255)) ** 2, np.float32)
    v.setflags(write=False)
    return v


def _scaled(cam, scale):
    return vv.Camera(origin=cam.origin, look_at=cam.look_at, up=cam.up, fov_y=cam.fov_y, scale=scale)


def _level_table(level):
    """Opaque from `level` upwards, the index readable in the red byte: entry k = ((k + .5) / 255, 0, 0, 1)."""
    tf = np.zeros((256, 4), np.float32)
    k = np.arange(level, 256)
    tf[k, 0] = (k.astype(np.float32) + np.float32(0.5)) / np.float32(255)
    tf[k, 3] = 1.0
    return tf.reshape(1024)


def _colour_table(seed=7):
    # entries outside [0, 1] too: the conversion clamps
    return np.random.default_rng(seed).uniform(-0.3, 1.4, 1024).astype(np.float32)


def _median_level(M):
    return int(np.median(M[M > 0]))


def _model(vol, tf, W, H, cam, level, *, stype=vv.SLICE_NONE, step=None, filt=vv.FILTER_TEX8, images=None, slab_rows=(0, 0), shard=None,
           fill=FILL):
    return IM.render_cam(vol, tf, W, H, cam, level, slice_type=stype, plane=(*CUT["point"], *CUT["normal"]), step=step, filt=filt,
                         images=images, slab_rows=slab_rows, shard=shard, fill=fill)


def _oracle_level_frame(vol, W, H, cam, level, **okw):
    """(rgba, executed samples) of the oracle under the level table and true early termination."""
    sp = okw.pop("slice", None); rays = okw.pop("rays", None)
    return O.render(vol, _level_table(level), W, H, cam, slice=sp, rays=rays, options=vv.make_options(ert_mode=vv.ERT_TRUE, **okw), fill=0)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _same_triple(got, m, what):
    rgba, idx, hit = got
    _same(idx, m["index"], f"{what}: index image")
    _same(hit, m["hit"], f"{what}: hit records")
    _same(rgba, m["rgba"], f"{what}: rgba")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_iso():
    for name in ("render_iso", "render_iso_device"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert "vv_render_iso" in vv.EXPORTS and hasattr(vv.load_library(), "vv_render_iso")


CPU_FRAMES = [(v, c) for v in ("noise_u8", "brain64", "noise_f32", "aniso") for c in ("camA", "camB")]
CPU_IDS = [f"{v}-{c}" for v, c in CPU_FRAMES]


@functools.lru_cache(maxsize=None)
def _cpu_frame(name, cam_id):
    """One 99 x 71 frame of the model at the median of the frame's non-zero MIP indices: computed once, shared, read-only."""
    vol = _volume(name)
    cam = _scaled(CAMS[cam_id], ANISO_SCALE) if name == "aniso" else CAMS[cam_id]
    W, H = 99, 71
    _, M, _ = Wt.render(vol, np.zeros(1024, np.float32), W, H, cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y, scale=cam.scale,
                        mip=True)
    level = _median_level(M)
    m = _model(vol, _level_table(level), W, H, cam, level, fill=0)
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vol, cam, M, level, m


@pytest.mark.parametrize("name,cam_id", CPU_FRAMES, ids=CPU_IDS)
def test_model_equals_oracle(name, cam_id):
    vol, cam, M, level, m = _cpu_frame(name, cam_id)
    frame, n = _oracle_level_frame(vol, 99, 71, cam, level)
    print(f"{name} {cam_id}: level {level}, model count {m['count']}, oracle count {n}")
    hit = m["index"] > 0
    _same(frame[..., 0], m["index"], "the oracle's red byte against the model's index image")
    assert np.array_equal(frame[..., 3] == 255, hit) and np.isin(frame[..., 3], (0, 255)).all(), "alpha 255 exactly on the model's hit mask"
    assert n == m["count"], f"the oracle executes {n} samples, the model {m['count']}"
    assert np.array_equal(hit, M >= level), "a pixel has a hit iff its MIP index reaches the level"
    assert np.array_equal(hit, m["hit"][..., 3] > 0) and (m["index"][hit] >= level).all()
    assert not m["written"][-1].any() and not m["written"][:, -1].any() and m["written"][:-1, :-1].all()


@pytest.mark.parametrize("name,cam_id", CPU_FRAMES, ids=CPU_IDS)
def test_model_frames_are_not_vacuous(name, cam_id):
    _, _, _, level, m = _cpu_frame(name, cam_id)
    hit = m["index"] > 0
    share = hit.mean(); miss = (m["written"] & ~hit).sum() / m["written"].sum()
    ordinals = len(np.unique(m["hit"][..., 3][hit])); shades = len(np.unique(m["shade"][hit]))
    print(f"{name} {cam_id}: level {level}, hit share {share:.3f}, written without a hit {miss:.3f}, {ordinals} ordinals, {shades} shades")
    assert share >= 0.10 and miss >= 0.10 and ordinals >= 15 and shades >= 500


def test_both_branches_of_diffuse_are_exercised():
    zero = positive = 0
    for name, cam_id in CPU_FRAMES:
        m = _cpu_frame(name, cam_id)[4]
        hit = m["index"] > 0
        z = hit & ~m["g"].any(axis=-1)
        assert (m["shade"][z] == np.float32(0.3)).all()
        zero += int(z.sum()); positive += int((hit & ~z).sum())
    assert zero > 0 and positive > 0, (zero, positive)


def test_shading_arithmetic():
    f = np.float32
    one = np.ones(3, f)
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0.6, 0, 0.8], [1, 0, 0], [0, 0, -1]], f)
    g = np.array([[0, 0, 0], [0, 0, 7], [5, 0, 0], [0, 0, -3], [2, 2, 0], [0, 0, 9]])
    got = IM.shade_of(g, one, (4, 4, 4), d)
    want = [f(0.3),                                              # g = 0: len = 0
            f(0.3) + f(0.7) * f(1),                              # along the ray
            f(0.3),                                              # across it
            f(0.3) + f(0.7) * f(0.8),                            # |dp| / len = fl(3 * 4 * .8) / 12: sign dropped
            f(0.3) + f(0.7) * (f(8) / np.sqrt(f(128))),
            f(0.3) + f(0.7) * f(1)]
    assert got.dtype == np.float32 and got.view(np.uint32).tolist() == np.array(want, f).view(np.uint32).tolist()
    # an anisotropic scale and dimensions: G = ((g * 1 / scale) * n), each product rounded
    inv = f(1) / np.array([1.57, 1.0, 0.5], f)
    dims = (20, 36, 52)
    g = np.array([[3, -2, 1]]); d = np.array([[0.48, 0.6, 0.64]], f)
    G = [(f(g[0, a]) * inv[a]) * f(dims[a]) for a in range(3)]
    dp = G[0] * d[0, 0] + G[1] * d[0, 1] + G[2] * d[0, 2]
    ln = np.sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2])
    want = f(0.3) + f(0.7) * np.fmin(np.abs(dp) / ln, f(1))
    got = IM.shade_of(g, inv, dims, d)
    assert got.view(np.uint32)[0] == np.array([want], f).view(np.uint32)[0]
    assert got[0] != IM.shade_of(g, np.ones(3, f), (1, 1, 1), d)[0], "the scale and the dimensions enter the shade"
    # the conversion to bytes: clamp, then truncate
    assert IM.pack(np.array([-1.0, 0.5, 1.0, 7.0, 0.999999, 0.004], f)).tolist() == [0, 127, 255, 255, 254, 1]
    # the gradient reads through the march's classification: outside [0, 1)^3 the index is 0
    vol = np.full((4, 4, 4), 200, np.uint8)
    t = np.array([[0.5, 0.5, 0.5], [0.9, 0.5, 0.1]], f)
    assert IM.gradient(vol, t).tolist() == [[0, 0, 0], [-200, 0, 200]]


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


def _iso(ctx, W, H, cam, level, fill=FILL, **kw):
    return ctx.render_iso(W, H, cam, level, fill=fill, return_index=True, return_hit=True, **kw)


# (name, volume, camera, W, H, filter, step, envs, the layout the policy itself picks (None: forced layouts are not checked)): test_mip.py's PARITY table
# and the anisotropic volume under an anisotropic object scale
PARITY = [
    ("u8-tex8",        "noise_u8",  CAM_A, 99, 71, vv.FILTER_TEX8,  None,   ENVS + (ZFAST_ONLY,), 0),
    ("f32-exact",      "noise_f32", CAM_B, 99, 71, vv.FILTER_EXACT, None,   ENVS + (ZFAST_ONLY,), 0),
    ("brain128-1mod14", "brain128", CAM_A, 113, 85, vv.FILTER_TEX8, None,   ({}, {"VV_BRICKED": "1"}, {"VV_ZFAST": "1"}, ZFAST_ONLY), 2),
    ("f32-axis-step-scale", "noise_f32", vv.Camera(origin=(0.0, 0.0, -3.0), scale=(1.0, 0.8, 1.2)), 101, 67, vv.FILTER_TEX8, 1 / 50,
     ({}, {"VV_ZPAIR": "1"}, {"VV_ZPAIR": "0", "VV_FORCE_BIG": "1"}, {"VV_ZPAIR": "0", "VV_UNROLL": "2"}, {"VV_BRICKED": "1"}), None),
    ("u8-axis-exact",  "noise_u8",  vv.Camera(origin=(0.3, 0.2, -3.0)), 86, 57, vv.FILTER_EXACT, (1 / 40, 1 / 70, 1 / 33), ({}, {"VV_ZPAIR": "0"}, {"VV_FORCE_BIG": "1", "VV_ZPAIR": "0"}), None),
    ("aniso-scale",    "aniso",     _scaled(CAM_A, ANISO_SCALE), 99, 71, vv.FILTER_TEX8, None, ENVS + (ZFAST_ONLY,), None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["median", 1, 255])
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_iso_matches_model_on_every_build(ctx, case, which, monkeypatch):
    _, name, cam, W, H, filt, step, envs, policy_layout = case
    vol = _volume(name)
    okw = dict(filter=filt)
    if step is not None:
        okw["step"] = step
    tf = _colour_table()
    _set_env(monkeypatch, {})
    ctx.load_volume(vol, tf)
    if which == "median":
        _, M = ctx.render_mip(W, H, cam, options=vv.make_options(**okw), return_index=True)
        level = _median_level(M)
    else:
        level = which
    m = _model(vol, tf, W, H, cam, level, step=step, filt=filt)
    _, n_oracle = _oracle_level_frame(vol, W, H, cam, level, **okw)
    hits = (m["index"] != FILL) & (m["index"] > 0) if level > FILL else m["written"] & (m["hit"][..., 3] > 0)
    print(f"{case[0]} level {level}: {int(hits.sum())} hits, model count {m['count']}, oracle count {n_oracle}")
    assert m["count"] == n_oracle
    if which == "median":
        assert hits.mean() >= 0.10
    assert (m["index"][~m["written"]] == FILL).all() and m["written"][:-1, :-1].all() and m["written"].sum() == (W - 1) * (H - 1)
    layouts = set()
    for env in envs:
        _set_env(monkeypatch, env)
        ctx.load_volume(vol, tf)                    # (the knobs are read at volume load)
        got = _iso(ctx, W, H, cam, level, options=vv.make_options(**okw))
        lay = ctx.last_launch()
        _same_triple(got, m, f"{case[0]} level {level} {env}")
        assert lay["phong"] == 3, lay                 # an isosurface launch was reported
        layouts.add(lay["layout"])
        if policy_layout is not None:
            assert lay["layout"] == _forced_layout(env, policy_layout), (env, lay)
        if "VV_UNROLL" in env:
            assert lay["unroll"] == int(env["VV_UNROLL"]), lay
        counted = _iso(ctx, W, H, cam, level, options=vv.make_options(count_samples=True, **okw))
        n = ctx.last_sample_count()
        _same_triple(counted, m, f"{case[0]} level {level} {env}, instrumented")
        assert n == m["count"] == n_oracle, f"{case[0]} level {level} {env}: {n} samples counted, the model executes {m['count']}, the oracle {n_oracle}"
    if case[0] == "brain128-1mod14":
        assert layouts == {2, 4, 5}, layouts
    elif policy_layout is not None:
        assert layouts == {0, 1, 2, 3, 4, 5}, layouts           # every kernel build, for this voxel type


@pytest.mark.gpu
def test_iso_cut_plane(ctx, monkeypatch):
    vol = _volume("brain64")
    tf = _colour_table(11)
    W, H = 99, 71
    _set_env(monkeypatch, {})
    ctx.load_volume(vol, tf)
    frames = {}
    for stype in (vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT):
        sp = vv.make_slice_params(stype, **CUT)
        _, M = ctx.render_mip(W, H, CAM_A, slice=sp, return_index=True)
        level = _median_level(M) if stype != vv.SLICE_PLANE else frames[vv.SLICE_NONE][0]
        m = _model(vol, tf, W, H, CAM_A, level, stype=stype, fill=3)
        _, n_oracle = _oracle_level_frame(vol, W, H, CAM_A, level, slice=sp)
        assert (m["hit"][..., 3] > 0)[m["written"]].mean() >= 0.10
        for env in ({}, {"VV_BRICKED": "1"}, {"VV_FORCE_BIG": "1"}):
            _set_env(monkeypatch, env)
            ctx.load_volume(vol, tf)
            got = _iso(ctx, W, H, CAM_A, level, fill=3, slice=sp, options=vv.make_options(count_samples=True))
            _same_triple(got, m, f"slice type {stype} {env}")
            assert ctx.last_sample_count() == m["count"]
            if stype != vv.SLICE_PLANE:               # (the oracle draws SLICE_PLANE's highlight into the red channel and past the threshold)
                assert m["count"] == n_oracle
        frames[stype] = (level, got, m)
    for a, b in zip(frames[vv.SLICE_PLANE][1], frames[vv.SLICE_NONE][1]):
        _same(a, b, "SLICE_PLANE marches as SLICE_NONE")
    assert frames[vv.SLICE_PLANE_CUT][2]["count"] < frames[vv.SLICE_NONE][2]["count"]
    assert not np.array_equal(frames[vv.SLICE_PLANE_CUT][2]["index"], frames[vv.SLICE_NONE][2]["index"])


@pytest.mark.gpu
def test_iso_image_ray_source(ctx, monkeypatch):
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
    _, M = ctx.render_mip(W, H, CAM_B, rays=rays, return_index=True)
    level = _median_level(M)
    m = _model(vol, tf, W, H, CAM_B, level, images=(front, back), fill=0xEE)
    _, n_oracle = _oracle_level_frame(vol, W, H, CAM_B, level, rays=rays)
    assert (m["hit"][..., 3] > 0).mean() >= 0.10 and m["count"] == n_oracle
    for r in (rays, vv.image_rays(front, back, hint=CAM_B)):
        got = _iso(ctx, W, H, CAM_B, level, fill=0xEE, rays=r, options=vv.make_options(count_samples=True))
        _same_triple(got, m, "image rays")
        assert ctx.last_sample_count() == m["count"]


@pytest.mark.gpu
def test_iso_shards_and_slab_rows(ctx, monkeypatch):
    """Rows of other shards and outside the slab-row window keep the fill in all three images; the shards' union is the whole frame."""
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = _colour_table(3)
    ctx.load_volume(vol, tf)
    W, H = 99, 141                                   # 11 slab rows: bands of 4 -> 3 bands
    _, M = ctx.render_mip(W, H, CAM_A, return_index=True)
    level = _median_level(M)
    whole = _model(vol, tf, W, H, CAM_A, level, fill=0x77)
    full = _iso(ctx, W, H, CAM_A, level, fill=0x77)
    _same_triple(full, whole, "unsharded")
    union = [np.full_like(a, 0) for a in full]
    for a in union:
        a.view(np.uint8)[...] = 0x77
    covered = np.zeros((H, W), bool)
    for i in range(2):
        okw = dict(shard=(4, 2, i))
        m = _model(vol, tf, W, H, CAM_A, level, shard=(4, 2, i), fill=0x77)
        assert m["written"].any() and not (m["written"] & covered).any()
        got = _iso(ctx, W, H, CAM_A, level, fill=0x77, options=vv.make_options(**okw))
        _same_triple(got, m, f"shard {i} of 2")
        for u, g in zip(union, got):
            u[m["written"]] = g[m["written"]]
        covered |= m["written"]
    assert np.array_equal(covered, whole["written"])
    for u, f, what in zip(union, full, ("rgba", "index image", "hit records")):
        _same(u, f, f"union of 2 shards: {what}")
    m = _model(vol, tf, W, H, CAM_A, level, slab_rows=(2, 7), fill=0x11)
    assert m["written"][28:98, :-1].all() and m["written"].sum() == 70 * (W - 1)
    got = _iso(ctx, W, H, CAM_A, level, fill=0x11, options=vv.make_options(slab_rows=(2, 7)))
    _same_triple(got, m, "slab rows 2..7")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 29), (31, 1)])
def test_iso_frames_one_pixel_wide_or_high(ctx, W, H, monkeypatch):
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = _colour_table(13)
    ctx.load_volume(vol, tf)
    cam = vv.Camera(origin=(0.2, 0.1, -3.0))
    hits = 0
    for level in (1, 60):
        m = _model(vol, tf, W, H, cam, level)
        assert m["written"][:H - 1 if H > 1 else 1, :W - 1 if W > 1 else 1].all() and m["written"].sum() == max(W - 1, 1) * max(H - 1, 1)     # the lone column / row is written, but for its last pixel
        hits += int((m["hit"][..., 3] > 0).sum())
        got = _iso(ctx, W, H, cam, level, options=vv.make_options(count_samples=True))
        _same_triple(got, m, f"{W} x {H} level {level}")
        assert ctx.last_sample_count() == m["count"] > 0
    assert hits > 0


@pytest.mark.gpu
def test_iso_hits_where_the_mip_reaches_the_level(ctx, monkeypatch):
    _set_env(monkeypatch, {})
    W, H = 99, 71
    for name, cam in (("noise_u8", CAM_A), ("noise_f32", CAM_B)):
        vol = _volume(name)
        ctx.load_volume(vol, _colour_table())
        _, M = ctx.render_mip(W, H, cam, return_index=True)
        some = 0
        for level in (1, 64, 128, 200, 255):
            _, idx, hit = _iso(ctx, W, H, cam, level, fill=0)
            assert np.array_equal(idx > 0, M >= level), f"{name} level {level}"
            assert np.array_equal(hit[..., 3] > 0, M >= level) and (idx[idx > 0] >= level).all()
            some += int((idx > 0).sum())
        assert some > 0


@pytest.mark.gpu
def test_iso_output_subsets_device_outputs_and_instruments(ctx, monkeypatch):
    import torch
    _set_env(monkeypatch, {})
    vol = _volume("noise_f32")
    tf = _colour_table(4)
    ctx.load_volume(vol, tf)
    W, H = 128, 96
    _, M = ctx.render_mip(W, H, CAM_B, return_index=True)
    level = _median_level(M)
    want = _iso(ctx, W, H, CAM_B, level, fill=0x42)
    assert (want[1] != 0x42).any() and len(np.unique(want[2][..., 3])) >= 15
    # each image alone
    _same(ctx.render_iso(W, H, CAM_B, level, fill=0x42), want[0], "rgba alone")
    lib, h = ctx.lib, ctx.h
    import ctypes as C
    sp = vv.make_slice_params(); cp = CAM_B.params(W, H); rs = vv.analytic_rays(CAM_B)
    idx = np.full((H, W), 0x42, np.uint8); hit = np.full((H, W, 16), 0x42, np.uint8).view(np.float32)
    assert lib.vv_render_iso(h, W, H, C.byref(sp), C.byref(cp), C.byref(rs), None, level, None, idx.ctypes.data, None, 0, None) == 0
    assert lib.vv_render_iso(h, W, H, C.byref(sp), C.byref(cp), C.byref(rs), None, level, None, None, hit.ctypes.data, 0, None) == 0
    _same(idx, want[1], "index image alone")
    _same(hit, want[2], "hit records alone")
    # device pointers, enqueue-only on a torch stream and synchronous
    dev = torch.device("cuda", 0)
    for ts in (torch.cuda.Stream(device=dev), torch.cuda.default_stream(dev)):
        d_rgba = torch.full((H, W, 4), 0x42, dtype=torch.uint8, device=dev)
        d_idx = torch.full((H, W), 0x42, dtype=torch.uint8, device=dev)
        d_hit = torch.full((H, W, 16), 0x42, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            ctx.render_iso_device(W, H, CAM_B, level, d_rgba.data_ptr(), d_idx.data_ptr(), d_hit.data_ptr(), stream=vv.stream_handle(ts))
        ts.synchronize()
        _same(d_rgba.cpu().numpy(), want[0], "enqueue-only: rgba")
        _same(d_idx.cpu().numpy(), want[1], "enqueue-only: index image")
        _same(d_hit.cpu().numpy().view(np.float32), want[2], "enqueue-only: hit records")
    d_hit = torch.full((H, W, 16), 0x42, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.render_iso_device(W, H, CAM_B, level, 0, 0, d_hit.data_ptr())
    _same(d_hit.cpu().numpy().view(np.float32), want[2], "hit records alone, device")
    # instrumented frames: the same three images
    nb = (40 + 7) // 8
    bricks = torch.zeros((nb ** 3 + 31) // 32, dtype=torch.int32, device=dev)
    lines = torch.zeros(4096, dtype=torch.int32, device=dev)
    for okw in (dict(count_samples=True), dict(touched_bricks=bricks.data_ptr()),
                dict(touched_lines=lines.data_ptr(), touched_line_bits=4096 * 32, touched_lines_all=True)):
        _same_triple(_iso(ctx, W, H, CAM_B, level, fill=0x42, options=vv.make_options(**okw)),
                     dict(rgba=want[0], index=want[1], hit=want[2]), f"instrumented {sorted(okw)}")
    assert int(bricks.count_nonzero()) > 0 and int(lines.count_nonzero()) > 0
    assert ctx.last_frame_ms() > 0.0


@pytest.mark.gpu
def test_iso_leaves_the_context_alone_and_reports_errors(ctx, monkeypatch):
    import torch
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    W, H = 170, 130
    for phong in (False, True):
        before = ctx.render(W, H, CAM_A, phong=phong, fill=1)
        want, _ = O.render(vol, tf, W, H, CAM_A, phong=phong, fill=1)
        assert np.array_equal(before, want)
        _iso(ctx, W, H, CAM_A, 40)
        ctx.render_iso(W, H, CAM_B, 90, slice=vv.make_slice_params(vv.SLICE_PLANE_CUT, **CUT), options=vv.make_options(count_samples=True))
        after = ctx.render(W, H, CAM_A, phong=phong, fill=1)
        assert np.array_equal(after, before), f"phong={phong}"
    for level in (0, 256, -1):
        with pytest.raises(vv.VolvizError) as e:
            ctx.render_iso(W, H, CAM_A, level)
        assert e.value.code == ERR_INVALID
    with pytest.raises(vv.VolvizError) as e:
        ctx.render_iso_device(W, H, CAM_A, 40, 0, 0, 0)
    assert e.value.code == ERR_INVALID
    d_hit = torch.zeros(W * H * 16 + 16, dtype=torch.uint8, device=torch.device("cuda", 0))
    with pytest.raises(vv.VolvizError) as e:
        ctx.render_iso_device(W, H, CAM_A, 40, 0, 0, d_hit.data_ptr() + 4)
    assert e.value.code == ERR_INVALID
    with vv.Context(0) as empty:
        with pytest.raises(vv.VolvizError) as e:
            empty.render_iso(W, H, CAM_A, 40)
        assert e.value.code == ERR_NO_VOLUME
    assert np.array_equal(ctx.render(W, H, CAM_A, fill=1), O.render(vol, tf, W, H, CAM_A, fill=1)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the screen rectangle and the fill beside it (fill_outside_kernel, shared with the MIP and projection frames): test_mip_geometry's frames
# ---------------------------------------------------------------------------------------------------------------------
RECT_CIS = (0, 1, RECT_OFF_SCREEN)               # cube partly off the left edge, partly off the bottom, wholly off the screen
RECT_MIN_HIT_SHARE = {0: 0.10, 1: 0.015}         # of the (W-1) x (H-1) pixels; the model gives 0.135 and 0.0187 (levels 146 and 136)


def _rect_calls(H):
    return [{}, {"shard": (4, 2, 0)}, {"shard": (4, 2, 1)}] + ([{"slab_rows": (1, 3)}] if H >= 43 else [])


@functools.lru_cache(maxsize=None)
def _rect_frames(ci):
    """(W, H, level, table, calls, the model's frame for each call) of one rectangle camera: computed once, shared, read-only.  The level is the median
    of the MIP model's non-zero indices (128 where it has none: the cube is off the screen)."""
    W, H, M = _rect_case(ci)
    level = _median_level(M) if M.any() else 128
    tf = _colour_table(17)
    calls = _rect_calls(H)
    models = [_model(_rect_volume(), tf, W, H, RECT_CAMS[ci], level, **kw) for kw in calls]
    for m in models:
        for a in m.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return W, H, level, tf, calls, models


@pytest.mark.parametrize("ci", RECT_CIS)
def test_iso_screen_rectangle_preconditions(ci):
    """What keeps test_iso_screen_rectangle_and_fill from passing on an empty frame (the models alone)."""
    W, H, level, _, calls, models = _rect_frames(ci)
    whole = models[0]
    assert whole["written"][:-1, :-1].all() and whole["written"].sum() == (W - 1) * (H - 1)
    hit = whole["written"] & (whole["hit"][..., 3] > 0)
    share = hit.sum() / ((W - 1) * (H - 1))
    print(f"camera {ci} {W}x{H}: level {level}, hit on {share:.4f} of the written pixels")
    if ci == RECT_OFF_SCREEN:
        assert not hit.any()                      # every pixel is the fill kernel's
    else:
        assert share >= RECT_MIN_HIT_SHARE[ci], f"camera {ci}: a hit on {share:.4f} of the pixels only"
        assert (whole["written"] & ~hit).sum() > hit.sum()       # most written pixels lie beside the cube
    assert (whole["rgba"][whole["written"] & ~hit] == 0).all() and FILL != 0           # "no hit" is told from the fill byte


@pytest.mark.gpu
@pytest.mark.parametrize("ci", RECT_CIS)
def test_iso_screen_rectangle_and_fill(ctx, ci):
    """iso_kernel covers the tiles under the volume's screen rectangle, fill_outside_kernel writes "no hit" (zeros in all three images) beside it: whole
    frames, both shards of two, a row range, and the same frames with the rectangle switched off -- all equal to the model, bit for bit."""
    vol, cam = _rect_volume(), RECT_CAMS[ci]
    W, H, level, tf, calls, models = _rect_frames(ci)
    frames = {}
    for rect in (None, "0"):
        with MO.knobs(ctx, {} if rect is None else {"VV_RECT": rect}):
            ctx.load_volume(vol, tf)
            for k, kw in enumerate(calls):
                frames[rect, k] = _iso(ctx, W, H, cam, level, options=vv.make_options(**kw))
                _same_triple(frames[rect, k], models[k], f"camera {ci} {W}x{H} level {level} VV_RECT={rect} {kw}")
                assert ctx.last_launch()["phong"] == 3
    for k in range(len(calls)):
        for a, b in zip(frames[None, k], frames["0", k]):
            _same(a, b, f"camera {ci} {calls[k]}: with and without the rectangle")
