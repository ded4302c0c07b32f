"""Maximum-intensity projection (vv_render_mip / vv_classify_indices) against the CPU oracle.

The oracle only composites; tests/mip_oracle.py derives the per-pixel maximum M from 255 of its frames (the level-set
identity).  Every comparison below is exact and no pixel is excluded."""
import os

import numpy as np
import pytest

import mip_oracle as MO
import oracle_lib as O
import volviz_amd as vv

CAM_A = vv.Camera.orbit(3.0, 1.0, 0.6)
CAM_B = vv.Camera.orbit(1.2, 1.3, 2.0)
CUT = dict(point=(.5, .5, .5), normal=(.3, .2, 1.))
LAYOUT_KNOBS = ("VV_BRICKED", "VV_ZPAIR", "VV_ZFAST", "VV_FORCE_BIG", "VV_UNROLL")
ENVS = ({}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}, {"VV_ZFAST": "1"}, {"VV_FORCE_BIG": "1"}, {"VV_UNROLL": "2"})
ZFAST_ONLY = {"VV_ZFAST": "1", "VV_ZPAIR": "0"}            # the z-fastest build itself: VV_ZFAST=1 alone takes the x-pair copy built from it


def _forced_layout(env, default):
    """The layout code vv_debug_last_launch must report for a knob set on a view off the memory axes; `default` is the policy's own choice."""
    if env.get("VV_ZFAST") == "1":
        return 4 if env.get("VV_ZPAIR") == "0" else 5
    for knob, code in (("VV_BRICKED", 2), ("VV_ZPAIR", 3), ("VV_FORCE_BIG", 1)):
        if env.get(knob) == "1":
            return code
    return default


def _volume(name):
    if name == "brain64":
        return O.draw_default_brain(64, 64, 64)
    if name == "brain128":
        return O.draw_default_brain(128, 128, 128)
    if name == "noise_u8":
        return O.noise_u8(48, 40, 56, 3)
    assert name == "noise_f32"
    return np.ascontiguousarray((O.noise_u8(40, 40, 40, 5).astype(np.float32) / np.float32(255)) ** 2, np.float32)


def _colour_table(seed=7):
    # entries outside [0, 1] too: the conversion clamps
    return np.random.default_rng(seed).uniform(-0.3, 1.4, 1024).astype(np.float32)


def _grey_table():
    ramp = (np.arange(256, dtype=np.float32) / np.float32(255)) ** np.float32(0.5)
    return np.repeat(ramp[:, None], 4, axis=1).reshape(1024).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_mip():
    for name in ("render_mip", "render_mip_device", "classify_indices"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    lib = vv.load_library()
    for sym in ("vv_render_mip", "vv_classify_indices"):
        assert sym in vv.EXPORTS and hasattr(lib, sym)


@pytest.mark.parametrize("cut", [False, True], ids=["nocut", "cut"])
@pytest.mark.parametrize("cam", [CAM_A, CAM_B], ids=["camA", "camB"])
@pytest.mark.parametrize("name", ["brain64", "noise_u8", "noise_f32"])
def test_level_set_sweep_preconditions(name, cam, cut):
    """The identity's preconditions (checked inside sweep) and the two that keep the GPU comparisons from passing vacuously, with the oracle alone."""
    sp = vv.make_slice_params(vv.SLICE_PLANE_CUT, **CUT) if cut else None
    M = MO.sweep(_volume(name), 99, 71, cam, slice=sp)
    MO.assert_not_vacuous(M, f"{name} cut={cut}")
    assert not M[-1].any() and not M[:, -1].any()          # row H-1 / column W-1 are never written


def test_rgba_conversion_model():
    tf = np.zeros(1024, np.float32)
    tf[0:4] = (-1.0, 0.5, 1.0, 7.0)
    tf[4:8] = (0.999999, 0.004, 0.00390625, np.float32(254.5 / 255))
    got = MO.rgba_of(tf, np.array([0, 1], np.uint8))
    assert got.tolist() == [[0, 127, 255, 255], [254, 1, 0, 254]]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _set_env(monkeypatch, env):
    for k in LAYOUT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _expect(M, written, tf, fill):
    """The two images a frame over `fill` bytes must hold."""
    idx = np.where(written, M, np.uint8(fill)).astype(np.uint8)
    rgba = np.where(written[..., None], MO.rgba_of(tf, M), np.uint8(fill)).astype(np.uint8)
    return rgba, idx


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


# (name, volume, camera, W, H, filter, step, envs, the layout the policy itself picks (None: forced layouts are not checked))
PARITY = [
    ("u8-tex8",        "noise_u8",  CAM_A, 99, 71, vv.FILTER_TEX8,  None,   ENVS + (ZFAST_ONLY,), 0),
    ("f32-exact",      "noise_f32", CAM_B, 99, 71, vv.FILTER_EXACT, None,   ENVS + (ZFAST_ONLY,), 0),
    # W, H == 1 (mod 14); 2 M voxels: the default policy itself takes the bricked copy for this view
    ("brain128-1mod14", "brain128", CAM_A, 113, 85, vv.FILTER_TEX8, None,   ({}, {"VV_BRICKED": "1"}, {"VV_ZFAST": "1"}, ZFAST_ONLY), 2),
    # along the memory axis (32 x 2 wave tiles, 3 samples per trip), a step that is not 1 / dims, an object scale != 1, a ragged frame
    ("f32-axis-step-scale", "noise_f32", vv.Camera(origin=(0.0, 0.0, -3.0), scale=(1.0, 0.8, 1.2)), 101, 67, vv.FILTER_TEX8, 1 / 50,
     ({}, {"VV_ZPAIR": "1"}, {"VV_ZPAIR": "0", "VV_FORCE_BIG": "1"}, {"VV_ZPAIR": "0", "VV_UNROLL": "2"}, {"VV_BRICKED": "1"}), None),
    ("u8-axis-exact",  "noise_u8",  vv.Camera(origin=(0.3, 0.2, -3.0)), 86, 57, vv.FILTER_EXACT, (1 / 40, 1 / 70, 1 / 33), ({}, {"VV_ZPAIR": "0"}, {"VV_FORCE_BIG": "1", "VV_ZPAIR": "0"}), None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_mip_matches_oracle_sweep(ctx, case, monkeypatch):
    _, name, cam, W, H, filt, step, envs, policy_layout = case
    vol = _volume(name)
    okw = dict(filter=filt)
    if step is not None:
        okw["step"] = step
    M = MO.sweep(vol, W, H, cam, options_kw=okw)
    MO.assert_not_vacuous(M, case[0])
    written = MO.written_mask(vol, W, H, cam, options=vv.make_options(**okw))
    tables = (_colour_table(), vv.transfer_preset(vv.TF_HEAD))          # a colour table and a grey preset
    layouts = set()
    for env in envs:
        _set_env(monkeypatch, env)
        for tf in tables:
            ctx.load_volume(vol, tf)                    # (the knobs are read at volume load)
            rgba, idx = ctx.render_mip(W, H, cam, options=vv.make_options(**okw), fill=0x5A, return_index=True)
            lay = ctx.last_launch()
            want_rgba, want_idx = _expect(M, written, tf, 0x5A)
            _assert_same(idx, want_idx, f"{case[0]} {env}: index image")
            _assert_same(rgba, want_rgba, f"{case[0]} {env}: rgba")
            assert lay["phong"] == 2, lay                 # a MIP launch was reported
            layouts.add(lay["layout"])
            if policy_layout is not None:
                assert lay["layout"] == _forced_layout(env, policy_layout), (env, lay)
            if "VV_UNROLL" in env:
                assert lay["unroll"] == int(env["VV_UNROLL"]), lay
            # one image at a time
            only_rgba = ctx.render_mip(W, H, cam, options=vv.make_options(**okw), fill=0x5A)
            _assert_same(only_rgba, want_rgba, f"{case[0]} {env}: rgba alone")
    if case[0] == "brain128-1mod14":
        assert layouts == {2, 4, 5}, layouts
    elif policy_layout is not None:
        assert layouts == {0, 1, 2, 3, 4, 5}, layouts           # every kernel build, for this voxel type


@pytest.mark.gpu
@pytest.mark.parametrize("stype", [vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT], ids=["none", "plane", "cut"])
def test_mip_slice_types(ctx, stype, monkeypatch):
    vol = _volume("brain64")
    sp = vv.make_slice_params(stype, **CUT)
    W, H = 99, 71
    M = MO.sweep(vol, W, H, CAM_A, slice=sp)
    MO.assert_not_vacuous(M, f"slice type {stype}")
    if stype == vv.SLICE_PLANE:                    # marches as SLICE_NONE
        assert np.array_equal(M, MO.sweep(vol, W, H, CAM_A))
    written = MO.written_mask(vol, W, H, CAM_A, slice=sp)
    tf = _colour_table(11)
    for env in ({}, {"VV_BRICKED": "1"}, {"VV_FORCE_BIG": "1"}):
        _set_env(monkeypatch, env)
        ctx.load_volume(vol, tf)
        rgba, idx = ctx.render_mip(W, H, CAM_A, slice=sp, fill=3, return_index=True)
        want_rgba, want_idx = _expect(M, written, tf, 3)
        _assert_same(idx, want_idx, f"slice type {stype} {env}: index image")
        _assert_same(rgba, want_rgba, f"slice type {stype} {env}: rgba")


@pytest.mark.gpu
def test_mip_image_ray_source(ctx, monkeypatch):
    """End points read from first-pass images (point-sampled, UNORM8), as the reference's second pass reads its FBOs."""
    _set_env(monkeypatch, {})
    vol = _volume("noise_u8")
    W, H = 90, 62
    front, back = O.first_pass(CAM_B, 3 * W, 3 * H)
    rays = vv.image_rays(front, back)
    M = MO.sweep(vol, W, H, CAM_B, rays=rays)
    MO.assert_not_vacuous(M, "image rays")
    written = MO.written_mask(vol, W, H, CAM_B, rays=rays)
    tf = _colour_table(5)
    ctx.load_volume(vol, tf)
    for r in (rays, vv.image_rays(front, back, hint=CAM_B)):
        rgba, idx = ctx.render_mip(W, H, CAM_B, rays=r, fill=0xEE, return_index=True)
        want_rgba, want_idx = _expect(M, written, tf, 0xEE)
        _assert_same(idx, want_idx, "image rays: index image")
        _assert_same(rgba, want_rgba, "image rays: rgba")


@pytest.mark.gpu
def test_mip_untouched_pixels_and_shards(ctx, monkeypatch):
    """Column W-1, row H-1 and the rows of other shards keep the fill byte in both images; the shards' union is the unsharded frame."""
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = _colour_table(3)
    ctx.load_volume(vol, tf)
    W, H = 99, 141                                   # 11 slab rows: bands of 4 -> 3 bands
    M = MO.sweep(vol, W, H, CAM_A)
    MO.assert_not_vacuous(M, "sharded frame")
    full_rgba, full_idx = ctx.render_mip(W, H, CAM_A, fill=0x77, return_index=True)
    whole = MO.written_mask(vol, W, H, CAM_A)
    assert not whole[-1].any() and not whole[:, -1].any() and whole[:-1, :-1].all()
    want_rgba, want_idx = _expect(M, whole, tf, 0x77)
    _assert_same(full_idx, want_idx, "unsharded index image")
    _assert_same(full_rgba, want_rgba, "unsharded rgba")
    for count in (2, 3):
        union_rgba = np.full((H, W, 4), 0x77, np.uint8); union_idx = np.full((H, W), 0x77, np.uint8)
        covered = np.zeros((H, W), bool)
        for i in range(count):
            okw = dict(shard=(4, count, i))
            written = MO.written_mask(vol, W, H, CAM_A, options=vv.make_options(**okw))
            assert written.any() and not (written & covered).any()
            rgba, idx = ctx.render_mip(W, H, CAM_A, options=vv.make_options(**okw), fill=0x77, return_index=True)
            w_rgba, w_idx = _expect(M, written, tf, 0x77)
            _assert_same(idx, w_idx, f"shard {i} of {count}: index image")
            _assert_same(rgba, w_rgba, f"shard {i} of {count}: rgba")
            union_rgba[written] = rgba[written]; union_idx[written] = idx[written]
            covered |= written
        assert np.array_equal(covered, whole)
        _assert_same(union_idx, full_idx, f"union of {count} shards: index image")
        _assert_same(union_rgba, full_rgba, f"union of {count} shards: rgba")
    # a slab-row range
    okw = dict(slab_rows=(2, 7))
    written = MO.written_mask(vol, W, H, CAM_A, options=vv.make_options(**okw))
    rgba, idx = ctx.render_mip(W, H, CAM_A, options=vv.make_options(**okw), fill=0x11, return_index=True)
    w_rgba, w_idx = _expect(M, written, tf, 0x11)
    _assert_same(idx, w_idx, "slab rows 2..7: index image")
    _assert_same(rgba, w_rgba, "slab rows 2..7: rgba")


@pytest.mark.gpu
@pytest.mark.parametrize("name,cam", [("noise_u8", CAM_A), ("noise_f32", CAM_B), ("noise_f32", vv.Camera(origin=(0.0, 0.0, -3.0)))], ids=["u8", "f32", "f32-axis"])
def test_mip_sample_count(ctx, name, cam, monkeypatch):
    """count_samples: the full executed count (an instrumented frame never drops a ray early), and the same bytes as the uninstrumented frame."""
    vol = _volume(name)
    tf = _colour_table(9)
    W, H = 120, 90
    for cut in (False, True):
        sp = vv.make_slice_params(vv.SLICE_PLANE_CUT, **CUT) if cut else None
        okw = dict(step=1 / 64)
        n = MO.executed_samples(vol, W, H, cam, slice=sp, options_kw=okw)
        assert n > 0
        for env in ENVS:
            _set_env(monkeypatch, env)
            ctx.load_volume(vol, tf)
            rgba, idx = ctx.render_mip(W, H, cam, slice=sp, options=vv.make_options(count_samples=True, **okw), fill=9, return_index=True)
            n_got = ctx.last_sample_count()
            assert n_got == n, f"{name} cut={cut} {env}: {n_got} samples counted, the oracle executes {n}"
            rgba2, idx2 = ctx.render_mip(W, H, cam, slice=sp, options=vv.make_options(**okw), fill=9, return_index=True)
            _assert_same(idx2, idx, f"{name} cut={cut} {env}: uninstrumented index image")
            _assert_same(rgba2, rgba, f"{name} cut={cut} {env}: uninstrumented rgba")
            assert ctx.last_frame_ms() > 0.0


@pytest.mark.gpu
def test_mip_saturated_rays_stop_exactly(ctx, monkeypatch):
    """A volume that reaches index 255: uninstrumented frames may drop such rays early, which must not change a byte."""
    _set_env(monkeypatch, {})
    vol = np.ascontiguousarray(np.minimum(_volume("noise_f32") * np.float32(4), np.float32(1.5)))
    W, H = 99, 71
    M = MO.sweep(vol, W, H, CAM_A)
    assert (M == 255).mean() > 0.05
    written = MO.written_mask(vol, W, H, CAM_A)
    tf = _colour_table(2)
    ctx.load_volume(vol, tf)
    want_rgba, want_idx = _expect(M, written, tf, 0)
    for count in (False, True):
        rgba, idx = ctx.render_mip(W, H, CAM_A, options=vv.make_options(count_samples=count), return_index=True)
        _assert_same(idx, want_idx, f"count_samples={count}: index image")
        _assert_same(rgba, want_rgba, f"count_samples={count}: rgba")
    assert ctx.last_sample_count() == MO.executed_samples(vol, W, H, CAM_A)


@pytest.mark.gpu
def test_classify_indices(ctx, monkeypatch):
    import torch
    _set_env(monkeypatch, {})
    vol = _volume("noise_u8")
    tf = _colour_table(21)
    ctx.load_volume(vol, tf)
    W, H = 99, 71
    rgba, idx = ctx.render_mip(W, H, CAM_A, fill=0, return_index=True)
    wr = np.s_[:-1, :-1]
    assert len(np.unique(idx)) >= 30
    # the context's table and an explicit one, host buffers
    got = ctx.classify_indices(idx)
    assert got.shape == (H, W, 4)
    _assert_same(got[wr], rgba[wr], "context table, host")
    _assert_same(got, MO.rgba_of(tf, idx), "context table, host, every entry")
    other = _grey_table()
    _assert_same(ctx.classify_indices(idx, other), MO.rgba_of(other, idx), "explicit table, host")
    _assert_same(ctx.classify_indices(idx), MO.rgba_of(tf, idx), "an explicit table does not replace the context's")
    # device buffers, synchronous and enqueue-only
    dev = torch.device("cuda", 0)
    d_idx = torch.from_numpy(idx.copy()).to(dev)
    for table in (None, other):
        for stream in (0, vv.stream_handle(torch.cuda.current_stream())):
            d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.classify_indices_device(d_idx.data_ptr(), idx.size, d_out.data_ptr(), tf=table, stream=stream)
            torch.cuda.synchronize()
            _assert_same(d_out.cpu().numpy(), MO.rgba_of(tf if table is None else table, idx), f"device buffers, table={'own' if table is None else 'explicit'}, stream={stream}")
    # all 256 indices
    every = np.arange(256, dtype=np.uint8)
    _assert_same(ctx.classify_indices(every), MO.rgba_of(tf, every), "all indices")
    # a table edit: the look-up over the old index image equals a fresh frame
    ctx.set_transfer_function(other)
    fresh = ctx.render_mip(W, H, CAM_A, fill=0)
    _assert_same(ctx.classify_indices(idx)[wr], fresh[wr], "after set_transfer_function")
    with pytest.raises(vv.VolvizError):
        bad = other.copy(); bad[5] = np.nan
        ctx.classify_indices(idx, bad)


@pytest.mark.gpu
def test_mip_enqueue_only_on_a_torch_stream(ctx, monkeypatch):
    import torch
    _set_env(monkeypatch, {})
    vol = _volume("noise_f32")
    tf = _colour_table(4)
    ctx.load_volume(vol, tf)
    W, H = 128, 96
    want_rgba, want_idx = ctx.render_mip(W, H, CAM_B, fill=0x42, return_index=True)
    assert len(np.unique(want_idx)) >= 30
    dev = torch.device("cuda", 0)
    for ts in (torch.cuda.Stream(device=dev), torch.cuda.default_stream(dev)):
        d_rgba = torch.full((H, W, 4), 0x42, dtype=torch.uint8, device=dev)
        d_idx = torch.full((H, W), 0x42, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            ctx.render_mip_device(W, H, CAM_B, d_rgba.data_ptr(), d_idx.data_ptr(), stream=vv.stream_handle(ts))
        ts.synchronize()
        _assert_same(d_idx.cpu().numpy(), want_idx, "enqueue-only: index image")
        _assert_same(d_rgba.cpu().numpy(), want_rgba, "enqueue-only: rgba")
    # one device image at a time, synchronous
    d_idx = torch.full((H, W), 0x42, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.render_mip_device(W, H, CAM_B, 0, d_idx.data_ptr())
    _assert_same(d_idx.cpu().numpy(), want_idx, "index image alone, device")
    with pytest.raises(vv.VolvizError):
        ctx.render_mip_device(W, H, CAM_B, 0, 0)


@pytest.mark.gpu
def test_mip_leaves_the_context_alone(ctx, monkeypatch):
    """A compositing frame before and after a MIP frame on the same context is byte-identical."""
    _set_env(monkeypatch, {})
    vol = _volume("brain64")
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    W, H = 170, 130
    for phong in (False, True):
        before = ctx.render(W, H, CAM_A, phong=phong, fill=1)
        want, _ = O.render(vol, tf, W, H, CAM_A, phong=phong, fill=1)
        assert np.array_equal(before, want)
        ctx.render_mip(W, H, CAM_A, return_index=True)
        ctx.render_mip(W, H, CAM_B, slice=vv.make_slice_params(vv.SLICE_PLANE_CUT, **CUT), options=vv.make_options(count_samples=True))
        ctx.classify_indices(np.arange(256, dtype=np.uint8), _grey_table())
        after = ctx.render(W, H, CAM_A, phong=phong, fill=1)
        assert np.array_equal(after, before), f"phong={phong}"
