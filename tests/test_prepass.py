"""The radius pre-pass of unshaded frames runs only when its arguments changed, and the zeros beside the volume's screen rectangle of a composite frame
are written by fill blocks of the march launch (vv_api.cpp: issue_prepass / launch_kernels, csrc/vv_fill.h).  Neither may change a pixel: every frame
here is compared exactly with the oracle and with the same library under VV_RAD_REUSE=0 VV_TAIL_FILL=0, over buffers pre-filled with 0xA5 (pixels the
frame does not own keep it), and Context.prepass_state() is held to what the frame's arguments say.

Shapes: a 64^3 noise volume (u8 and f32); frames 97 x 61, 128 x 72, 29 x 43, 15 x 16 (14 k + 1 and 14 k + 2 pixels a side) and 2 x 2."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
import volviz_amd as vv

FILL = 0xA5
FRAMES = ((97, 61), (128, 72), (29, 43), (15, 16), (2, 2))
KNOBS = ("VV_TILE_LOG2W", "VV_XCD_BAND", "VV_UNROLL", "VV_LDS_RESERVE", "VV_LDS_RESERVE_PHONG", "VV_BRICKED", "VV_ZPAIR", "VV_BLOCK_W", "VV_TAIL", "VV_ZFAST",
         "VV_FORCE_BIG", "VV_RECT", "VV_LPT", "VV_LPT_RUN", "VV_PHONG_BRICKS", "VV_RAD_REUSE", "VV_TAIL_FILL")
OFF = {"VV_RAD_REUSE": "0", "VV_TAIL_FILL": "0"}

# the cube (half side 1) seen from 4 away with a 45 degree field of view: inside the frame, cut by each frame edge, covering the whole frame (no pixel
# beside the rectangle), behind the camera (no rectangle: the whole frame marches) and in front of it but off the screen (an empty rectangle: nothing marches)
CAMERAS = {
    "inside": vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5),
    "cut_left": vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(1.5, 0.0, 0.0)),
    "cut_right": vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(-1.5, 0.0, 0.0)),
    "cut_top": vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(0.0, -1.5, 0.0)),
    "cut_bottom": vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(0.0, 1.5, 0.0)),
    "cover": vv.Camera(origin=(0.0, 0.0, -2.2)),
    "behind": vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(0.0, 0.0, -8.0)),
    "off_screen": vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(4.0, 0.0, -2.5)),
}
KNOB_SETS = ({}, {"VV_BLOCK_W": "32"}, {"VV_BLOCK_W": "64"}, {"VV_BLOCK_W": "128"}, {"VV_TILE_LOG2W": "3"}, {"VV_TILE_LOG2W": "5"},
             {"VV_XCD_BAND": "0"}, {"VV_XCD_BAND": "3"}, {"VV_LPT": "1", "VV_LPT_RUN": "1"})


@contextlib.contextmanager
def knobs(ctx, env):
    """The VV_* knobs of `env` and no others, picked up by `ctx`; the environment the block found is put back at its end and re-read."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        ctx.reread_env()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ctx.reread_env()


_VOL8 = None


def volume(dtype):
    global _VOL8
    if _VOL8 is None:
        _VOL8 = O.noise_u8(64, 64, 64, 11)
    return _VOL8 if dtype == "u8" else (_VOL8.astype(np.float32) / np.float32(255))


_WANT = {}


def want(dtype, tf_id, tf, W, H, cam_key, cam, *, rays=None, **okw):
    """The oracle's frame over FILL (computed once per distinct frame, shared and never written to)."""
    key = (dtype, tf_id, W, H, cam_key, rays is not None, tuple(sorted(okw.items())))
    if key not in _WANT:
        img, _ = O.render(volume(dtype), tf, W, H, cam, rays=rays, options=vv.make_options(**okw) if okw else None, fill=FILL)
        img.setflags(write=False)
        _WANT[key] = img
    return _WANT[key]


def same(got, exp, what):
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {exp[tuple(bad[0])]}"


def something_to_fill(ctx, W, H, cam, slab_rows=(0, 0), shard=None):
    """Does the frame just rendered have owned pixels beside the rectangle its marching blocks cover?  Restated from the frame's definition: the screen
    rectangle (vv_debug_screen_rect) widened to whole blocks of the launch (last_launch: 2^blk_log2w x (256 >> blk_log2w) pixels, strips counted from the
    first pixel row of the row range; a shard's rectangle limits columns only).  False too when nothing marches (the pre-pass writes the frame then)."""
    if W < 2 or H < 2:
        return False
    r = vv.screen_rect(cam, W, H)
    if r is None:
        return False
    bl = ctx.last_launch()["blk_log2w"]
    bw, bh = 1 << bl, 256 >> bl
    nby = (H + 13) // 14
    rb, re = (0, nby) if slab_rows == (0, 0) else slab_rows
    ys = np.arange(H)
    owned = (ys <= H - 2) & (ys // 14 >= rb) & (ys // 14 < re)
    clamp = lambda v, lo, hi: int(min(max(np.floor(v), lo), hi))
    ntx = (W + bw - 1) // bw
    tx0 = clamp(r[0] / bw, 0, ntx); tx1 = clamp(r[1] / bw, -1, ntx - 1) + 1
    if shard is not None:
        band, count, index = shard
        owned &= (ys // 14 // band) % count == index
        y0, y1 = 0, H
    else:
        ylo, yhi = rb * 14, min(re * 14, H - 1)
        nst = ((yhi - ylo + 7) // 8 * 8 + bh - 1) // bh
        s0 = clamp((r[2] - ylo) / bh, 0, nst); s1 = clamp((r[3] - ylo) / bh, -1, nst - 1) + 1
        y0, y1 = ylo + s0 * bh, ylo + max(s1, s0) * bh
    if tx1 <= tx0 or y1 <= y0 or not owned.any():
        return False
    xs = np.arange(W)
    inside = ((xs >= tx0 * bw) & (xs < tx1 * bw) & (xs <= W - 2))[None, :] & ((ys >= y0) & (ys < y1))[:, None]
    return bool((owned[:, None] & (xs <= W - 2)[None, :] & ~inside).any())


def check_frame(ctx, dtype, tf, W, H, cam_key, env, what, **okw):
    """One host-buffer frame under `env` and once more under VV_RAD_REUSE=0 VV_TAIL_FILL=0: both equal the oracle; fill blocks exactly when there is something to fill."""
    cam = CAMERAS[cam_key]
    exp = want(dtype, "engine", tf, W, H, cam_key, cam, **okw)
    opts = vv.make_options(**okw) if okw else None
    with knobs(ctx, env):
        got = ctx.render(W, H, cam, options=opts, fill=FILL)
        state = ctx.prepass_state()
        fill = something_to_fill(ctx, W, H, cam, okw.get("slab_rows", (0, 0)), okw.get("shard"))
    same(got, exp, f"{what} {env}")
    assert (state[3] != 0) == fill, (what, env, state, fill)
    with knobs(ctx, {**env, **OFF}):
        ref = ctx.render(W, H, cam, options=opts, fill=FILL)
        assert ctx.prepass_state()[2:] == (0, 0), (what, env)
    same(ref, exp, f"{what} {env} with the pre-pass on every frame and its zeros")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("cam_key", list(CAMERAS))
def test_fill_geometry(ctx, dtype, cam_key):
    """Every frame size under every block shape, wave tile, XCD band and the forced order table, for one camera and voxel type."""
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(volume(dtype), tf)
    for W, H in FRAMES:
        for env in KNOB_SETS:
            check_frame(ctx, dtype, tf, W, H, cam_key, env, f"{dtype} {cam_key} {W} x {H}")


@pytest.mark.gpu
@pytest.mark.parametrize("cam_key", ["inside", "cut_left", "cover"])
def test_fill_geometry_shards_and_row_ranges(ctx, cam_key):
    """Shards of 2 and 3 ranks (bands of 4 slab rows) and a slab_rows range: the other ranks' rows and the rows outside the range keep 0xA5."""
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(volume("f32"), tf)
    for W, H in ((97, 61), (128, 72)):
        for count in (2, 3):
            for index in range(count):
                check_frame(ctx, "f32", tf, W, H, cam_key, {}, f"shard {index} of {count} {cam_key} {W} x {H}", shard=(4, count, index))
        check_frame(ctx, "f32", tf, W, H, cam_key, {}, f"rows 1..3 {cam_key} {W} x {H}", slab_rows=(1, 3))
        check_frame(ctx, "f32", tf, W, H, cam_key, {"VV_BLOCK_W": "64"}, f"rows 1..3, 64 x 4 blocks {cam_key} {W} x {H}", slab_rows=(1, 3))


@pytest.mark.gpu
def test_reuse_happens_and_only_when_it_may():
    """One sequence of frames on one context of its own; after each, the frame against the oracle and prepass_state() against what the key says."""
    import torch
    dev = torch.device("cuda", 0)
    W, H = 97, 61
    tf_a, tf_b = vv.transfer_preset(vv.TF_ENGINE), vv.transfer_preset(vv.TF_HEAD)
    tf_c = tf_a.copy().reshape(256, 4); tf_c[40:, 3] *= 1.5; tf_c = tf_c.reshape(1024)       # opacities above 1: FrameParams::alpha_unit changes
    unit = lambda t: bool(((t.reshape(256, 4)[:, 3] >= 0) & (t.reshape(256, 4)[:, 3] <= 1)).all())
    assert unit(tf_a) and not unit(tf_c)
    tfs = {"engine": tf_a, "head": tf_b, "over": tf_c}
    cam = CAMERAS["inside"]
    ulp = vv.Camera(origin=(float(np.nextafter(np.float32(cam.origin[0]), np.float32(np.inf))), cam.origin[1], cam.origin[2]))
    assert np.float32(ulp.origin[0]) != np.float32(cam.origin[0])
    cams = {"inside": cam, "ulp": ulp, "orbit": vv.Camera.orbit(4.0, np.pi / 3 + 0.3, np.pi / 5 + 0.4)}
    front, back = O.first_pass(cam, W, H)
    with vv.Context(0) as c:
        c.load_volume(volume("f32"), tf_a)
        state = {"tf": "engine", "prev": c.prepass_state()}
        bufs = [torch.full((400, 400, 4), FILL, dtype=torch.uint8, device=dev) for _ in range(2)]

        def frame(what, expect, *, cam_key="inside", w=W, h=H, buf=0, host=False, stream=0, rays=None, **okw):
            """A composite frame; expect: "launch", "reuse" or None (whatever it decides)."""
            opts = vv.make_options(**okw) if okw else None
            exp = want("f32", state["tf"], tfs[state["tf"]], w, h, cam_key, cams[cam_key], rays=rays, **okw)
            if host:
                got = c.render(w, h, cams[cam_key], options=opts, rays=rays, fill=FILL)
            else:
                out = bufs[buf].view(-1)[: w * h * 4]
                out.fill_(FILL)
                torch.cuda.synchronize()
                c.render_device(w, h, cams[cam_key], out.data_ptr(), options=opts, rays=rays, stream=stream)
                torch.cuda.synchronize()
                got = out.cpu().numpy().reshape(h, w, 4)
            same(got, exp, what)
            now = c.prepass_state()
            launched, reused = now[0] - state["prev"][0], now[1] - state["prev"][1]
            state["prev"] = now
            assert launched + reused == (1 if w >= 2 and h >= 2 else 0) and now[2] == reused, (what, now)
            if expect is not None:
                assert (launched, reused) == ((1, 0) if expect == "launch" else (0, 1)), (what, expect, now)

        def table(name, what):
            before = unit(tfs[state["tf"]])
            c.set_transfer_function(tfs[name]); state["tf"] = name
            frame(what, "reuse" if unit(tfs[name]) == before else "launch")      # (the table is no argument of the pre-pass; whether its opacities lie in [0, 1] is)

        frame("first frame after the volume load", "launch")
        frame("same view into another buffer", "reuse", buf=1)
        table("head", "table changed")
        table("over", "table with opacities above 1")
        table("engine", "table back")
        frame("step changed", "launch", step=1.0 / 100)
        frame("step back", "launch")
        frame("camera moved by one ulp of one coordinate", "launch", cam_key="ulp")
        frame("orbit camera", "launch", cam_key="orbit")
        frame("orbit camera again", "reuse", cam_key="orbit")
        for w, h in ((98, 61), (97, 61), (97, 62), (97, 61)):
            frame(f"frame size {w} x {h}", "launch", w=w, h=h)
        frame("shard 0 of 2", "launch", shard=(4, 2, 0))
        frame("shard 1 of 2", "launch", shard=(4, 2, 1))
        frame("rows 0..3", "launch", slab_rows=(0, 3))
        frame("rows 1..3", "launch", slab_rows=(1, 3))
        frame("analytic rays", "launch")
        frame("image rays", "launch", host=True, rays=vv.image_rays(front, back))
        frame("image rays again", "launch", host=True, rays=vv.image_rays(front, back))
        frame("analytic rays again, same camera", "launch")
        def other(render, *a, **k):
            """A frame of another kind (its own pre-pass, if it has one, is not this test's to count)."""
            render(W, H, cam, *a, fill=FILL, **k)
            state["prev"] = c.prepass_state()

        other(c.render_mip); frame("after a MIP frame", None)
        other(c.render_iso, 100); frame("after an isosurface frame", None)
        other(c.render_projection, vv.PROJ_MEAN); frame("after a projection frame", None)
        other(c.render_mip); other(c.render_mip)
        assert c.prepass_state()[2] == 1, "the second of two equal MIP frames reuses the first one's radii"
        frame("before a Phong frame", None)
        other(c.render, phong=True); frame("after a Phong frame (which neither hits nor invalidates)", "reuse")
        ts = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(ts):
            frame("second stream", "launch", stream=vv.stream_handle(ts))
        frame("the context's stream again", "launch")
        c.load_volume(volume("f32"), tf_a)
        frame("volume reload", "launch")
        with knobs(c, {"VV_BLOCK_W": "64"}):
            frame("reread_env with another block shape", "launch")
        frame("reread_env back", "launch")
        frame("a frame that grows the radius buffer", "launch", w=200, h=150)
        frame("the small one again", "launch")
        frame("device-output frame", "reuse")
        frame("host-output frame between device-output frames", None, host=True)
        frame("device-output frame after it", None)
        frame("2 x 2 (no pre-pass exists)", None, w=2, h=2)
        frame("1 x 5 (no pre-pass exists)", None, w=1, h=5)


@pytest.mark.gpu
def test_order_table_reuse():
    """The forced order table (VV_LPT=1) on an unchanged view: the second frame launches nothing but the march and equals the first."""
    tf = vv.transfer_preset(vv.TF_ENGINE)
    W, H = 128, 72
    for cam_key in ("cover", "inside"):
        cam = CAMERAS[cam_key]
        exp = want("u8", "engine", tf, W, H, cam_key, cam)
        with vv.Context(0) as c:
            c.load_volume(volume("u8"), tf)
            with knobs(c, {"VV_LPT": "1", "VV_LPT_RUN": "1"}):
                a = c.render(W, H, cam, fill=FILL); sa = c.prepass_state()
                b = c.render(W, H, cam, fill=FILL); sb = c.prepass_state()
            same(a, exp, f"{cam_key}: first frame"); same(b, a, f"{cam_key}: second frame")
            assert sa[:3] == (1, 0, 0) and sb[:3] == (1, 1, 1), (cam_key, sa, sb)
