"""Maximum-intensity projection: every kernel build, the frame's edges and the launch geometry, against the level-set sweep of the CPU oracle.

tests/test_mip.py pins the MIP frame itself; this module drives mip_kernel / fill_outside_kernel through the mechanisms they share with (but hold their own
copy of) the compositing path: the seven builds, the screen rectangle and its fill, the block-to-pixel mapping, tiny and ragged frames, odd volume shapes
and the instruments.  Every comparison is exact, covers every pixel of both images (RGBA and index) over a non-zero fill byte, and takes its expectation
from MO.sweep / MO.written_mask / MO.rgba_of / MO.executed_samples alone.  One sweep per camera serves all of its knob sets, shards and row ranges.

Coverage (rows: what could be wrong; cells: the test that would notice):

  builds        layout 0 linear, 1 linear 64-bit, 2 bricked (cached), 3 z-pair, 5 x-pair, u8 + f32   test_mip.py::test_mip_matches_oracle_sweep (exact codes)
                layout 4 z-fastest (VV_ZFAST=1 VV_ZPAIR=0), u8 + f32                                 test_mip.py::test_mip_matches_oracle_sweep, test_mip_side_view_layouts
                side view under the policy: 5, with VV_ZPAIR=0: 4                                    test_mip_side_view_layouts
                bricked build for volumes beyond the caches (namespace brick), unroll 3,
                lds_reserve 155000 + 4 KB, 64 x 4 blocks                                             test_mip_volume_beyond_the_caches
  mechanisms    tile-order table (M.order), unit lengths 1 / 5 / 64, partial rounds                  test_mip_block_to_pixel_mapping
                XCD bands 0 / 1 / 3                                                                  test_mip_block_to_pixel_mapping
                block shapes 8 x 32, 16 x 16, 32 x 8, 64 x 4, 128 x 2; wave tiles 8 x 8, 16 x 4, 32 x 2  test_mip_block_to_pixel_mapping
                no LDS reserve (more blocks per CU)                                                  test_mip_block_to_pixel_mapping
                fill_outside_kernel: rectangle partly / wholly off the screen, no rectangle, VV_RECT=0,
                shards and row ranges that cut the rectangle                                         test_mip_screen_rectangle_and_fill
                instruments (sample count, slots, touched bricks, touched lines)                     test_mip_instruments_equal_the_march
  edges         frames of 1 x 1 ... 16 x 15 and 29 x 43 (no rad_kernel, no fill below 2 pixels)      test_mip_tiny_frames
                seeded sweep: dims 5..47, both types, f32 outside [0, 1], W, H == 1 (mod 14),
                scaled cubes, cut planes, steps, filters                                             test_mip_random_sweep
                re-pitched rows, edges off the 4-voxel brick, single-voxel axes, through every copy  test_mip_volume_shapes
  preconditions the oracle alone (not gpu): the frames above are not empty and not flat              test_*_preconditions
"""
import functools

import numpy as np
import pytest

import iso_model as IM
import mip_oracle as MO
import oracle_lib as O
import proj_model as PM
import volviz_amd as vv

CAM_A = vv.Camera.orbit(3.0, 1.0, 0.6)
CAM_AXIS = vv.Camera(origin=(0.0, 0.0, -3.0))
CAM_SIDE = vv.Camera.orbit(4.0, np.pi / 2, np.pi)         # from -x: screen x runs along the volume's z axis (orbit(4, pi/2, -pi/2) is the front view (0, 0, -4))
ZFAST_ONLY = {"VV_ZFAST": "1", "VV_ZPAIR": "0"}
ENVS = ({}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}, {"VV_ZFAST": "1"}, {"VV_FORCE_BIG": "1"}, {"VV_UNROLL": "2"}, ZFAST_ONLY)
FILL = 0x5A


def _table(seed=7):
    """A colour table with entries outside [0, 1] whose entry 0 differs from the fill byte in every channel."""
    tf = np.random.default_rng(seed).uniform(-0.3, 1.4, 1024).astype(np.float32)
    assert (MO.rgba_of(tf, 0) != FILL).all()
    return tf


def _f32(vol8):
    return np.ascontiguousarray(vol8.astype(np.float32) / np.float32(255))


_mask_cache = {}


def _written(vol, W, H, cam, okw, slice=None):
    key = (id(vol), W, H, id(cam), tuple(sorted(okw.items())), id(slice))
    if key not in _mask_cache:
        _mask_cache[key] = (MO.written_mask(vol, W, H, cam, slice=slice, options=vv.make_options(**okw)), vol, cam, slice)     # (keeps the ids alive)
    return _mask_cache[key][0]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the side view: x-pair under the policy, z-fastest with VV_ZPAIR=0
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _side_case(dtype):
    vol = O.noise_u8(128, 128, 128, 9)                       # 2^21 voxels: the policy's threshold for the side view's copies (noise: the brain fills too little of this frame)
    if dtype == "f32":
        vol = _f32(vol)
    W, H = 113, 85
    return vol, W, H, MO.sweep(vol, W, H, CAM_SIDE)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_side_view_preconditions(dtype):
    vol, W, H, M = _side_case(dtype)
    MO.assert_not_vacuous(M, f"side view {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_mip_side_view_layouts(ctx, dtype):
    vol, W, H, M = _side_case(dtype)
    MO.assert_not_vacuous(M, f"side view {dtype}")
    tf = _table()
    written = _written(vol, W, H, CAM_SIDE, {})
    for env, code in (({}, 5), ({"VV_ZPAIR": "0"}, 4), ({"VV_ZFAST": "0"}, 2), ({"VV_ZFAST": "0", "VV_BRICKED": "0"}, 0)):
        with MO.knobs(ctx, env):
            ctx.load_volume(vol, tf)
            MO.assert_frame(ctx, M, written, tf, FILL, W, H, CAM_SIDE, f"side view {dtype} {env}")
            lay = ctx.last_launch()
            assert lay["layout"] == code and lay["phong"] == 2, (env, lay)
            if code in (4, 5):
                assert lay["tile_log2w"] == 5 and lay["unroll"] == 3, (env, lay)      # the front view's tiles on the copy whose rows run along z


# ---------------------------------------------------------------------------------------------------------------------
# 2. screen rectangle and fill
# ---------------------------------------------------------------------------------------------------------------------
RECT_CAMS = [vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(2.4, 0.0, 0.0)),                  # cube at the left edge, partly off
             vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(0.0, 3.0, 0.0)),                  # ... at the bottom edge
             vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(9.0, 0.0, 0.0)),                  # wholly off the screen
             vv.Camera(origin=(0.0, 0.0, -40.0), fov_y=4.0),                               # far away, long lens
             vv.Camera(origin=(0.0, 0.0, -400.0), fov_y=0.4),
             vv.Camera(origin=(0.3, 0.2, -1.6), fov_y=100.0),                              # close: corners near the eye's plane
             vv.Camera(origin=(0.0, 0.0, -1.0005)),                                        # on the cube's face: no rectangle
             vv.Camera(origin=(1.3, 0.9, -2.2), look_at=(0.2, -0.1, 0.0), scale=(0.4, 1.0, 0.25)),
             vv.Camera(origin=(-3.0, 2.0, 2.5), scale=(1.5, 0.3, 0.8), up=(0.2, 1.0, 0.1)),
             vv.Camera.orbit(4.0, 1.0, 0.6, fov_y=20.0),
             vv.Camera.orbit(6.0, 0.4, -1.2, look_at=(0.5, 0.5, -0.5))]
RECT_SIZES = [(170, 113), (113, 57), (29, 43), (64, 15), (200, 150)]
RECT_OFF_SCREEN = 2


@functools.lru_cache(maxsize=None)
def _rect_volume():
    return _f32(O.noise_u8(20, 24, 28, 3))


@functools.lru_cache(maxsize=None)
def _rect_case(ci):
    W, H = RECT_SIZES[ci % len(RECT_SIZES)]
    return W, H, MO.sweep(_rect_volume(), W, H, RECT_CAMS[ci])


@pytest.mark.parametrize("ci", range(len(RECT_CAMS)))
def test_screen_rectangle_preconditions(ci):
    """What keeps the rectangle comparisons from passing on an empty frame; thresholds below test_mip.py's because the cube fills little of these frames by design."""
    W, H, M = _rect_case(ci)
    assert not M[-1].any() and not M[:, -1].any()
    if ci == RECT_OFF_SCREEN:
        assert not M.any()
        written = _written(_rect_volume(), W, H, RECT_CAMS[ci], {})
        assert written[:-1, :-1].all() and not written[-1].any() and not written[:, -1].any()       # every pixel is fill_outside_kernel's
    else:
        share, levels = MO.share_and_levels(M)
        assert share >= 0.03, f"camera {ci}: M > 0 on {share:.3f} of the pixels only"
        assert levels >= 30, f"camera {ci}: {levels} distinct levels only"


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(RECT_CAMS)))
def test_mip_screen_rectangle_and_fill(ctx, ci):
    """mip_kernel covers the tiles under the volume's screen rectangle, fill_outside_kernel writes table entry 0 / index 0 beside it: whole frames, both shards
    of two, a row range, and the same frames with the rectangle switched off -- all equal to one expectation."""
    vol, cam = _rect_volume(), RECT_CAMS[ci]
    W, H, M = _rect_case(ci)
    tf = _table()
    calls = [{}, {"shard": (4, 2, 0)}, {"shard": (4, 2, 1)}] + ([{"slab_rows": (1, 3)}] if H >= 43 else [])
    frames = {}
    for rect in (None, "0"):
        with MO.knobs(ctx, {} if rect is None else {"VV_RECT": rect}):
            ctx.load_volume(vol, tf)
            for k, kw in enumerate(calls):
                written = _written(vol, W, H, cam, kw)
                frames[rect, k] = MO.assert_frame(ctx, M, written, tf, FILL, W, H, cam, f"camera {ci} {W}x{H} VV_RECT={rect} {kw}", options=vv.make_options(**kw))
    for k in range(len(calls)):
        for a, b in zip(frames[None, k], frames["0", k]):
            assert np.array_equal(a, b), (ci, calls[k])


# ---------------------------------------------------------------------------------------------------------------------
# 3. block-to-pixel mapping
# ---------------------------------------------------------------------------------------------------------------------
# the four cameras of test_tile_order_table (the third is a front view like the first, its x component 2e-16) and a true side view
MAP_CAMS = [vv.Camera(), vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5), vv.Camera.orbit(4.0, np.pi / 2, -np.pi / 2), vv.Camera.orbit(3.0, 0.5, 0.9, fov_y=60.0), CAM_SIDE]
MAP_ENVS = [{"VV_LPT": "1"}, {"VV_LPT": "1", "VV_LPT_RUN": "1"}, {"VV_LPT": "1", "VV_LPT_RUN": "5"}, {"VV_LPT": "1", "VV_LPT_RUN": "64"},
            {"VV_LPT": "1", "VV_BRICKED": "0"}, {"VV_LPT": "1", "VV_BLOCK_W": "128", "VV_TILE_LOG2W": "5"},
            {"VV_XCD_BAND": "0"}, {"VV_XCD_BAND": "3"}, {"VV_BLOCK_W": "8"}, {"VV_BLOCK_W": "64"}, {"VV_BLOCK_W": "128"},
            {"VV_TILE_LOG2W": "4"}, {"VV_TILE_LOG2W": "5"}, {"VV_LDS_RESERVE": "0"}]
MAP_CALLS = [{}, {"shard": (4, 2, 1)}, {"slab_rows": (2, 9)}]
MAP_W, MAP_H, MAP_STEP = 200, 150, 1 / 48
MAP_ALIGNED = (0, 2)                     # cameras whose screen x runs along the volume's x: 32 x 2 wave tiles by policy


@functools.lru_cache(maxsize=None)
def _map_volume():
    return _f32(O.noise_u8(36, 30, 33, 5))


@functools.lru_cache(maxsize=None)
def _map_case(ci):
    vol, cam = _map_volume(), MAP_CAMS[ci]
    M = MO.sweep(vol, MAP_W, MAP_H, cam, options_kw=dict(step=MAP_STEP))
    counts = [MO.executed_samples(vol, MAP_W, MAP_H, cam, options_kw=dict(step=MAP_STEP, **kw)) for kw in MAP_CALLS]
    return M, counts


def _expected_shape(env, aligned):
    """(tile_log2w, blk_log2w, unroll, lds_reserve) choose_launch must report for a volume in the caches without a z-fastest copy: the knob where the
    policy honours it (a block is at least one wave tile wide and high), its own choice elsewhere."""
    tile = int(env.get("VV_TILE_LOG2W", 5 if aligned else 3))
    block_w = int(env.get("VV_BLOCK_W", 16 if tile == 3 else 32))
    lw = block_w.bit_length() - 1
    blk = lw if lw == 5 or (lw >= tile and (256 >> lw) >= (64 >> tile)) else 5
    return tile, blk, 3 if tile == 5 else 2, int(env.get("VV_LDS_RESERVE", 36000))


@pytest.mark.parametrize("ci", range(len(MAP_CAMS)))
def test_block_to_pixel_mapping_preconditions(ci):
    M, counts = _map_case(ci)
    MO.assert_not_vacuous(M, f"mapping camera {ci}")
    assert counts[0] > counts[1] > 0 and counts[0] > counts[2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(MAP_CAMS)))
def test_mip_block_to_pixel_mapping(ctx, ci):
    """mip_kernel on the block -> (strip, tile) -> pixel mapping it shares with march_kernel (csrc/vv_tiles.h): the balanced tile order with several unit lengths, XCD bands, every block
    and wave-tile shape the knobs reach, with shards and row ranges; both images, the executed-sample count and the launch record."""
    vol, cam = _map_volume(), MAP_CAMS[ci]
    M, counts = _map_case(ci)
    MO.assert_not_vacuous(M, f"mapping camera {ci}")
    tf = _table()
    shapes = set()
    for env in MAP_ENVS:
        with MO.knobs(ctx, env):
            ctx.load_volume(vol, tf)
            for kw, n in zip(MAP_CALLS, counts):
                written = _written(vol, MAP_W, MAP_H, cam, dict(step=MAP_STEP, **kw))
                what = f"camera {ci} {env} {kw}"
                a = MO.assert_frame(ctx, M, written, tf, FILL, MAP_W, MAP_H, cam, what, options=vv.make_options(step=MAP_STEP, **kw))
                lay = ctx.last_launch()
                b = MO.assert_frame(ctx, M, written, tf, FILL, MAP_W, MAP_H, cam, what + " counted", options=vv.make_options(step=MAP_STEP, count_samples=True, **kw))
                assert ctx.last_sample_count() == n, f"{what}: {ctx.last_sample_count()} samples counted, the oracle executes {n}"
                want = _expected_shape(env, ci in MAP_ALIGNED)
                for l in (lay, ctx.last_launch()):
                    assert (l["tile_log2w"], l["blk_log2w"], l["unroll"], l["lds_reserve"]) == want and l["phong"] == 2, (env, l, want)
                assert l["layout"] == (3 if want[0] == 5 else 0), (env, l)       # 32 x 2 tiles of a small volume: the z-pair copy
                shapes.add(want[:2])
    # the block shapes these knob sets must have reached for this camera (tile_log2w, blk_log2w)
    assert shapes == ({(5, 5), (5, 6), (5, 7), (4, 5)} if ci in MAP_ALIGNED else {(3, 3), (3, 4), (3, 5), (4, 5), (5, 5), (5, 7)}), shapes


# ---------------------------------------------------------------------------------------------------------------------
# 4. frame edges
# ---------------------------------------------------------------------------------------------------------------------
TINY = [(1, 1), (1, 9), (9, 1), (2, 2), (14, 14), (15, 16), (16, 15), (29, 43)]
TINY_WRITTEN = {(1, 1): 1, (1, 9): 8, (9, 1): 8}          # a one-pixel-wide frame writes its column but for row H-1 (and the other way round)


@functools.lru_cache(maxsize=None)
def _tiny_volume():
    return O.noise_u8(9, 8, 10, 3)


@functools.lru_cache(maxsize=None)
def _tiny_case(W, H):
    return MO.sweep(_tiny_volume(), W, H, vv.Camera())


@pytest.mark.parametrize("W,H", TINY)
def test_tiny_frames_preconditions(W, H):
    M = _tiny_case(W, H)
    written = _written(_tiny_volume(), W, H, vv.Camera(), {})
    assert M.any() and not (M > 0)[~written].any()
    if (W, H) in TINY_WRITTEN:
        assert int(written.sum()) == TINY_WRITTEN[W, H]
    else:
        assert written[:-1, :-1].all() and int(written.sum()) == (W - 1) * (H - 1)
    if W >= 14 and H >= 14:
        assert len(np.unique(M)) >= 30


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", TINY)
def test_mip_tiny_frames(ctx, W, H):
    """Below 2 pixels a side there is no rad_kernel and no fill, and the radius comes from the ray's own front point; 14 k + 1 and 14 k + 2 pixels a side."""
    vol, cam = _tiny_volume(), vv.Camera()
    M = _tiny_case(W, H)
    assert M.any()
    written = _written(vol, W, H, cam, {})
    tf = _table()
    for env in ({}, {"VV_ZPAIR": "0"}, {"VV_BRICKED": "1"}, {"VV_LPT": "1", "VV_LPT_RUN": "1"}):
        with MO.knobs(ctx, env):
            ctx.load_volume(vol, tf)
            for count in (False, True):
                MO.assert_frame(ctx, M, written, tf, FILL, W, H, cam, f"{W}x{H} {env} count_samples={count}", options=vv.make_options(count_samples=count))
            assert ctx.last_sample_count() == MO.executed_samples(vol, W, H, cam)


N_RANDOM = 16


def _random_case(seed):
    """One seeded configuration of everything vv_render_mip takes (after test_gpu_parity.py's _random_case; noise volumes only, brains have too few levels)."""
    rng = np.random.default_rng(4000 + seed)
    dims = tuple(int(v) for v in rng.integers(5, 48, size=3))                     # nx, ny, nz
    if seed % 2:
        vol = O.noise_u8(*dims, int(rng.integers(1, 2**31)))
    else:
        vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)               # white noise
    if rng.random() < 0.5:
        vol = vol.astype(np.float32) / np.float32(255)
        if rng.random() < 0.5:
            vol = (vol * np.float32(1.3) - np.float32(0.1)).astype(np.float32)     # values outside [0,1]: saturating index
    W = int(rng.choice([int(rng.integers(20, 90)), 29, 43, 57, 71]))              # incl. W == 1 (mod 14)
    H = int(rng.choice([int(rng.integers(20, 90)), 29, 43, 57]))
    scale = tuple(float(v) for v in rng.choice([1.0, 1.0, 0.8, 1.57, 0.5], size=3))
    r = float(rng.uniform(1.5, 3.5))
    cam = vv.Camera.orbit(r, float(rng.uniform(0.15, np.pi - 0.15)), float(rng.uniform(-np.pi, np.pi)), scale=scale)
    st = int(rng.choice([vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT]))
    point = rng.uniform(0.35, 0.65, size=3); normal = rng.normal(size=3)
    sp = vv.make_slice_params(st, tuple(point), tuple(normal))
    step = None if rng.random() < 0.4 else float(rng.choice([1 / 16, 1 / 37, 1 / 64, 1 / 130]))
    okw = dict(step=step, filter=int(rng.choice([vv.FILTER_TEX8, vv.FILTER_EXACT])))
    env = ENVS[1:][int(rng.integers(0, len(ENVS) - 1))]
    return np.ascontiguousarray(vol), W, H, cam, sp, okw, env


@functools.lru_cache(maxsize=None)
def _random_sweep(seed):
    vol, W, H, cam, sp, okw, env = _random_case(seed)
    return (vol, W, H, cam, sp, okw, env), MO.sweep(vol, W, H, cam, slice=sp, options_kw=okw)


@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_random_sweep_preconditions(seed):
    (vol, W, H, cam, sp, okw, env), M = _random_sweep(seed)
    share, levels = MO.share_and_levels(M)
    assert share >= 0.10, f"seed {seed}: M > 0 on {share:.3f} of the pixels only"
    assert levels >= 30, f"seed {seed}: {levels} distinct levels only"


def test_random_sweep_reaches_every_variant():
    cases = [_random_case(s) for s in range(N_RANDOM)]
    assert {c[0].dtype for c in cases} == {np.dtype(np.uint8), np.dtype(np.float32)}
    assert any(c[0].dtype == np.float32 and (c[0].min() < 0 or c[0].max() > 1) for c in cases)
    assert {c[4].type for c in cases} == {vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT}
    assert any(c[1] % 14 == 1 for c in cases) and any(c[2] % 14 == 1 for c in cases)
    assert len({tuple(sorted(c[6].items())) for c in cases}) >= 4 and any(c[6] == ZFAST_ONLY for c in cases)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_mip_random_sweep(ctx, seed):
    (vol, W, H, cam, sp, okw, env), M = _random_sweep(seed)
    written = _written(vol, W, H, cam, okw, slice=sp)
    n = MO.executed_samples(vol, W, H, cam, slice=sp, options_kw=okw)
    tf = _table(100 + seed)
    for e in ({}, env):
        with MO.knobs(ctx, e):
            ctx.load_volume(vol, tf)
            what = f"seed {seed}: {vol.shape} {vol.dtype} {W}x{H} {okw} {e}"
            MO.assert_frame(ctx, M, written, tf, FILL, W, H, cam, what, slice=sp, options=vv.make_options(**okw))
            MO.assert_frame(ctx, M, written, tf, FILL, W, H, cam, what + " counted", slice=sp, options=vv.make_options(count_samples=True, **okw))
            assert ctx.last_sample_count() == n, what


# ---------------------------------------------------------------------------------------------------------------------
# 5. volume shapes through every copy
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [((256, 9, 7), "f32"), ((1024, 5, 6), "u8")] + [(d, t) for d in ((5, 4, 3), (3, 9, 1), (1, 1, 1), (17, 16, 15)) for t in ("u8", "f32")]
SHAPE_CAMS = [vv.Camera(), vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5)]
SHAPE_ENVS = [{}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}, {"VV_ZFAST": "1"}, ZFAST_ONLY, {"VV_FORCE_BIG": "1"}]
SHAPE_W, SHAPE_H, SHAPE_STEP = 75, 59, 1 / 60
SHAPE_IDS = ["x".join(map(str, d)) + "-" + t for d, t in SHAPES]


@functools.lru_cache(maxsize=None)
def _shape_case(k):
    dims, dtype = SHAPES[k]
    vol = np.random.default_rng(17).integers(0, 256, size=dims[::-1], dtype=np.uint8)
    if dtype == "f32":
        vol = vol.astype(np.float32) / np.float32(255)
        if dims[0] < 256:                                                                    # the small shapes also leave [0, 1]: the index saturates
            vol = (vol * np.float32(1.3) - np.float32(0.1)).astype(np.float32)
    vol = np.ascontiguousarray(vol)
    return vol, [MO.sweep(vol, SHAPE_W, SHAPE_H, cam, options_kw=dict(step=SHAPE_STEP)) for cam in SHAPE_CAMS]


def _assert_shape_frames_not_vacuous(k, Ms):
    for M in Ms:
        if SHAPES[k][0] == (1, 1, 1):                   # one voxel: one level besides 0
            assert (M > 0).mean() >= 0.25 and M.max() > 0
        else:
            MO.assert_not_vacuous(M, SHAPE_IDS[k])


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_volume_shapes_preconditions(k):
    vol, Ms = _shape_case(k)
    _assert_shape_frames_not_vacuous(k, Ms)
    if vol.dtype == np.float32 and SHAPES[k][0][0] < 256 and vol.size > 1:
        assert vol.max() > 1 and any((M == 255).any() for M in Ms)           # saturates at the top; the 27- and 60-voxel draws need not go below 0
        assert vol.size < 1000 or vol.min() < 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_mip_volume_shapes(ctx, k):
    """Re-pitched volumes (rows a multiple of 1 KiB), edges off the 4-voxel brick and single-voxel axes, f32 values outside [0, 1]: through the linear
    layout with both addressings and through the bricked, z-pair, z-fastest and x-pair copies, along the memory axis and off it."""
    (nx, ny, nz), _ = SHAPES[k]
    vol, Ms = _shape_case(k)
    _assert_shape_frames_not_vacuous(k, Ms)
    tf = _table()
    okw = dict(step=SHAPE_STEP)
    counts = [MO.executed_samples(vol, SHAPE_W, SHAPE_H, cam, options_kw=okw) for cam in SHAPE_CAMS]
    for env in SHAPE_ENVS:
        with MO.knobs(ctx, env):
            ctx.load_volume(vol, tf)
            if nx * vol.itemsize % 1024 == 0:           # the padded layout (test_padded_pitch_layout's formula)
                row = nx * vol.itemsize + 32
                rows = ny + (1 if (ny * row) % 4096 == 0 else 0)
                assert ctx.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096
            for cam, M, n in zip(SHAPE_CAMS, Ms, counts):
                written = _written(vol, SHAPE_W, SHAPE_H, cam, okw)
                what = f"{SHAPE_IDS[k]} {env} camera {SHAPE_CAMS.index(cam)}"
                MO.assert_frame(ctx, M, written, tf, FILL, SHAPE_W, SHAPE_H, cam, what, options=vv.make_options(**okw))
                MO.assert_frame(ctx, M, written, tf, FILL, SHAPE_W, SHAPE_H, cam, what + " counted", options=vv.make_options(count_samples=True, **okw))
                assert ctx.last_sample_count() == n, what
                lay = ctx.last_launch()["layout"]
                if cam is SHAPE_CAMS[1]:                # off the memory axes the forced knob decides alone
                    assert lay == {(): 0, ("VV_BRICKED",): 2, ("VV_ZPAIR",): 3, ("VV_ZFAST",): 5, ("VV_ZFAST", "VV_ZPAIR"): 4, ("VV_FORCE_BIG",): 1}[tuple(sorted(env))], (env, lay)


# ---------------------------------------------------------------------------------------------------------------------
# 6. a volume beyond the caches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mip_volume_beyond_the_caches(ctx):
    """1032^3 u8 (the smallest cube of whole 8-voxel bricks above 1 GiB, generated on the device): the policy's branch for volumes beyond the caches -- the uncached bricked build,
    3 samples per trip and 155000 + 4096 bytes of LDS on the linear layout off the axis, 64 x 4 blocks along it."""
    import torch
    n = 1032
    assert n ** 3 > (1 << 30) >= (n - 8) ** 3                # beyond the caches: vol_bytes > 1 GiB
    dev = torch.device("cuda", 0)
    tf = _table()
    W, H = 99, 71
    okw = dict(step=1 / 64)
    try:
        with MO.knobs(ctx, {}):
            v8 = torch.empty(n * n * n, dtype=torch.uint8, device=dev)
            ctx.generate_noise_device(v8.data_ptr(), n, n, n, 11)
            ctx.load_volume_device(v8.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
            torch.cuda.synchronize()
            host = v8.cpu().numpy().reshape(n, n, n)
            del v8
            torch.cuda.empty_cache()
        for cam, frames in ((CAM_A, (({}, 2), ({"VV_BRICKED": "0"}, 0))), (CAM_AXIS, (({}, 3), ({"VV_ZPAIR": "0"}, 0)))):
            M = MO.sweep(host, W, H, cam, options_kw=okw)
            MO.assert_not_vacuous(M, "1032^3")
            written = MO.written_mask(host, W, H, cam, options=vv.make_options(**okw))
            n_want = MO.executed_samples(host, W, H, cam, options_kw=okw)
            for env, code in frames:
                with MO.knobs(ctx, env):
                    what = f"1032^3 {'oblique' if cam is CAM_A else 'axis'} {env}"
                    MO.assert_frame(ctx, M, written, tf, FILL, W, H, cam, what, options=vv.make_options(**okw))
                    lay = ctx.last_launch()
                    MO.assert_frame(ctx, M, written, tf, FILL, W, H, cam, what + " counted", options=vv.make_options(count_samples=True, **okw))
                    assert ctx.last_sample_count() == n_want, what
                    assert lay == ctx.last_launch() and lay["layout"] == code and lay["phong"] == 2, (env, lay)
                    assert (ctx.debug_counters()[2] > 0) == (code == 2), what               # waves that sampled the bricked copy
                    if code == 0:
                        assert lay["unroll"] == 3, lay
                    if cam is CAM_A:
                        assert lay["tile_log2w"] == 3 and lay["blk_log2w"] == 4, lay
                        if code == 0:
                            assert lay["lds_reserve"] == 155000, lay                         # one block per CU
                    else:
                        assert lay["tile_log2w"] == 5 and lay["blk_log2w"] == 6, lay         # a sparse frame: 64 x 4 blocks
    finally:
        with MO.knobs(ctx, {}):
            ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)                               # frees the volume and its copies for the tests that follow


# ---------------------------------------------------------------------------------------------------------------------
# 7. instruments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cam,env,code", [(CAM_A, {"VV_BRICKED": "1"}, 2), (CAM_AXIS, {"VV_ZPAIR": "0"}, 0)], ids=["oblique-bricked", "axis-linear"])
def test_mip_instruments_equal_the_march(ctx, cam, env, code):
    """mip_kernel<INSTR> and march_kernel<INSTR> execute the same samples when no ray of the march ends early (an all-zero table, a threshold no opacity
    reaches): equal counts, equal slots, the same touched bricks and the same touched lines."""
    import torch
    nx, ny, nz = 48, 40, 56
    vol = _f32(O.noise_u8(nx, ny, nz, 3))
    W, H = 120, 90
    dev = torch.device("cuda", 0)
    with MO.knobs(ctx, env):
        ctx.load_volume(vol, np.zeros(1024, np.float32))
        ctx.render_mip(W, H, cam, options=vv.make_options(step=1 / 64))                       # (builds the copy)
        assert ctx.last_launch()["layout"] == code
        line_bits = max(ctx.device_bytes()[:3]) // 128 + 64
        brick_bits = ((nx + 7) // 8) * ((ny + 7) // 8) * ((nz + 7) // 8)
        got = {}
        for kind in ("mip", "march"):
            bricks = torch.zeros((brick_bits + 31) // 32, dtype=torch.int32, device=dev)
            lines = torch.zeros((line_bits + 31) // 32, dtype=torch.int32, device=dev)
            rgba = torch.zeros(H * W, dtype=torch.int32, device=dev)
            o = dict(step=1 / 64, count_samples=True, touched_bricks=bricks.data_ptr(), touched_lines=lines.data_ptr(), touched_line_bits=line_bits)
            torch.cuda.synchronize()
            if kind == "mip":
                ctx.render_mip_device(W, H, cam, rgba.data_ptr(), 0, options=vv.make_options(**o))
            else:
                ctx.render_device(W, H, cam, rgba.data_ptr(), options=vv.make_options(ert_threshold=2.0, **o))
            torch.cuda.synchronize()
            lay = ctx.last_launch()
            assert lay["layout"] == code and lay["phong"] == (2 if kind == "mip" else 0), lay
            counters = ctx.debug_counters()
            got[kind] = (ctx.last_sample_count(), int(counters[1]), np.unpackbits(bricks.cpu().numpy().view(np.uint8)), np.unpackbits(lines.cpu().numpy().view(np.uint8)),
                         (lay["tile_log2w"], lay["blk_log2w"], lay["unroll"]))
    mip, march = got["mip"], got["march"]
    print(f"instruments {env}: samples {mip[0]} / {march[0]}, slots {mip[1]} / {march[1]}, bricks {int(mip[2].sum())} / {int(march[2].sum())}, lines {int(mip[3].sum())} / {int(march[3].sum())}")
    assert mip[4] == march[4], (mip[4], march[4])
    assert mip[0] == march[0] == MO.executed_samples(vol, W, H, cam, options_kw=dict(step=1 / 64)) and mip[0] > 0
    assert mip[1] == march[1] and mip[1] >= mip[0], (mip[1], march[1])                          # slots: 64 lanes x the trips' samples, executed or predicated off
    assert np.array_equal(mip[2], march[2]) and mip[2].sum() > 0, (int(mip[2].sum()), int(march[2].sum()))
    assert np.array_equal(mip[3], march[3]) and mip[3].sum() > 0, (int(mip[3].sum()), int(march[3].sum()))
    assert mip[2].sum() >= 0.5 * brick_bits                                                       # the frame sees most of the volume


@pytest.mark.gpu
@pytest.mark.parametrize("cam,env,code", [(CAM_A, {"VV_BRICKED": "1"}, 2), (CAM_AXIS, {"VV_ZPAIR": "0"}, 0)], ids=["oblique-bricked", "axis-linear"])
def test_reducer_kinds_instruments_equal_mip(ctx, cam, env, code):
    """proj_kernel<INSTR> in its three modes and iso_kernel<INSTR> at a level no sample reaches execute the samples of mip_kernel<INSTR>, in its trips:
    equal counts, equal slots, the same touched bricks and the same touched lines.  (The volume's values are halved: every index stays far below the level.)"""
    import torch
    nx, ny, nz = 48, 40, 56
    vol = np.ascontiguousarray(_f32(O.noise_u8(nx, ny, nz, 3)) * np.float32(0.5))
    W, H, LEVEL = 120, 90, 200
    tf = _table()
    okw = dict(step=1 / 64)
    n_want = MO.executed_samples(vol, W, H, cam, options_kw=okw)
    iso = IM.render_cam(vol, tf, W, H, cam, LEVEL, **okw)
    assert n_want > 0 and iso["count"] == n_want and not iso["index"].any() and np.isnan(iso["shade"]).all(), (n_want, iso["count"])     # no pixel has a hit
    assert PM.render_cam(vol, tf, W, H, cam, PM.PROJ_MEAN, **okw)["count"] == n_want
    dev = torch.device("cuda", 0)
    with MO.knobs(ctx, env):
        ctx.load_volume(vol, tf)
        ctx.render_mip(W, H, cam, options=vv.make_options(**okw))                                  # (builds the copy)
        assert ctx.last_launch()["layout"] == code
        line_bits = max(ctx.device_bytes()[:3]) // 128 + 64
        brick_bits = ((nx + 7) // 8) * ((ny + 7) // 8) * ((nz + 7) // 8)
        rgba = torch.zeros(H * W, dtype=torch.int32, device=dev)
        index = torch.zeros(H * W, dtype=torch.uint8, device=dev)
        record = torch.zeros(H * W * 4, dtype=torch.float32, device=dev)                          # the stat image (8 bytes a pixel) or the hit image (16)
        frames = [("mip", 2, lambda o: ctx.render_mip_device(W, H, cam, rgba.data_ptr(), index.data_ptr(), options=o))]
        frames += [(f"proj {m}", 4, lambda o, m=m: ctx.render_projection_device(W, H, cam, m, rgba.data_ptr(), index.data_ptr(), record.data_ptr(), options=o))
                   for m in (vv.PROJ_MAX, vv.PROJ_MIN, vv.PROJ_MEAN)]
        frames += [("iso", 3, lambda o: ctx.render_iso_device(W, H, cam, LEVEL, rgba.data_ptr(), index.data_ptr(), record.data_ptr(), options=o))]
        got = {}
        for kind, phong, call in frames:
            bricks = torch.zeros((brick_bits + 31) // 32, dtype=torch.int32, device=dev)
            lines = torch.zeros((line_bits + 31) // 32, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            call(vv.make_options(count_samples=True, touched_bricks=bricks.data_ptr(), touched_lines=lines.data_ptr(), touched_line_bits=line_bits, **okw))
            torch.cuda.synchronize()
            lay = ctx.last_launch()
            assert lay["layout"] == code and lay["phong"] == phong, (kind, lay)
            got[kind] = (ctx.last_sample_count(), int(ctx.debug_counters()[1]), np.unpackbits(bricks.cpu().numpy().view(np.uint8)),
                         np.unpackbits(lines.cpu().numpy().view(np.uint8)))
    mip = got.pop("mip")
    assert mip[0] == n_want and mip[1] >= mip[0] and mip[2].sum() >= 0.5 * brick_bits and mip[3].sum() > 0, (mip[0], mip[1], int(mip[2].sum()), int(mip[3].sum()))
    for kind, g in got.items():
        print(f"instruments {env} {kind}: samples {g[0]} / {mip[0]}, slots {g[1]} / {mip[1]}, bricks {int(g[2].sum())} / {int(mip[2].sum())}, lines {int(g[3].sum())} / {int(mip[3].sum())}")
        assert g[0] == mip[0] and g[1] == mip[1], (kind, g[:2], mip[:2])
        assert np.array_equal(g[2], mip[2]) and np.array_equal(g[3], mip[3]), (kind, int(g[2].sum()), int(mip[2].sum()), int(g[3].sum()), int(mip[3].sum()))
