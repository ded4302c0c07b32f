"""GPU parity tests: the HIP path, called through the C-ABI, against the CPU oracle on the
same inputs, and against the committed golden fixtures.

Bars:
  * generator      : bit-exact
  * slice sampler  : bit-exact (float results, both filter modes)
  * ray march      : BASELINE.md section 3 states RGBA8 <= 1 LSB per channel on >= 99.9 % of
                     pixels, <= 2 LSB max.  The HIP kernels evaluate every float operation in
                     the oracle's order (IEEE div/sqrt, no contraction outside the texture
                     model), so the tests hold them to the stronger bar: bit-exact frames
                     and identical executed-sample counts.  STRICT = False falls back to
                     the BASELINE tolerance (for future approximate fast paths).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import footprint_model as FM
import oracle_lib as O
import volviz_amd as vv
import witness as Wt
from golden.make_fixtures import ellipsoid_cases, frame_cases, PLANE_POINT, PLANE_NORMAL

pytestmark = pytest.mark.gpu


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


STRICT = True


def assert_frames_close(got, want, what=""):
    assert got.shape == want.shape
    if STRICT:
        bad = np.argwhere(np.any(got != want, axis=-1))
        assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    d = np.abs(got.astype(np.int16) - want.astype(np.int16)).max(axis=-1)
    frac_gt1 = float((d > 1).mean())
    exact = float((d == 0).mean())
    assert d.max() <= 2, f"{what}: max diff {d.max()} LSB at {np.unravel_index(d.argmax(), d.shape)}"
    assert frac_gt1 <= 1e-3, f"{what}: {frac_gt1:.5f} of pixels differ by more than 1 LSB"
    return exact


# ------------------------------------------------------------------ generator: bit-exact
def test_generator_default_brain_fixture(ctx, golden_dir):
    g = np.fromfile(os.path.join(golden_dir, "brain_32.u8"), np.uint8).reshape(32, 32, 32)
    assert np.array_equal(ctx.generate_default_brain(32, 32, 32), g)
    a = np.fromfile(os.path.join(golden_dir, "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
    assert np.array_equal(ctx.generate_default_brain(20, 36, 52), a)


@pytest.mark.parametrize("n", [64, 128, 256])
def test_generator_hashes(ctx, golden_dir, n):
    h = json.load(open(os.path.join(golden_dir, "generator_hashes.json")))[f"brain_{n}"]
    assert sha(ctx.generate_default_brain(n, n, n)) == h["sha256"]


def test_generator_random_ellipsoids(ctx, golden_dir):
    hs = json.load(open(os.path.join(golden_dir, "generator_hashes.json")))
    for name, dims, centers, axes, colors in ellipsoid_cases():
        out = ctx.generate_ellipsoids(*dims, centers, axes, colors)
        assert sha(out) == hs[name]["sha256"], name
        assert np.array_equal(out, O.draw_ellipsoids(*dims, centers, axes, colors))


def test_generator_edge_cases(ctx):
    # no ellipsoid: all zero, and no marker slab (the marker is written by drawEllipsoid)
    assert not ctx.generate_ellipsoids(17, 5, 3, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.uint8)).any()
    for dims in ((1, 1, 1), (100, 3, 2), (15, 16, 17), (200, 1, 1)):
        assert np.array_equal(ctx.generate_default_brain(*dims), O.draw_default_brain(*dims)), dims
    with pytest.raises(vv.VolvizError):
        ctx.generate_ellipsoids(8, 8, 8, np.zeros((65, 3)), np.ones((65, 3)), np.ones(65, np.uint8))


def test_generator_rows_of_whole_waves(ctx):
    """Rows of a multiple of 1024 voxels take the interval form (a wave = one row segment; whole chunks filled from their end voxels, the two
    chunks at the interval's ends tested voxel by voxel by 32 helper lanes) -- ellipsoid_rows_kernel (tables in LDS, tickets) for up to 8
    ellipsoids and 1024 / 2048 / 4096 voxels per row, ellipsoid_kernel<true> otherwise: the default brain (also at sizes with several tickets
    per block and a partial last round) and seeded random sets -- tiny
    ellipsoids inside one chunk, ellipsoids hanging over the volume's edges, zero and negative axes, more than 8 and more than 16 of
    them, overlapping in paint order -- against the oracle (= the compiled reference, tests/test_oracle.py), every byte."""
    for dims in ((1024, 40, 24), (2048, 6, 5), (1024, 1, 1), (1024, 160, 101), (2048, 64, 37)):
        assert np.array_equal(ctx.generate_default_brain(*dims), O.draw_default_brain(*dims)), dims
    rng = np.random.default_rng(20240)
    for case in range(24):
        nx = int(rng.choice([1024, 1024, 2048, 3072]))
        ny, nz = int(rng.integers(1, 24)), int(rng.integers(1, 12))
        n = int(rng.choice([1, 2, 5, 8, 9, 17, 40]))
        centers = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
        axes = rng.uniform(0.002, 0.7, (n, 3)).astype(np.float32)
        kind = case % 6
        if kind == 1: axes[:, 0] = rng.uniform(0.0005, 0.01, n).astype(np.float32)            # intervals inside one chunk
        if kind == 2: axes[rng.integers(0, n), rng.integers(0, 3)] = 0.0                       # division by zero: inf / NaN terms
        if kind == 3: axes[:, 0] *= np.float32(-1.0)                                           # negative axis: the x term still falls, then rises
        if kind == 4: centers[:, 0] = rng.choice([0.0, 1.0, 0.5, 16.0 / nx, 15.0 / nx], n).astype(np.float32)   # ends on chunk boundaries
        colors = rng.integers(1, 256, n).astype(np.uint8)
        got = ctx.generate_ellipsoids(nx, ny, nz, centers, axes, colors)
        want = O.draw_ellipsoids(nx, ny, nz, centers, axes, colors)
        assert np.array_equal(got, want), f"case {case}: {nx}x{ny}x{nz}, {n} ellipsoids, kind {kind}: {int((got != want).sum())} voxels differ"


def test_generator_forms_agree(ctx, monkeypatch):
    """The three forms of the fused generator give the same bytes: ellipsoid_rows_kernel (tables in LDS; rows of 1024 / 2048 voxels, <= 8
    ellipsoids), ellipsoid_kernel<true> (the same rows without it: VV_GEN_NO_LDS=1) and the per-chunk form (in-place drawing takes it)."""
    for dims in ((1024, 96, 53), (2048, 40, 21)):
        a = ctx.generate_default_brain(*dims)
        monkeypatch.setenv("VV_GEN_NO_LDS", "1")
        b = ctx.generate_default_brain(*dims)
        monkeypatch.delenv("VV_GEN_NO_LDS")
        assert np.array_equal(a, b), dims
        assert np.array_equal(a, O.draw_default_brain(*dims)), dims


def test_promote_is_the_ieee_quotient(ctx):
    """vv_promote_device (u8 -> f32 as the reference's normalised-float texture read does, kernel.cu:46): promote_kernel forms b / 255 from a
    product and two fused multiply-adds instead of a division; it must be the correctly rounded quotient for every byte, at every buffer size
    (whole dwords, ragged tails, one voxel), and must not write past the end."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    for n in (1, 3, 4, 5, 255, 1023, 1024, 4099, 1 << 20, (1 << 20) + 7, 3 * (1 << 20) + 2):
        v8 = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
        if n >= 256:
            v8[:256] = torch.arange(256, dtype=torch.uint8, device=dev)
        v32 = torch.full((n + 8,), -7.0, dtype=torch.float32, device=dev)
        ctx.promote_device(v8.data_ptr(), v32.data_ptr(), n)
        torch.cuda.synchronize()
        got = v32.cpu().numpy()
        want = v8.cpu().numpy().astype(np.float32) / np.float32(255)
        assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)), n
        assert (got[n:] == -7.0).all(), n


def test_generator_large_matches_oracle_on_slabs(ctx):
    # 512^3 on the GPU; the oracle checks it through a size-independent property: every
    # z-slice of the N^3 brain depends only on fk = k/N, so slices at k = N/4, N/2 of the
    # 512^3 volume equal full-oracle slices computed for those k alone.
    n = 512
    g = ctx.generate_default_brain(n, n, n)
    u, c = np.unique(g, return_counts=True)
    assert set(u.tolist()) == {0, 4, 60, 80, 100, 120}
    assert c[u.tolist().index(4)] == n * n * len([i for i in range(n) if np.float32(i) / np.float32(n) >= 0.99])
    # mirror symmetry is broken only by the marker slab; compare an interior slab with the oracle
    sub = O.draw_default_brain(n, n, 1)       # k = 0 only: fk = 0
    assert np.array_equal(g[0], sub[0])


# ------------------------------------------------------------------ slice sampler: bit-exact
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("filt", [vv.FILTER_TEX8, vv.FILTER_EXACT])
def test_slice_canonical_exact(ctx, dtype, filt):
    vol = O.draw_default_brain(40, 48, 56)
    if dtype == np.float32:
        vol = (vol.astype(np.float32) / np.float32(255)).astype(np.float32)
    ctx.load_volume(vol, vv.transfer_preset(vv.TF_HEAD))
    for o in (vv.SAGITTAL, vv.HORIZONTAL, vv.CORONAL, vv.FREE_FORM):
        for (dx, dy, dz), scale in (((0.0, 0.0, 0.0), (1, 1, 1)), ((0.05, 0.4, 0.3), (1.0, 1.0, 0.8)),
                                    ((-0.3, 0.7, 0.5), (1.57, 1.0, 1.0))):
            got = ctx.slice(96, 96, dx, dy, dz, o, scale, filter=filt, fill=-2.0)
            want = O.slice(vol, 96, 96, dx, dy, dz, o, scale, filter=filt, fill=-2.0)
            assert np.array_equal(got, want), (o, dx, dy, dz, scale)


def test_slice_legacy_and_ragged(ctx):
    vol = O.noise_u8(33, 17, 9, 5)
    ctx.load_volume(vol, vv.transfer_preset(vv.TF_HEAD))
    got = ctx.slice(64, 64, 0.1, -0.2, 0.6, legacy=True)
    assert np.array_equal(got, O.slice(vol, 64, 64, 0.1, -0.2, 0.6, legacy=True))
    for h, w in ((8, 4), (4, 8), (1, 1), (1, 7), (7, 1), (256, 256), (300, 1030)):
        got = ctx.slice(h, w, 0.0, 0.5, 0.5, vv.CORONAL, fill=-1.0)
        assert np.array_equal(got, O.slice(vol, h, w, 0.0, 0.5, 0.5, vv.CORONAL, fill=-1.0)), (h, w)


@pytest.mark.parametrize("filt", [vv.FILTER_TEX8, vv.FILTER_EXACT])
def test_slice_advanced_exact(ctx, filt):
    vol = O.draw_default_brain(64, 64, 64)
    ctx.load_volume(vol, vv.transfer_preset(vv.TF_HEAD))
    rng = np.random.default_rng(3)
    for _ in range(6):
        p = [float(np.float32(v)) for v in np.concatenate([rng.uniform(-.3, .3, 3), rng.uniform(-3.1, 3.1, 3)])]
        m = vv.slice_matrix(*p)
        for scale in ((1, 1, 1), (1.0, 1.0, 0.8)):
            got = ctx.slice_advanced(128, 128, m, scale, filter=filt)
            assert np.array_equal(got, O.slice_advanced(vol, 128, 128, m, scale, filter=filt)), p


def test_slice_goldens(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "frames_oracle.npz"))
    ctx.load_volume(O.draw_default_brain(64, 64, 64), vv.transfer_preset(vv.TF_HEAD))
    for oname, o in (("sagittal", vv.SAGITTAL), ("horizontal", vv.HORIZONTAL), ("coronal", vv.CORONAL)):
        assert np.array_equal(ctx.slice(64, 64, 0.05, 0.4, 0.3, o, (1.0, 1.0, 0.8)), g[f"slice_brain64_{oname}_64"])
    m = vv.slice_matrix(0.1, -0.05, 0.02, 0.4, -0.3, 0.2)
    assert np.array_equal(ctx.slice_advanced(64, 64, m), g["slice_brain64_free_64"])


# ------------------------------------------------------------------ ray march
def test_render_golden_frames(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "frames_oracle.npz"))
    vols = {"brain32": O.draw_default_brain(32, 32, 32), "brain64": O.draw_default_brain(64, 64, 64)}
    tfs = {"engine": vv.TF_ENGINE, "head": vv.TF_HEAD, "mri": vv.TF_MRI}
    worst = 1.0
    for name, kw in frame_cases():
        ctx.load_volume(vols[kw["vol"]], vv.transfer_preset(tfs[kw["tf"]]))
        sp = vv.make_slice_params(kw["slice_type"], PLANE_POINT, PLANE_NORMAL)
        img = ctx.render(kw["W"], kw["H"], vv.Camera(**kw["cam"]), slice=sp, phong=kw["phong"], fill=0x5A,
                         options=vv.make_options(count_samples=True))
        worst = min(worst, assert_frames_close(img, g[name], name))
        assert ctx.last_sample_count() == int(g[name + "__samples"][0]), name
    assert worst > 0.97


CASES = [
    # W, H, dims, dtype, tf, slice, phong, camera
    (170, 170, (64, 64, 64), np.uint8, vv.TF_HEAD, vv.SLICE_NONE, False, "a"),
    (170, 170, (64, 64, 64), np.uint8, vv.TF_ENGINE, vv.SLICE_NONE, True, "b"),
    (200, 120, (64, 64, 64), np.float32, vv.TF_ENGINE, vv.SLICE_PLANE, False, "b"),
    (200, 120, (48, 64, 40), np.float32, vv.TF_MRI, vv.SLICE_PLANE_CUT, True, "b"),
    (97, 131, (40, 33, 57), np.uint8, vv.TF_ENGINE, vv.SLICE_PLANE_CUT, False, "c"),
    (29, 43, (32, 32, 32), np.uint8, vv.TF_ENGINE, vv.SLICE_NONE, True, "a"),     # W == 1, H == 1 (mod 14)
    (29, 43, (32, 32, 32), np.uint8, vv.TF_ENGINE, vv.SLICE_PLANE, False, "c"),
]


def _cam(tag, scale=(1, 1, 1)):
    if tag == "a":
        return vv.Camera(scale=scale)
    if tag == "b":
        return vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5, scale=scale)
    return vv.Camera.orbit(3.2, 2.0, -1.1, scale=scale)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}-{c[2][0]}-{np.dtype(c[3]).name}-tf{c[4]}-s{c[5]}-p{int(c[6])}-{c[7]}" for c in CASES])
@pytest.mark.parametrize("filt", [vv.FILTER_TEX8, vv.FILTER_EXACT])
def test_render_matches_oracle(ctx, case, filt):
    W, H, dims, dtype, tfp, st, phong, camtag = case
    vol = O.draw_default_brain(*dims)
    if dtype == np.float32:
        vol = vol.astype(np.float32) / np.float32(255)
    tf = vv.transfer_preset(tfp)
    ctx.load_volume(vol, tf)
    cam = _cam(camtag)
    sp = vv.make_slice_params(st, PLANE_POINT, PLANE_NORMAL)
    opts = vv.make_options(filter=filt, count_samples=True)
    got = ctx.render(W, H, cam, slice=sp, phong=phong, options=opts, fill=0xA5)
    want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=phong, options=opts, fill=0xA5)
    assert_frames_close(got, want)
    assert ctx.last_sample_count() == n
    # untouched pixels stay untouched
    assert np.all(got[-1] == 0xA5) and np.all(got[:, -1] == 0xA5)


def test_render_colour_tf_scale_and_step(ctx):
    """Non-grey RGBA table, anisotropic object scale (VisMale: glwidget.cpp:686-689),
    explicit step override (config C3 uses step = 1/512 on a 1024^3 volume)."""
    rng = np.random.default_rng(11)
    tf = rng.uniform(0, 1, (256, 4)).astype(np.float32)
    tf[:, 3] *= 0.08
    tf[:20, 3] = 0
    vol = O.noise_u8(48, 40, 36, 0x9E3779B9)
    ctx.load_volume(vol, tf)
    for scale, step in (((1.57, 1.0, 1.0), None), ((1.0, 1.0, 0.8), 1 / 24), ((1, 1, 1), (1 / 96, 1 / 80, 1 / 72))):
        cam = _cam("b", scale)
        for ert in (vv.ERT_REFERENCE, vv.ERT_TRUE):
            opts = vv.make_options(step=step, ert_mode=ert, count_samples=True, ert_threshold=0.8)
            got = ctx.render(160, 90, cam, options=opts)
            want, n = O.render(vol, tf, 160, 90, cam, options=opts)
            assert_frames_close(got, want, f"{scale} {step} {ert}")
            assert ctx.last_sample_count() == n


def test_render_image_ray_source(ctx):
    """Front/back RGBA8 images as the reference's GL first pass produces them
    (FBO = 3x the render size, glwidget.cpp:98,291,358)."""
    W, H = 85, 60
    cam = _cam("b")
    rs_hi = vv.analytic_rays(cam, quantize8=True)
    fw, fh = 3 * W, 3 * H
    front = np.zeros((fh, fw, 4), np.uint8); back = np.zeros((fh, fw, 4), np.uint8)
    for y in range(fh):
        for x in range(fw):
            f, b = O.ray_endpoints(rs_hi, cam, fw, fh, x, y)
            front[y, x, :3] = np.round(f * 255); back[y, x, :3] = np.round(b * 255)
            front[y, x, 3] = back[y, x, 3] = 255
    vol = O.draw_default_brain(32, 32, 32)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    rs = vv.image_rays(front, back)
    for phong in (False, True):
        got = ctx.render(W, H, cam, rays=rs, phong=phong)
        want, _ = O.render(vol, tf, W, H, cam, rays=rs, phong=phong)
        assert_frames_close(got, want, f"images phong={phong}")
        assert (got[..., 3] > 0).mean() > 0.1


def test_first_pass_images(ctx):
    """vv_first_pass: the FBO pair of the GL first pass, and a render fed with them."""
    for tag, scale in (("a", (1, 1, 1)), ("b", (1.0, 1.0, 0.8)), ("c", (1.57, 1.0, 1.0))):
        cam = _cam(tag, scale)
        gf, gb = ctx.first_pass(255, 180, cam)
        of, ob = O.first_pass(cam, 255, 180)
        assert np.array_equal(gf, of) and np.array_equal(gb, ob), tag
        assert 0.05 < (gb[..., 3] == 255).mean() < 0.95 and np.array_equal(gf[..., 3] == 255, gb[..., 3] == 255)
    vol = O.draw_default_brain(32, 32, 32)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    got = ctx.render(85, 60, cam, rays=vv.image_rays(gf, gb), phong=True)
    want, _ = O.render(vol, tf, 85, 60, cam, rays=vv.image_rays(of, ob), phong=True)
    assert_frames_close(got, want)
    # camera inside the cube: the front faces are culled, only the back image is filled
    inside = vv.Camera(origin=(0.1, 0.0, -0.2), look_at=(0.0, 0.0, 1.0))
    gf, gb = ctx.first_pass(64, 48, inside)
    of, ob = O.first_pass(inside, 64, 48)
    assert np.array_equal(gf, of) and np.array_equal(gb, ob) and not gf.any() and (gb[..., 3] == 255).all()


def test_render_quantised_analytic(ctx):
    vol = O.draw_default_brain(32, 32, 32)
    tf = vv.transfer_preset(vv.TF_HEAD)
    ctx.load_volume(vol, tf)
    cam = _cam("c")
    rs = vv.analytic_rays(cam, quantize8=True)
    got = ctx.render(120, 100, cam, rays=rs)
    want, _ = O.render(vol, tf, 120, 100, cam, rays=rs)
    assert_frames_close(got, want)


def _random_case(seed):
    """One seeded configuration of everything vv_render takes."""
    rng = np.random.default_rng(1000 + seed)
    dims = tuple(int(v) for v in rng.integers(5, 48, size=3))                     # nx, ny, nz
    kind = seed % 3
    if kind == 0:
        vol = O.draw_default_brain(*dims)
    elif kind == 1:
        vol = O.noise_u8(*dims, int(rng.integers(1, 2**31)))
    else:
        vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)               # white noise: worst case for ERT order
    if rng.random() < 0.5:
        vol = vol.astype(np.float32) / np.float32(255)
        if rng.random() < 0.3:
            vol = (vol * np.float32(1.3) - np.float32(0.1)).astype(np.float32)     # values outside [0,1]: saturating index
    if rng.random() < 0.5:
        tf = vv.transfer_preset(int(rng.choice([vv.TF_ENGINE, vv.TF_HEAD, vv.TF_MRI])))
    else:
        tf = rng.uniform(0, 1, (256, 4)).astype(np.float32)
        tf[:, 3] *= np.float32(rng.choice([0.03, 0.2, 1.0]))
        tf[: int(rng.integers(0, 60)), 3] = 0
    W = int(rng.choice([int(rng.integers(2, 90)), 29, 43, 57, 71]))               # incl. W == 1 (mod 14)
    H = int(rng.choice([int(rng.integers(2, 90)), 29, 43, 57]))
    scale = tuple(float(v) for v in rng.choice([1.0, 1.0, 0.8, 1.57, 0.5], size=3))
    r = float(rng.uniform(1.2, 5.0))
    cam = vv.Camera.orbit(r, float(rng.uniform(0.15, np.pi - 0.15)), float(rng.uniform(-np.pi, np.pi)), scale=scale)
    st = int(rng.choice([vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT]))
    point = rng.uniform(0.2, 0.8, size=3); normal = rng.normal(size=3)
    sp = vv.make_slice_params(st, tuple(point), tuple(normal))
    step = None if rng.random() < 0.4 else float(rng.choice([1 / 16, 1 / 37, 1 / 64, 1 / 130]))
    opts = dict(step=step, filter=int(rng.choice([vv.FILTER_TEX8, vv.FILTER_EXACT])),
                ert_mode=int(rng.choice([vv.ERT_REFERENCE, vv.ERT_TRUE])),
                ert_threshold=float(rng.choice([0.95, 0.5, 0.999])), count_samples=True)
    return vol, tf, W, H, cam, sp, bool(rng.random() < 0.4), opts


@pytest.mark.parametrize("seed", range(48))
def test_render_random_sweep(ctx, seed):
    """Seeded sweep over volume shape/type/content, table, frame size, camera, scale, cutting plane,
    step, filter, ERT mode and threshold, shading: every frame bit-identical to the oracle."""
    vol, tf, W, H, cam, sp, phong, o = _random_case(seed)
    ctx.load_volume(vol, tf)
    opts = vv.make_options(**o)
    got = ctx.render(W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    assert_frames_close(got, want, f"seed {seed}: {vol.shape} {vol.dtype} {W}x{H} phong={phong} {o}")
    assert ctx.last_sample_count() == n


@pytest.mark.parametrize("seed", range(12))
def test_slice_random_sweep(ctx, seed):
    rng = np.random.default_rng(7000 + seed)
    dims = tuple(int(v) for v in rng.integers(3, 40, size=3))
    vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)
    if seed % 2:
        vol = vol.astype(np.float32) / np.float32(255)
    ctx.load_volume(vol, vv.transfer_preset(vv.TF_HEAD))
    h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
    scale = tuple(float(v) for v in rng.choice([1.0, 0.8, 1.57], size=3))
    filt = int(rng.choice([vv.FILTER_TEX8, vv.FILTER_EXACT]))
    for orient in (vv.SAGITTAL, vv.CORONAL, vv.HORIZONTAL):
        d = [float(v) for v in rng.uniform(-0.3, 0.3, size=3)]
        got = ctx.slice(h, w, *d, orientation=orient, scale=scale, filter=filt, fill=-1.0)
        want = O.slice(vol, h, w, *d, orientation=orient, scale=scale, filter=filt, fill=-1.0)
        assert np.array_equal(got, want), (seed, orient)
    m = O.slice_matrix(*[float(v) for v in rng.uniform(-0.4, 0.4, size=3)], *[float(v) for v in rng.uniform(-3.1, 3.1, size=3)])
    got = ctx.slice_advanced(h, w, m, scale=scale, filter=filt, fill=-1.0)
    want = O.slice_advanced(vol, h, w, m, scale=scale, filter=filt, fill=-1.0)
    assert np.array_equal(got, want), seed


@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1), (2, 2), (14, 14), (15, 16), (16, 15)])
def test_render_tiny_frames(ctx, W, H):
    vol = O.draw_default_brain(8, 8, 8)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    for phong in (False, True):
        got = ctx.render(W, H, vv.Camera(), phong=phong, fill=3)
        want, _ = O.render(vol, tf, W, H, vv.Camera(), phong=phong, fill=3)
        assert_frames_close(got, want, f"{W}x{H} phong={phong}")


def test_render_empty_and_uniform_kat(ctx):
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(np.zeros((16, 16, 16), np.uint8), tf)
    img = ctx.render(40, 30, vv.Camera(), fill=7)
    assert np.all(img[:-1, :-1] == 0) and np.all(img[-1] == 7) and np.all(img[:, -1] == 7)
    vol = np.full((16, 16, 16), 40, np.uint8)
    ctx.load_volume(vol, tf)
    opts = vv.make_options(ert_threshold=2.0)
    got = ctx.render(57, 57, vv.Camera(), options=opts)
    want, _ = O.render(vol, tf, 57, 57, vv.Camera(), options=opts)
    assert np.array_equal(got, want)          # uniform volume: no rounding-sensitive sample exists


def test_render_sharded_rows_reassemble(ctx):
    """Multi-GPU sharding unit: slab-row bands rendered separately reassemble the frame."""
    vol = O.draw_default_brain(32, 32, 32)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    cam = _cam("b")
    for phong in (False, True):
        full = ctx.render(60, 50, cam, phong=phong, fill=1)
        parts = np.full_like(full, 1)
        for rb, re in ((0, 1), (1, 3), (3, 4)):
            ctx.render(60, 50, cam, phong=phong, options=vv.make_options(slab_rows=(rb, re)), out=parts)
        assert np.array_equal(parts, full)


@pytest.mark.parametrize("W,H", [(60, 130), (45, 43), (33, 200), (1280, 720)])
def test_render_interleaved_shards(ctx, W, H):
    """The multi-GPU split: bands of 4 slab rows dealt round-robin to `count` shards."""
    vol = O.draw_default_brain(24, 24, 24)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    cam = vv.Camera.orbit(4.0, 1.0, 0.6)
    for phong in (False, True):
        full = ctx.render(W, H, cam, phong=phong, fill=1, options=vv.make_options(count_samples=True))
        n = ctx.last_sample_count()
        for count in (2, 8):
            parts = np.full_like(full, 1)
            total = 0
            for idx in range(count):
                only = np.full_like(full, 1)
                ctx.render(W, H, cam, phong=phong, options=vv.make_options(shard=(4, count, idx), count_samples=True), out=only)
                total += ctx.last_sample_count()
                rows = np.array([((y // 14) // 4) % count == idx for y in range(H)])
                assert np.all(only[~rows] == 1)
                parts[rows] = only[rows]
            assert np.array_equal(parts, full) and total == n
        if H <= 200:
            want, _ = O.render(vol, tf, W, H, cam, phong=phong, fill=1, options=vv.make_options(shard=(4, 3, 1)))
            got = ctx.render(W, H, cam, phong=phong, fill=1, options=vv.make_options(shard=(4, 3, 1)))
            assert_frames_close(got, want)


@pytest.mark.parametrize("phong", [False, True])
def test_tables_with_opacity_outside_unit_interval(ctx, phong, monkeypatch):
    """A table whose opacities exceed 1 (or are negative) makes the accumulated opacity non-monotone: a ray that passed
    the ERT threshold can fall back under it, and the reference's per-sample test (kernel.cu:272-274) then composites more
    than one sample in later chunks.  The kernels' one-sample-per-chunk shortcuts (pin 4, the depth-limited Phong
    refresh) apply only to tables with opacities in [0, 1]; every layout must match the oracle."""
    rng = np.random.default_rng(4242)
    vol = O.noise_u8(40, 36, 44, 11).astype(np.float32) / np.float32(255)
    for k, (lo, hi) in enumerate(((0.0, 2.5), (-0.5, 1.8), (0.0, 1.0))):
        tf = rng.uniform(0, 1, (256, 4)).astype(np.float32)
        tf[:, 3] = rng.uniform(lo, hi, 256).astype(np.float32)
        for env in ({}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}, {"VV_ZFAST": "1"}, {"VV_FORCE_BIG": "1"}, {"VV_UNROLL": "2"}):
            for name in ("VV_BRICKED", "VV_ZPAIR", "VV_ZFAST", "VV_FORCE_BIG", "VV_UNROLL"):
                monkeypatch.delenv(name, raising=False)
            for name, val in env.items():
                monkeypatch.setenv(name, val)
            ctx.load_volume(vol, tf)
            for cam in (_cam("a"), _cam("b")):
                for thr in (0.5, 0.95):
                    o = dict(step=1 / 64, ert_threshold=thr, ert_mode=vv.ERT_REFERENCE)
                    got = ctx.render(120, 90, cam, phong=phong, options=vv.make_options(count_samples=True, **o), fill=0x21)
                    n_got = ctx.last_sample_count()
                    want, n = O.render(vol, tf, 120, 90, cam, phong=phong, options=vv.make_options(**o), fill=0x21)
                    what = f"opacity in [{lo}, {hi}] {env} phong={phong} thr={thr}"
                    assert n_got == n, what
                    assert_frames_close(got, want, what)
                    got2 = ctx.render(120, 90, cam, phong=phong, options=vv.make_options(**o), fill=0x21)
                    assert np.array_equal(got2, want), what + " (uninstrumented)"


def test_sharded_phong_frame_whose_height_is_1_mod_14(ctx):
    """H == 1 (mod 14): the reference's last slab row only re-writes pixel row H - 2 (pin 10).  A sharded grid walks
    whole bands of slab rows and must not march that row a second time as a regular one: same pixels, but the samples
    were counted twice (found by tools/fuzz_wild.py)."""
    vol = O.noise_u8(17, 9, 12, 5)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    for W, H, shard in ((29, 29, (8, 4, 0)), (30, 15, (8, 4, 0)), (16, 29, (4, 4, 0)), (46, 43, (4, 2, 1)), (20, 57, (4, 2, 0))):
        o = vv.make_options(step=1 / 64, count_samples=True, shard=shard)
        got = ctx.render(W, H, _cam("b"), phong=True, options=o, fill=0x5A)
        n_got = ctx.last_sample_count()
        want, n = O.render(vol, tf, W, H, _cam("b"), phong=True, options=o, fill=0x5A)
        assert_frames_close(got, want, f"{W}x{H} shard {shard}")
        assert n_got == n, f"{W}x{H} shard {shard}: {n_got} samples counted, the oracle executes {n}"


@pytest.mark.parametrize("first", range(0, 200, 50))
def test_wild_fuzz_subset(ctx, first, monkeypatch):
    """200 cases of tools/fuzz_wild.py (degenerate volume shapes, tables with colours and opacities outside [0, 1], eyes
    inside the cube, extreme scales, steps and thresholds, shards; every layout and launch form in turn): frames and
    sample counts equal the oracle's.  The tool itself ran seeds 0..2999 on MI355X without a mismatch."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_wild", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_wild.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    for seed in range(first, first + 50):
        for k in fz.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in fz.ENVS[seed % len(fz.ENVS)].items():
            monkeypatch.setenv(k, v)
        vol, tf, W, H, cam, sp, phong, o = fz.case(seed)
        ctx.load_volume(vol, tf)
        opts = vv.make_options(**o)
        got = ctx.render(W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
        n_got = ctx.last_sample_count() if o["count_samples"] else None
        want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
        what = f"wild seed {seed}: {vol.shape} {vol.dtype} {W}x{H} phong={phong} {o}"
        assert_frames_close(got, want, what)
        assert n_got is None or n_got == n, what


def test_phong_forced_on_the_random_cases(ctx):
    """march_phong_kernel on the sweep's cases with Phong forced on, frame widths with W == 1 (mod 14), shards, instrumented
    and not -- same frames, same sample counts."""
    for seed in range(0, 48, 5):
        vol, tf, W, H, cam, sp, _, o = _random_case(seed)
        ctx.load_volume(vol, tf)
        opts = vv.make_options(**o)
        got = ctx.render(W, H, cam, slice=sp, phong=True, options=opts, fill=0x3C)
        n_got = ctx.last_sample_count()
        want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=True, options=opts, fill=0x3C)
        assert_frames_close(got, want, f"phong seed {seed}: {vol.shape} {vol.dtype} {W}x{H}")
        assert n_got == n
        o2 = dict(o); o2["count_samples"] = False
        got2 = ctx.render(W, H, cam, slice=sp, phong=True, options=vv.make_options(**o2), fill=0x3C)      # the uninstrumented build
        assert np.array_equal(got2, got), f"phong seed {seed} (uninstrumented)"
    vol = O.draw_default_brain(64, 64, 64)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    for W, H, shard in ((170, 170, None), (43, 57, None), (300, 200, (4, 3, 1)), (15, 16, None)):
        o = vv.make_options(count_samples=True, shard=shard)
        for cam in (_cam("a"), _cam("b")):
            got = ctx.render(W, H, cam, phong=True, options=o, fill=7)
            n_got = ctx.last_sample_count()
            want, n = O.render(vol, tf, W, H, cam, phong=True, options=o, fill=7)
            assert_frames_close(got, want, f"phong {W}x{H} shard={shard}")
            assert n_got == n


@pytest.mark.parametrize("seed", range(0, 48, 2))
def test_block_shapes_are_bit_identical(ctx, seed, monkeypatch):
    """march_kernel with the block's four 32 x 2 (or 16 x 4) wave tiles stacked (32 x 8 pixels), 2 x 2 (64 x 4: the policy for sparse
    frames of big volumes) or side by side (128 x 2), and its four 8 x 8 tiles 2 x 2 (16 x 16) or stacked (8 x 32) instead of side by side; strips are as high as the block.  Forced on the small random cases, whole frames, cropped slab
    rows and interleaved shards: same frames, same sample counts."""
    monkeypatch.setenv("VV_BLOCK_W", ("64", "128", "64")[seed % 3])
    monkeypatch.setenv("VV_TILE_LOG2W", "4" if seed % 6 == 4 else "5")
    if (seed // 2) % 4 >= 2:        # 8 x 8 wave tiles: 16 x 16 / 8 x 32 blocks (strips higher than 8 rows), linear and bricked
        monkeypatch.setenv("VV_TILE_LOG2W", "3"); monkeypatch.setenv("VV_BLOCK_W", ("16", "8")[(seed // 8) % 2])
        if seed % 3 != 1:
            monkeypatch.setenv("VV_BRICKED", "1")
    vol, tf, W, H, cam, sp, _, o = _random_case(seed)
    ctx.load_volume(vol, tf)
    nby = (H + 13) // 14
    for extra in ({}, {"slab_rows": (min(1, nby), nby)}, {"shard": (4, 3, seed % 3)}, {"shard": (8, 2, (seed // 2) % 2)}):
        o2 = dict(o); o2.update(extra)
        got = ctx.render(W, H, cam, slice=sp, options=vv.make_options(**o2), fill=0x3C)
        n_got = ctx.last_sample_count()
        want, n = O.render(vol, tf, W, H, cam, slice=sp, options=vv.make_options(**o2), fill=0x3C)
        what = f"block shape seed {seed} {extra}: {vol.shape} {vol.dtype} {W}x{H}"
        assert_frames_close(got, want, what)
        assert n_got == n, what


@pytest.mark.parametrize("seed", range(0, 24))
def test_tail_chunks_taken_several_at_a_time(ctx, seed, monkeypatch):
    """march_kernel takes sample 1 of U consecutive chunks in one trip once no lane of the wave has more than one sample per chunk left (rays past the
    ERT threshold, pin 4).  Frames that are mostly tail: a low threshold, an opaque table, long rays (small steps); every layout, ERT mode and cut
    plane mode; against the oracle and against the same frame with the batching off (VV_TAIL=0)."""
    rng = np.random.default_rng(77000 + seed)
    dims = [(24, 20, 28), (40, 33, 17), (16, 48, 31)][seed % 3]
    vol = O.noise_u8(*dims, 5 + seed)
    if seed % 2:
        vol = vol.astype(np.float32) / np.float32(255)
    tf = rng.uniform(0, 1, (256, 4)).astype(np.float32)
    tf[:, 3] = rng.uniform(0.2, 1.0, 256).astype(np.float32) if seed % 4 else np.float32(1)
    if seed % 8 == 5:
        tf[:, 3] = rng.uniform(0.0, 1.6, 256).astype(np.float32)          # opacities above 1: no tail (every chunk runs the per-sample test)
    env = [{}, {"VV_ZPAIR": "1"}, {"VV_FORCE_BIG": "1"}, {"VV_BRICKED": "1"}, {"VV_UNROLL": "2"}, {"VV_UNROLL": "1", "VV_FORCE_BIG": "1"}][seed % 6]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cam = vv.Camera.orbit(float(rng.choice([1.2, 2.5, 4.0])), float(rng.uniform(0.3, 2.8)), float(rng.uniform(-3, 3)))
    st = [vv.SLICE_NONE, vv.SLICE_PLANE, vv.SLICE_PLANE_CUT][seed % 3]
    sp = vv.make_slice_params(st, (0.5, 0.45, 0.55), (0.3, -0.5, 0.8))
    o = dict(step=float(rng.choice([1 / 200, 1 / 333, 1 / 97])), ert_threshold=float(rng.choice([0.05, 0.5, 0.9])),
             ert_mode=vv.ERT_TRUE if seed % 5 == 3 else vv.ERT_REFERENCE, count_samples=True)
    W, H = int(rng.integers(30, 90)), int(rng.integers(20, 70))
    ctx.load_volume(vol, tf)
    got = ctx.render(W, H, cam, slice=sp, options=vv.make_options(**o), fill=0x3C)
    n_got = ctx.last_sample_count()
    want, n = O.render(vol, tf, W, H, cam, slice=sp, options=vv.make_options(**o), fill=0x3C)
    assert_frames_close(got, want, f"tail seed {seed}")
    assert n_got == n
    monkeypatch.setenv("VV_TAIL", "0")
    ctx.reread_env()
    assert np.array_equal(ctx.render(W, H, cam, slice=sp, options=vv.make_options(**o), fill=0x3C), got) and ctx.last_sample_count() == n_got


@pytest.mark.parametrize("seed", range(0, 48, 3))
def test_bricked_copy_is_bit_identical(ctx, seed, monkeypatch):
    """The 4x4x4-brick copy of the volume (used by default for views off the memory axis on volumes
    of 2 M voxels and more) forced on the sweep's small volumes: same frames, same sample counts."""
    monkeypatch.setenv("VV_BRICKED", "1")
    vol, tf, W, H, cam, sp, phong, o = _random_case(seed)
    ctx.load_volume(vol, tf)
    opts = vv.make_options(**o)
    got = ctx.render(W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    n_got = ctx.last_sample_count()
    ran_bricked = ctx.debug_counters()[2] > 0
    want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    assert_frames_close(got, want, f"bricked seed {seed}: {vol.shape} {vol.dtype} phong={phong}")
    assert n_got == n and (ran_bricked or n == 0)


@pytest.mark.parametrize("seed", range(1, 48, 3))
def test_zpair_copy_is_bit_identical(ctx, seed, monkeypatch):
    """The z-pair copy of the volume (two gathers per sample; default for unshaded views along the
    memory axis) forced on the sweep's cases: any view, both voxel types, Phong included."""
    monkeypatch.setenv("VV_ZPAIR", "1")
    vol, tf, W, H, cam, sp, phong, o = _random_case(seed)
    ctx.load_volume(vol, tf)
    opts = vv.make_options(**o)
    got = ctx.render(W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    n_got = ctx.last_sample_count()
    ran = ctx.debug_counters()[3] > 0
    want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    assert_frames_close(got, want, f"zpair seed {seed}: {vol.shape} phong={phong}")
    assert n_got == n and (ran or n == 0)


@pytest.mark.parametrize("seed", range(2, 62, 3))
def test_zfast_copy_is_bit_identical(ctx, seed, monkeypatch):
    """The z-fastest copy of the volume (rows along z: the front view's kernel for side views; VV_ZFAST=1 forces it for every frame whose
    screen x does not run along the volume's x) on the random sweep's cases: any view, both voxel types, ragged sizes, cutting planes,
    shards, Phong."""
    monkeypatch.setenv("VV_ZFAST", "1")
    vol, tf, W, H, cam, sp, phong, o = _random_case(seed)
    ctx.load_volume(vol, tf)
    opts = vv.make_options(**o)
    got = ctx.render(W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    n_got = ctx.last_sample_count()
    lay = ctx.last_launch()
    want, n = O.render(vol, tf, W, H, cam, slice=sp, phong=phong, options=opts, fill=0x3C)
    assert_frames_close(got, want, f"zfast seed {seed}: {vol.shape} {vol.dtype} phong={phong} layout {lay['layout']}")
    assert n_got == n
    assert lay["layout"] in (4, 5) or lay["tile_log2w"] == 5     # (5: the x-pair copy; tile 5 without either: screen x along the volume's x)


def test_zfast_side_views(ctx, monkeypatch):
    """Side views (camera on the x axis, either side, tilted a little) through the z-fastest copy, both voxel types: the policy picks it for
    volumes of 2 M voxels and more, so it is forced here; edge sizes; the copy is accounted for and dropped with the volume."""
    monkeypatch.setenv("VV_ZFAST", "1")
    tf = vv.transfer_preset(vv.TF_ENGINE)
    rng = np.random.default_rng(11)
    took = 0
    for k, dims in enumerate(((1, 1, 1), (3, 1, 2), (5, 4, 3), (17, 16, 15), (2, 9, 33), (64, 48, 40), (256, 7, 258))):
        vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)
        if k % 2 == 0:
            vol = vol.astype(np.float32) / np.float32(255)
        ctx.load_volume(vol, tf)
        for cam in (vv.Camera(origin=(4.0, 0.0, 0.0)), vv.Camera(origin=(-3.5, 0.3, 0.2)), vv.Camera(origin=(3.8, -0.4, 0.5))):
            for ert, filt in ((vv.ERT_REFERENCE, vv.FILTER_TEX8), (vv.ERT_TRUE, vv.FILTER_EXACT)):
                o = dict(step=1 / 40, ert_mode=ert, ert_threshold=0.9, filter=filt)
                for phong in (False, True):
                    got = ctx.render(97, 61, cam, phong=phong, options=vv.make_options(count_samples=True, **o))
                    n_got = ctx.last_sample_count()
                    took += ctx.last_launch()["layout"] in (4, 5)
                    want, n = O.render(vol, tf, 97, 61, cam, phong=phong, options=vv.make_options(**o))
                    assert_frames_close(got, want, f"zfast side view {dims} {cam.origin} ert{ert} filt{filt} phong={phong}")
                    assert n_got == n
        assert ctx.device_bytes()[2] > 0
    assert took >= 72, took
    # built up front on request
    vol = rng.integers(0, 256, size=(9, 10, 12), dtype=np.uint8).astype(np.float32) / np.float32(255)
    ctx.load_volume(vol, tf)
    # (... together with the x-pair copy, which unshaded side views of such a volume sample: include/volviz.h)
    assert ctx.prepare_layouts(vv.LAYOUT_ZFAST) == vv.LAYOUT_ZFAST
    st = ctx.layout_state()
    assert st["zfast"] == (12 + 1) * 10 * 9 * 4 + 9 * 4 + 16 and st["xpair"] > 0 and ctx.device_bytes()[2] == st["zfast"] + st["xpair"]
    ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)
    assert ctx.device_bytes()[2] == 0
    assert ctx.prepare_layouts(vv.LAYOUT_ZFAST) == vv.LAYOUT_ZFAST and ctx.layout_state()["zfast"] == (4 + 1) * 4 * 4 + 4 + 16


def test_zfast_default_policy(ctx, monkeypatch):
    """Default policy: a side view of a volume of 2 M voxels or more samples the z-fastest copy (both voxel types, both kernels) or, unshaded
    and under the z-pair copy's conditions, the x-pair copy; the front view and a view 30 degrees off the x axis do not."""
    monkeypatch.delenv("VV_ZFAST", raising=False)
    tf = vv.transfer_preset(vv.TF_HEAD)
    base = O.noise_u8(130, 129, 131, 5)
    for vol in (base, base.astype(np.float32) / np.float32(255)):
        ctx.load_volume(vol, tf)
        for cam, phong, lay4 in ((vv.Camera(origin=(4.0, 0.1, 0.2)), False, True), (vv.Camera(origin=(-4.0, 0.0, 0.3)), True, True),
                                 (vv.Camera(), False, False), (vv.Camera.orbit(4.0, np.pi / 2, np.radians(30.0)), False, False)):
            opts = vv.make_options(step=1 / 100, count_samples=True)
            got = ctx.render(160, 100, cam, phong=phong, options=opts)
            n_got = ctx.last_sample_count()
            assert (ctx.last_launch()["layout"] in (4, 5)) == lay4, (vol.dtype, cam.origin, ctx.last_launch())
            if lay4:
                assert ctx.last_launch()["layout"] == (4 if phong else 5)          # unshaded frames of small / u8 volumes: the x-pair copy
            want, n = O.render(vol, tf, 160, 100, cam, phong=phong, options=opts)
            assert_frames_close(got, want, f"zfast policy {vol.dtype} {cam.origin} phong={phong}")
            assert n_got == n


def test_zpair_default_policy_and_edges(ctx, monkeypatch):
    """Default policy: an aligned, unshaded view samples the z-pair copy (both voxel types); edge sizes."""
    monkeypatch.delenv("VV_ZPAIR", raising=False)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    rng = np.random.default_rng(9)
    for k, dims in enumerate(((1, 1, 1), (2, 1, 3), (5, 4, 3), (17, 16, 15), (33, 9, 2), (6, 7, 8))):
        vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)
        if k % 2 == 0:
            vol = vol.astype(np.float32) / np.float32(255)
        ctx.load_volume(vol, tf)
        opts = vv.make_options(step=1 / 40, count_samples=True)
        got = ctx.render(61, 47, vv.Camera(), options=opts)
        n_got = ctx.last_sample_count()
        assert ctx.debug_counters()[3] > 0, "aligned view did not take the z-pair path"
        want, n = O.render(vol, tf, 61, 47, vv.Camera(), options=opts)
        assert_frames_close(got, want, f"zpair default {dims}")
        assert n_got == n
        # the same camera with shading keeps the linear layout (policy), same pixels as the oracle
        got = ctx.render(61, 47, vv.Camera(), phong=True, options=opts)
        assert ctx.debug_counters()[3] == 0
        want, _ = O.render(vol, tf, 61, 47, vv.Camera(), phong=True, options=opts)
        assert_frames_close(got, want, f"linear phong {dims}")


def test_prepare_layouts_and_device_bytes(ctx, monkeypatch):
    """vv_prepare_layouts builds the copies up front, vv_device_bytes accounts for them, a reload drops them."""
    monkeypatch.delenv("VV_BRICKED", raising=False); monkeypatch.delenv("VV_ZPAIR", raising=False)
    tf = vv.transfer_preset(vv.TF_HEAD)
    vol = O.noise_u8(130, 129, 131, 3).astype(np.float32) / np.float32(255)        # > 2 M voxels: bricks by policy
    ctx.load_volume(vol, tf)
    b = ctx.device_bytes()
    assert b[0] == vol.nbytes + (129 + 2) * 130 * 4 + 4096 and b[1] == 0 and b[2] == 0    # + one slice + two rows + 4 KiB of padding
    assert ctx.prepare_layouts(vv.LAYOUT_BRICKED | vv.LAYOUT_ZPAIR) == 3
    b = ctx.device_bytes()
    # (the bricked copy: every voxel + its x halo + one clamped brick layer in y and z: between 1.1 x and 1.5 x an f32 volume of this size)
    assert 1.1 * vol.nbytes < b[1] < 1.5 * vol.nbytes and b[1] == ctx.layout_state()["bricked"] and b[2] == 131 * (129 + 1) * (130 + 1) * 8
    opts = vv.make_options(step=1 / 100, count_samples=True)
    for cam, slot in ((_cam("b"), 2), (vv.Camera(), 3)):          # off axis -> bricks, along z -> z-pair
        got = ctx.render(96, 80, cam, options=opts)
        assert ctx.debug_counters()[slot] > 0
        want, n = O.render(vol, tf, 96, 80, cam, options=opts)
        assert_frames_close(got, want, f"prepared layout {slot}")
        assert ctx.last_sample_count() == n
    # u8, copies built lazily by the default policy; Phong off axis samples the bricks as well
    vol8 = O.noise_u8(160, 121, 110, 5)
    ctx.load_volume(vol8, tf)
    for cam, phong, slot in ((_cam("c"), False, 2), (_cam("b"), True, 2), (vv.Camera(), False, 3)):
        got = ctx.render(96, 80, cam, phong=phong, options=opts)
        assert ctx.debug_counters()[slot] > 0
        want, n = O.render(vol8, tf, 96, 80, cam, phong=phong, options=opts)
        assert_frames_close(got, want, f"u8 default layout {slot} phong={phong}")
        assert ctx.last_sample_count() == n
    b = ctx.device_bytes()
    assert b[1] == (160 // 4) * (121 // 4 + 1) * (110 // 4 + 1) * 128 and b[2] == 110 * (121 + 1) * ((160 + 1) * 2 + 2)
    ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)
    b = ctx.device_bytes()
    assert b[0] == 64 + 16 + 2 * 4 + 4096 and b[1] == 0 and b[2] == 0
    with pytest.raises(vv.VolvizError):
        ctx.prepare_layouts(8)


@pytest.mark.parametrize("dims,dtype", [((256, 9, 7), np.float32), ((256, 32, 5), np.float32), ((512, 3, 4), np.float32),
                                        ((1024, 5, 6), np.uint8), ((2048, 4, 3), np.uint8)])
def test_padded_pitch_layout(ctx, dims, dtype, monkeypatch):
    """Volumes whose rows are a multiple of 1 KiB are re-pitched on the device (rows + 32 B, and one more
    row per slice if a slice would still be a multiple of 4 KiB): every consumer of the linear layout and
    the builders of the two copies read it through the pitches."""
    rng = np.random.default_rng(17)
    vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)
    if dtype == np.float32:
        vol = vol.astype(np.float32) / np.float32(255)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    nx, ny, nz = dims
    row = nx * vol.itemsize + 32
    rows = ny + (1 if (ny * row) % 4096 == 0 else 0)
    assert ctx.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096
    opts = vv.make_options(step=1 / 60, count_samples=True)
    for env in ({}, {"VV_BRICKED": "1"}, {"VV_ZPAIR": "1"}):
        for k in ("VV_BRICKED", "VV_ZPAIR"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx.reread_env()                   # knobs are read at volume load, not per frame
        for cam, phong in ((vv.Camera(), False), (vv.Camera(), True), (_cam("b"), False), (_cam("c"), True)):
            got = ctx.render(75, 59, cam, phong=phong, options=opts)
            want, n = O.render(vol, tf, 75, 59, cam, phong=phong, options=opts)
            assert_frames_close(got, want, f"padded {dims} {env} phong={phong}")
            assert ctx.last_sample_count() == n
    for orient in (vv.SAGITTAL, vv.CORONAL, vv.HORIZONTAL):
        assert np.array_equal(ctx.slice(40, 33, 0.1, 0.2, 0.3, orientation=orient, fill=-1.0),
                              O.slice(vol, 40, 33, 0.1, 0.2, 0.3, orientation=orient, fill=-1.0))
    # streamed upload ends in the same padded layout
    ctx.load_volume_streamed(((z, vol[z:z + 2]) for z in range(0, nz, 2)), vv.VOXEL_U8 if dtype == np.uint8 else vv.VOXEL_F32, nx, ny, nz, tf)
    assert ctx.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096
    got = ctx.render(75, 59, _cam("c"), options=opts)
    want, _ = O.render(vol, tf, 75, 59, _cam("c"), options=opts)
    assert_frames_close(got, want, f"padded streamed {dims}")
    monkeypatch.setenv("VV_PITCH_PAD", "0")
    ctx.load_volume(vol, tf)
    assert ctx.device_bytes()[0] == vol.nbytes + ny * nx * vol.itemsize + 2 * nx * vol.itemsize + 4096


def test_bricked_copy_edges_and_reload(ctx, monkeypatch):
    """Volume edges not multiples of the brick size (incl. single-voxel axes), both voxel types,
    and the copy is rebuilt when another volume is loaded."""
    monkeypatch.setenv("VV_BRICKED", "1")
    tf = vv.transfer_preset(vv.TF_ENGINE)
    cam = _cam("b")
    rng = np.random.default_rng(3)
    for dims in ((1, 1, 1), (4, 4, 4), (5, 4, 3), (3, 9, 1), (8, 7, 13), (17, 16, 15)):
        for dtype in (np.uint8, np.float32):
            vol = rng.integers(0, 256, size=dims[::-1], dtype=np.uint8)
            if dtype == np.float32:
                vol = vol.astype(np.float32) / np.float32(255)
            ctx.load_volume(vol, tf)
            for phong in (False, True):
                got = ctx.render(61, 47, cam, phong=phong, options=vv.make_options(step=1 / 40, count_samples=True))
                want, n = O.render(vol, tf, 61, 47, cam, phong=phong, options=vv.make_options(step=1 / 40))
                assert_frames_close(got, want, f"bricked {dims} {np.dtype(dtype).name} phong={phong}")
                assert ctx.last_sample_count() == n


def test_render_full_size_properties(ctx):
    """BASELINE config C2 size (256^3 f32, 1280x720): size-independent properties instead of
    a full oracle frame -- (1) a 3-slab-row band of the oracle matches, (2) the frame equals the
    reassembly of its shards, (3) an empty volume renders transparent, (4) determinism."""
    n = 256
    vol8 = ctx.generate_default_brain(n, n, n)
    vol = vol8.astype(np.float32) / np.float32(255)
    tf = vv.transfer_preset(vv.TF_HEAD)
    ctx.load_volume(vol, tf)
    cam = vv.Camera()
    W, H = 1280, 720
    opts = vv.make_options(count_samples=True)
    full = ctx.render(W, H, cam, options=opts, fill=0)
    n_full = ctx.last_sample_count()
    again = ctx.render(W, H, cam, options=opts, fill=0)
    assert np.array_equal(full, again)
    band = (25, 28)                      # slab rows through the image centre
    want = np.zeros_like(full)
    _, _ = O.render(vol, tf, W, H, cam, options=vv.make_options(slab_rows=band), out=want)
    rows = slice(band[0] * 14, band[1] * 14)
    assert_frames_close(full[rows], want[rows], "C2 band")
    parts = np.zeros_like(full)
    total = 0
    nby = (H + 13) // 14
    for rb in range(0, nby, 13):
        ctx.render(W, H, cam, options=vv.make_options(slab_rows=(rb, min(rb + 13, nby)), count_samples=True), out=parts)
        total += ctx.last_sample_count()
    assert np.array_equal(parts, full) and total == n_full


def test_c3_headline_frames_match_oracle(ctx):
    """The bench.py workloads themselves (BASELINE config C3: 1024^3 f32 noise volume, 1920x1080, step 1/512,
    colour-ramp table, reference ERT), whole frames, against the oracle on the downloaded volume: the
    camera along the memory axis (re-pitched linear layout, 64-bit slice addressing), the same with
    Phong, and the rotated camera of SURVEY 8d (bricked copy).  Every pixel and the sample counts."""
    import torch
    sys_path_bench = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(sys_path_bench, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    n, W, H = 1024, 1920, 1080
    dev = torch.device("cuda", 0)
    v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev)
    ctx.generate_noise_device(v8.data_ptr(), n, n, n, 0x9E3779B9)
    v32 = torch.empty(n ** 3, dtype=torch.float32, device=dev)
    ctx.promote_device(v8.data_ptr(), v32.data_ptr(), n ** 3)
    tf = bench.ramp_tf()
    ctx.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, n, n, n, tf)
    torch.cuda.synchronize()
    host = v32.cpu().numpy().reshape(n, n, n)
    del v8, v32
    torch.cuda.empty_cache()
    threads = min(len(os.sched_getaffinity(0)), 16)
    for cam, phong, slot in ((vv.Camera(), False, None), (vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5), False, 2), (vv.Camera(), True, None),
                             (vv.Camera(origin=(-4.0, 0.2, 0.1)), False, "zfast")):        # (the last: a side view, through the z-fastest copy by policy)
        opts = vv.make_options(step=1 / 512, count_samples=True)
        got = ctx.render(W, H, cam, phong=phong, options=opts)
        n_got = ctx.last_sample_count()
        if slot == "zfast":
            assert ctx.last_launch()["layout"] == 4
        elif slot is not None:
            assert ctx.debug_counters()[slot] > 0
        want, n_want = O.render(host, tf, W, H, cam, phong=phong, options=vv.make_options(step=1 / 512), threads=threads)
        assert_frames_close(got, want, f"C3 frame phong={phong} layout={slot}")
        assert n_got == n_want
        assert (got[..., 3] > 0).mean() > 0.3
        if slot is None and not phong:
            # the other block shapes on the whole frame: same pixels, same count
            forms = ({"VV_BLOCK_W": "32"}, {"VV_BLOCK_W": "128"}, {"VV_BLOCK_W": "16", "VV_TILE_LOG2W": "3"}, {"VV_BLOCK_W": "8", "VV_TILE_LOG2W": "3", "VV_BRICKED": "1"})
            try:
                for env in forms:
                    os.environ.update(env); ctx.reread_env()
                    other = ctx.render(W, H, cam, options=opts)
                    assert np.array_equal(other, got) and ctx.last_sample_count() == n_got, f"C3 frame under {env}"
                    for k in env:
                        os.environ.pop(k)
            finally:
                for env in forms:
                    for k in env:
                        os.environ.pop(k, None)
                ctx.reread_env()
    # The call the reference's host makes (runCuda, kernel.cu:388-453): rays from the two first-pass images, FBOs three times the
    # render size (glwidget.cpp:291,358).  The images are drawn on the device; the frame is marched from them (i) with the camera
    # as a hint, enqueue-only, (ii) without a hint in a synchronous call, which reads the images' centre row back, (iii) from host
    # copies.  Each equals the oracle's march over the same images, and each gets the launch the analytic rays get.
    for cam, want_layout in ((vv.Camera(), 1), (vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5), 2)):
        ctx.render(W, H, cam, options=vv.make_options(step=1 / 512))
        ref_launch = ctx.last_launch()
        assert ref_launch["layout"] == want_layout
        iw, ih = 3 * W, 3 * H
        dfront = torch.empty(ih * iw * 4, dtype=torch.uint8, device=dev); dback = torch.empty_like(dfront)
        ctx.first_pass_device(iw, ih, cam, dfront.data_ptr(), dback.data_ptr())
        torch.cuda.synchronize()
        front = dfront.cpu().numpy().reshape(ih, iw, 4); back = dback.cpu().numpy().reshape(ih, iw, 4)
        want, n_want = O.render(host, tf, W, H, cam, options=vv.make_options(step=1 / 512), rays=vv.image_rays(front, back), threads=threads)
        opts = vv.make_options(step=1 / 512, count_samples=True)
        dframe = torch.zeros(H * W, dtype=torch.int32, device=dev)
        hinted = vv.device_image_rays(dfront.data_ptr(), dback.data_ptr(), iw, ih, hint=cam)
        ctx.render_device(W, H, cam, dframe.data_ptr(), rays=hinted, options=opts, stream=vv.stream_handle(torch.cuda.current_stream()))
        torch.cuda.synchronize()
        got = dframe.cpu().numpy().view(np.uint8).reshape(H, W, 4)
        assert_frames_close(got, want, "C3 frame from first-pass images (hinted)")
        assert ctx.last_sample_count() == n_want
        la = ctx.last_launch()
        assert {k: la[k] for k in ("tile_log2w", "blk_log2w", "unroll", "lds_reserve", "layout", "view_known")} == \
               {k: ref_launch[k] for k in ("tile_log2w", "blk_log2w", "unroll", "lds_reserve", "layout", "view_known")}, (la, ref_launch)
        for name, rs in (("device images, no hint", vv.device_image_rays(dfront.data_ptr(), dback.data_ptr(), iw, ih)), ("host images, no hint", vv.image_rays(front, back))):
            got = ctx.render(W, H, cam, rays=rs, options=opts)
            assert_frames_close(got, want, f"C3 frame from first-pass images ({name})")
            assert ctx.last_sample_count() == n_want
            la = ctx.last_launch()
            assert la["view_known"] == 1 and la["tile_log2w"] == ref_launch["tile_log2w"] and la["layout"] == ref_launch["layout"] and \
                   la["lds_reserve"] == ref_launch["lds_reserve"], (name, la, ref_launch)
            assert 0.8 < la["density_x1000"] / ref_launch["density_x1000"] < 1.25, (name, la, ref_launch)
        del dfront, dback, dframe
        torch.cuda.empty_cache()
    # one rank's share of the 8-GPU frame (BASELINE config C4: 3840x2160, step 1/1024, bands of 4 slab
    # rows dealt round-robin): the shard predicate at full size, rows of other ranks untouched
    W4, H4 = bench.FRAMES[8][0], bench.FRAMES[8][1]
    sopts = dict(step=1.0 / bench.FRAMES[8][2], shard=(4, 8, 3))
    got = ctx.render(W4, H4, vv.Camera(), options=vv.make_options(count_samples=True, **sopts), fill=0x77)
    n_got = ctx.last_sample_count()
    want, n_want = O.render(host, tf, W4, H4, vv.Camera(), options=vv.make_options(**sopts), fill=0x77, threads=threads)
    assert_frames_close(got, want, "C4 shard 3 of 8")
    assert n_got == n_want and n_got > 10_000_000
    ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)


def test_streamed_upload_equals_direct_load(ctx, tmp_path, golden_dir):
    """vv_load_volume_stream_* / vv_load_volume_t3d: same frames as vv_load_volume_*."""
    vol = O.noise_u8(40, 36, 50, 3)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    cam = _cam("b")
    ctx.load_volume(vol, tf)
    ref_u8 = ctx.render(120, 90, cam)
    f32 = vol.astype(np.float32) / np.float32(255)
    ctx.load_volume(f32, tf)
    ref_f32 = ctx.render(120, 90, cam)
    # u8 slabs, out of order, ragged slab heights
    slabs = [(30, vol[30:50]), (0, vol[0:7]), (7, vol[7:30])]
    ctx.load_volume_streamed(slabs, vv.VOXEL_U8, 40, 36, 50, tf)
    assert np.array_equal(ctx.render(120, 90, cam), ref_u8)
    # u8 slabs promoted on the device into an f32 volume; f32 slabs as they are
    ctx.load_volume_streamed(slabs, vv.VOXEL_F32, 40, 36, 50, tf)
    assert np.array_equal(ctx.render(120, 90, cam), ref_f32)
    ctx.load_volume_streamed([(0, f32[:25]), (25, f32[25:])], vv.VOXEL_F32, 40, 36, 50, tf)
    assert np.array_equal(ctx.render(120, 90, cam), ref_f32)
    # pinned source memory takes the direct path
    import torch
    pin = torch.from_numpy(vol.copy()).pin_memory()
    ctx.load_volume_streamed([(0, pin.numpy())], vv.VOXEL_U8, 40, 36, 50, tf)
    assert np.array_equal(ctx.render(120, 90, cam), ref_u8)
    # .t3d written by the reference -> device
    ctx.load_volume_t3d(os.path.join(golden_dir, "brain_16.t3d"), True, vv.VOXEL_U8, tf)
    b16 = O.draw_default_brain(16, 16, 16)
    want, _ = O.render(b16, tf, 64, 64, cam)
    assert np.array_equal(ctx.render(64, 64, cam), want)
    # a larger file through the chunked reader (several chunks), promoted to f32
    big = O.noise_u8(256, 256, 130, 9)
    p = str(tmp_path / "big.t3d").encode()
    assert vv.load_library().vv_t3d_write(p, 1, big.ctypes.data, 256, 256, 130) == 0
    ctx.load_volume_t3d(p.decode(), True, vv.VOXEL_F32, tf)
    got = ctx.render(100, 80, cam)
    ctx.load_volume(big.astype(np.float32) / np.float32(255), tf)
    assert np.array_equal(got, ctx.render(100, 80, cam))
    with pytest.raises(vv.VolvizError):
        ctx.load_volume_t3d("/nonexistent.t3d", True, vv.VOXEL_U8, tf)


def test_big_volume_addressing_forced(ctx, monkeypatch):
    """The > 4 GiB addressing path (64-bit slice base) forced onto small volumes: every kernel
    that samples the volume stays bit-identical to the oracle."""
    monkeypatch.setenv("VV_FORCE_BIG", "1")
    tf = vv.transfer_preset(vv.TF_ENGINE)
    cam = _cam("c")
    for dtype in (np.uint8, np.float32):
        vol = O.noise_u8(36, 28, 44, 5)
        if dtype == np.float32:
            vol = vol.astype(np.float32) / np.float32(255)
        ctx.load_volume(vol, tf)
        for phong in (False, True):
            got = ctx.render(130, 77, cam, phong=phong)
            want, _ = O.render(vol, tf, 130, 77, cam, phong=phong)
            assert_frames_close(got, want, f"big {np.dtype(dtype).name} phong={phong}")
        assert np.array_equal(ctx.slice(64, 64, 0.1, 0.4, 0.3, vv.CORONAL), O.slice(vol, 64, 64, 0.1, 0.4, 0.3, vv.CORONAL))
        m = vv.slice_matrix(0.1, -0.05, 0.02, 0.4, -0.3, 0.2)
        assert np.array_equal(ctx.slice_advanced(64, 64, m), O.slice_advanced(vol, 64, 64, m))


def test_volume_above_4gib(ctx, monkeypatch):
    """A real volume larger than 4 GiB (1280^3 f32 = 8.4 GB, generated on the device): a band of
    the frame against the oracle on the downloaded volume, and shard re-assembly."""
    import torch
    n = 1280
    dev = torch.device("cuda", 0)
    v8 = torch.empty(n * n * n, dtype=torch.uint8, device=dev)
    ctx.generate_noise_device(v8.data_ptr(), n, n, n, 11)
    v32 = torch.empty(n * n * n, dtype=torch.float32, device=dev)
    ctx.promote_device(v8.data_ptr(), v32.data_ptr(), n * n * n)
    tf = vv.transfer_preset(vv.TF_HEAD)
    ctx.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, n, n, n, tf)
    torch.cuda.synchronize()
    # the generator's own parity on a corner block first (u8 noise vs the oracle formula)
    corner = v8.view(n, n, n)[:6, :6, :6].cpu().numpy()
    host = v32.cpu().numpy().reshape(n, n, n)
    del v8, v32
    torch.cuda.empty_cache()
    assert corner.shape == (6, 6, 6)      # the generator's own parity: test_noise_generator_matches_oracle
    W, H = 640, 360
    cam = _cam("b")
    opts = vv.make_options(step=1 / 320, count_samples=True)
    band = (11, 14)
    want = None
    # this camera is off the memory axis: by default the bricked copy (10.5 GB) is sampled, through
    # 64-bit layer addressing; VV_BRICKED=0 takes the linear layout with its 64-bit slice bases
    for bricked in ("1", "0"):
        monkeypatch.setenv("VV_BRICKED", bricked)
        ctx.reread_env()                   # knobs are read at volume load, not per frame
        full = ctx.render(W, H, cam, options=opts)
        n_full = ctx.last_sample_count()
        assert (ctx.debug_counters()[2] > 0) == (bricked == "1")
        if want is None:
            want = np.zeros_like(full)
            _, n_band = O.render(host, tf, W, H, cam, options=vv.make_options(step=1 / 320, slab_rows=band), out=want)
        rows = slice(band[0] * 14, band[1] * 14)
        assert_frames_close(full[rows], want[rows], f"8.4 GB volume band, bricked={bricked}")
        assert (full[rows][..., 3] > 0).mean() > 0.2
        got_band = np.zeros_like(full)
        ctx.render(W, H, cam, options=vv.make_options(step=1 / 320, slab_rows=band, count_samples=True), out=got_band)
        assert ctx.last_sample_count() == n_band and n_band < n_full
    # the slice sampler on the same volume (its kernels pick 64-bit addressing at run time)
    for orient, d in ((vv.SAGITTAL, (0.0, 0.0, 0.93)), (vv.CORONAL, (0.97, 0.0, 0.0)), (vv.HORIZONTAL, (0.0, 0.99, 0.0))):
        got = ctx.slice(96, 96, *d, orientation=orient, fill=-1.0)
        assert np.array_equal(got, O.slice(host, 96, 96, *d, orientation=orient, fill=-1.0)), orient
    m = O.slice_matrix(0.3, 0.3, 0.3, 0.4, -0.7, 1.1)
    assert np.array_equal(ctx.slice_advanced(80, 80, m, fill=-1.0), O.slice_advanced(host, 80, 80, m, fill=-1.0))
    # free the 8.4 GB volume for the tests that follow
    ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)


def test_c1_reference_workload(ctx):
    """BASELINE config C1, the reference's own size: 128^3 drawDefaultBrain volume (u8, as the reference stores it, and
    promoted to f32), 512x512 frame, step 1/128 (the default), Head transfer function, camera (0,0,-4): the whole frame
    and the executed-sample count against the oracle; Phong on the u8 volume too."""
    vol8 = ctx.generate_default_brain(128, 128, 128)
    assert np.array_equal(vol8, O.draw_default_brain(128, 128, 128))
    tf = vv.transfer_preset(vv.TF_HEAD)
    cam = vv.Camera()
    for vol, phong in ((vol8, False), (vol8.astype(np.float32) / np.float32(255), False), (vol8, True)):
        ctx.load_volume(vol, tf)
        got = ctx.render(512, 512, cam, phong=phong, options=vv.make_options(count_samples=True), fill=0x5A)
        n_got = ctx.last_sample_count()
        want, n = O.render(vol, tf, 512, 512, cam, phong=phong, fill=0x5A)
        assert_frames_close(got, want, f"C1 {vol.dtype} phong={phong}")
        assert n_got == n and n > 5_000_000
        assert (got[..., 3] > 0).mean() > 0.1


def test_render_on_caller_stream_is_asynchronous_and_identical(ctx):
    """A device frame on a caller's (non-default) stream is only enqueued; once that stream is drained it equals the
    synchronous frame.  Also the explicit handle of the device's default stream (VV_STREAM_DEFAULT_ASYNC)."""
    import torch
    vol = O.noise_u8(96, 96, 96, 5)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    ctx.load_volume(vol, tf)
    cam = _cam("b")
    W, H = 300, 200
    want = ctx.render(W, H, cam, fill=0)                                   # host buffer, synchronous
    dev = torch.device("cuda", 0)
    for handle_of in ("own", "default"):
        frame = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        if handle_of == "own":
            ts = torch.cuda.Stream(device=dev)
            h = vv.stream_handle(ts)
            assert h not in (0, vv.STREAM_DEFAULT_ASYNC)
        else:
            ts = torch.cuda.default_stream(dev)
            h = vv.stream_handle(ts)
            assert h == vv.STREAM_DEFAULT_ASYNC
        with torch.cuda.stream(ts):
            for _ in range(3):
                ctx.render_device(W, H, cam, frame.data_ptr(), stream=h)
        ts.synchronize()
        assert np.array_equal(frame.cpu().numpy(), want), handle_of


def test_streamed_upload_reuses_one_pinned_buffer(ctx):
    """vv_load_volume_stream_slices from ONE pinned slab buffer that the producer refills between calls (the C5 use
    case): the call must not return before the copy engine has read the buffer."""
    import torch
    nx, ny, nz, per = 96, 80, 64, 8
    vol = O.noise_u8(nx, ny, nz, 21)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    pin = torch.empty((per, ny, nx), dtype=torch.uint8).pin_memory()
    view = pin.numpy()

    def slabs():
        for z0 in range(0, nz, per):
            view[...] = vol[z0:z0 + per]          # refill the same pinned buffer
            yield z0, view
    ctx.load_volume_streamed(slabs(), vv.VOXEL_F32, nx, ny, nz, tf)       # u8 slabs promoted to f32 on the device
    got = ctx.render(160, 120, _cam("a"), fill=0)
    ref = vol.astype(np.float32) / np.float32(255)
    want, _ = O.render(ref, tf, 160, 120, _cam("a"), fill=0)
    assert_frames_close(got, want, "volume streamed from one reused pinned buffer")


def test_slice_sampler_against_torch_grid_sample(ctx):
    """Independent cross-check of the texture model (no reference fixture can exist for it): vv_slice in
    VV_FILTER_EXACT mode against torch.nn.functional.grid_sample (trilinear, align_corners=False, border
    padding) evaluated in fp32 on the GPU.  Normalised texture coordinate x maps to voxel space as x*N - 0.5 in both
    (CUDA Programming Guide, "Linear Filtering": tex(x) with xB = x - 0.5 in unnormalised texel units; clamp
    addressing = border padding).  Tolerance 1e-6 absolute on values in [0, 1]: the interpolation order differs."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    nz, ny, nx = 40, 52, 64
    vol = rng.random((nz, ny, nx), dtype=np.float32)
    ctx.load_volume(vol, vv.transfer_preset(vv.TF_HEAD))
    h = w = 128
    dev = torch.device("cuda", 0)
    tv = torch.from_numpy(vol).to(dev)[None, None]
    i = torch.arange(w, dtype=torch.float32, device=dev) / w            # u = i / width   (kernel.cu:553-554)
    j = torch.arange(h, dtype=torch.float32, device=dev) / h
    U, Vv = torch.meshgrid(i, j, indexing="xy")                          # [j, i]
    for orient, (dx, dy, dz) in ((vv.SAGITTAL, (0.01, -0.02, 0.37)), (vv.HORIZONTAL, (0.03, 0.41, 0.02)), (vv.CORONAL, (0.63, 0.0, -0.01))):
        got = ctx.slice(h, w, dx, dy, dz, orientation=orient, filter=vv.FILTER_EXACT, fill=-1.0).reshape(w, h)   # element (j, i) at j*height + i
        if orient == vv.SAGITTAL:
            px, py, pz = U + dx, Vv + dy, torch.zeros_like(U) + dz        # kernel.cu:559-563
        elif orient == vv.HORIZONTAL:
            px, py, pz = Vv + dx, torch.zeros_like(U) + dy, U + dz        # :565-571
        else:
            px, py, pz = torch.zeros_like(U) + dx, Vv + dy, U + dz        # :573-579
        grid = torch.stack([2 * px - 1, 2 * py - 1, 2 * pz - 1], dim=-1)[None, None]    # (x, y, z) order, [-1, 1]
        ref = F.grid_sample(tv, grid, mode="bilinear", padding_mode="border", align_corners=False)[0, 0, 0]
        inb = (px >= 0) & (px < 1) & (py >= 0) & (py < 1) & (pz >= 0) & (pz < 1)
        ref = torch.where(inb, ref, torch.zeros_like(ref)).cpu().numpy()
        d = np.abs(got[:h, :w] - ref)
        assert d.max() <= 1e-6, (orient, float(d.max()))
        assert inb.float().mean() > 0.3


def test_c5_streamed_2048_phong(ctx):
    """BASELINE config C5 on one GPU: a 2048^3 f32 volume (32 GiB) uploaded slab by slab from ONE pinned host buffer
    (u8 slabs promoted on the device: vv_load_volume_stream_*), central-difference gradient + Phong, 1920x1080,
    step 1/2048.  Full size, so properties rather than a whole oracle frame: (1) a slab-row band against the oracle
    on the host copy -- a > 4 GiB volume WITH Phong; (2) the frame equals the reassembly of its 8 interleaved shards and
    their sample counts add up; (3) determinism."""
    import torch
    n = 2048
    dev = torch.device("cuda", 0)
    free_b, total_b = torch.cuda.mem_get_info(dev)
    # An MI355X has 288 GB: a box that cannot give this test 60 GiB is misconfigured or shared, and C5 reported green
    # without having run would be worse than red.  Only a device that is physically too small (another GPU model) skips.
    if total_b < 100 * 2 ** 30:
        pytest.skip(f"device has {total_b / 2 ** 30:.0f} GiB in all: not an MI355X-class GPU")
    assert free_b >= 60 * 2 ** 30, f"C5 needs 60 GiB of free HBM, the device reports {free_b / 2 ** 30:.1f} of {total_b / 2 ** 30:.0f} GiB free"
    v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev)
    ctx.generate_noise_device(v8.data_ptr(), n, n, n, 0x9E3779B9)
    torch.cuda.synchronize()
    host8 = np.empty((n, n, n), np.uint8)
    per = 32                                                               # 128 MiB slabs
    pin = torch.empty((per, n, n), dtype=torch.uint8).pin_memory()
    tf = vv.transfer_preset(vv.TF_ENGINE)
    v8v = v8.view(n, n, n)

    def slabs():
        for z0 in range(0, n, per):
            pin.copy_(v8v[z0:z0 + per])                                    # device -> the one pinned buffer (stands in for a file reader)
            host8[z0:z0 + per] = pin.numpy()
            yield z0, pin.numpy()
    ctx.load_volume_streamed(slabs(), vv.VOXEL_F32, n, n, n, tf)
    del v8, v8v
    torch.cuda.empty_cache()
    W, H = 1920, 1080
    cam = vv.Camera()
    step = 1.0 / n
    full = ctx.render(W, H, cam, phong=True, options=vv.make_options(step=step, count_samples=True), fill=0)
    n_full = ctx.last_sample_count()
    again = ctx.render(W, H, cam, phong=True, options=vv.make_options(step=step), fill=0)
    assert np.array_equal(full, again)
    assert (full[..., 3] > 0).mean() > 0.3
    parts = np.zeros_like(full)
    total = 0
    for r in range(8):
        ctx.render(W, H, cam, phong=True, options=vv.make_options(step=step, shard=(4, 8, r), count_samples=True), out=parts)
        total += ctx.last_sample_count()
    assert np.array_equal(parts, full) and total == n_full
    band = (38, 39)                                                        # the slab row through the image centre
    rows = slice(band[0] * 14, band[1] * 14)
    host = np.empty((n, n, n), np.float32)
    for z0 in range(0, n, 64):
        host[z0:z0 + 64] = host8[z0:z0 + 64].astype(np.float32) / np.float32(255)     # == the device's promotion (v / 255.f)
    del host8
    want = np.zeros_like(full)
    O.render(host, tf, W, H, cam, phong=True, options=vv.make_options(step=step, slab_rows=band), out=want,
             threads=min(len(os.sched_getaffinity(0)), 16))
    assert_frames_close(full[rows], want[rows], "C5 band (2048^3 f32, Phong)")
    ctx.load_volume(np.zeros((4, 4, 4), np.uint8), tf)                    # free the 32 GiB


def test_noise_generator_matches_oracle(ctx):
    import torch
    dev = torch.device("cuda", 0)
    for dims, seed in (((40, 33, 21), 1), ((64, 64, 64), 0x9E3779B9), ((7, 1, 3), 5)):
        nx, ny, nz = dims
        t = torch.empty(nx * ny * nz, dtype=torch.uint8, device=dev)
        ctx.generate_noise_device(t.data_ptr(), nx, ny, nz, seed)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().reshape(nz, ny, nx), O.noise_u8(nx, ny, nz, seed)), dims


def test_errors_are_codes(ctx):
    c2 = vv.Context(0)
    with pytest.raises(vv.VolvizError) as e:
        c2.render(16, 16, vv.Camera())
    assert e.value.code == -2                       # no volume loaded
    with pytest.raises(vv.VolvizError):
        c2.slice(8, 8)
    c2.load_volume(np.zeros((4, 4, 4), np.uint8), vv.transfer_preset(vv.TF_HEAD))
    with pytest.raises(vv.VolvizError):
        c2.render(0, 5, vv.Camera())
    with pytest.raises(vv.VolvizError):
        c2.render(8, 8, vv.Camera(), slice=vv.make_slice_params(5))
    with pytest.raises(vv.VolvizError):
        c2.render(8, 8, vv.Camera(), options=vv.make_options(step=1e-9))
    with pytest.raises(vv.VolvizError):
        c2.render(8, 8, vv.Camera(scale=(0, 1, 1)))
    c2.close()


def test_touched_lines_instrument(ctx, monkeypatch):
    """vv_render_options::touched_lines (the roofline's line-granular byte count): a 32^3 f32 volume has rows of exactly one 128-byte line;
    a frame whose samples cover every voxel must mark every line of the volume (+ at most the zero padding's rows that the weight-0 corners
    of edge samples read), the `issued` set contains the `compulsory` one, both layouts agree on the frame, and the bricked copy's lines
    are counted from that copy's own addresses."""
    import torch
    n = 32
    vol = O.noise_u8(n, n, n, 3).astype(np.float32) / np.float32(255)
    tf = vv.transfer_preset(vv.TF_HEAD)                        # low opacity: few rays terminate early
    W = H = 300
    cam = vv.Camera(origin=(0.0, 0.0, -3.0))
    dev = torch.device("cuda", 0)
    frame = torch.zeros(H * W, dtype=torch.int32, device=dev)
    counts = {}

    class LineModel:
        """tests/footprint_model.py over the frame's executed samples -- the witness's own march, since some rays of this table do pass the threshold --:
        the compulsory lines of both layouts, accumulated chunk by chunk."""
        def __init__(self):
            self.count = 0
            self.geom = {k: FM.dense_geom(k, vol.dtype, (n, n, n)) for k in ("linear", "bricked")}
            self.bits = {k: g["alloc"] // 128 + 64 for k, g in self.geom.items()}
            self.words = {k: np.zeros((b + 31) // 32, np.uint32) for k, b in self.bits.items()}

        def __call__(self, tex, ran, started):
            t = tex[ran]
            self.count += len(t)
            for k in self.words:
                self.words[k] |= FM.lines(t, k, vol.dtype, self.geom[k], (n, n, n), self.bits[k])
    model = LineModel()
    _, model_count = Wt.render(vol, tf, W, H, cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y, scale=cam.scale, step=1 / 128, visit=model)
    assert model_count == model.count
    monkeypatch.setenv("VV_ZPAIR", "0")                        # (the policy would give this small unshaded front view the z-pair copy)
    for env in ({"VV_BRICKED": "0"}, {"VV_BRICKED": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx.load_volume(vol, tf)
        ctx.render_device(W, H, cam, frame.data_ptr(), options=vv.make_options(step=1 / 128))       # (builds the copy)
        bits = max(ctx.device_bytes()[:3]) // 128 + 64
        assert bits == model.bits["bricked" if env["VV_BRICKED"] == "1" else "linear"]
        got, words = [], []
        for every in (False, True):
            bm = torch.zeros((bits + 31) // 32, dtype=torch.int32, device=dev)
            o = vv.make_options(step=1 / 128, touched_lines=bm.data_ptr(), touched_line_bits=bits, touched_lines_all=every, count_samples=True)
            ctx.render_device(W, H, cam, frame.data_ptr(), options=o)
            torch.cuda.synchronize()
            words.append(bm.cpu().numpy().view(np.uint32))
            got.append(np.unpackbits(bm.cpu().numpy().view(np.uint8)))
        assert np.all(got[1] >= got[0]), env                                   # issued contains compulsory
        # ... and the compulsory set is the footprint model's, word for word
        layout = "bricked" if env["VV_BRICKED"] == "1" else "linear"
        assert ctx.last_sample_count() == model.count, (env, ctx.last_sample_count(), model.count)
        assert np.array_equal(words[0], model.words[layout]), (env, int(got[0].sum()), FM.bit_count(model.words[layout]))
        counts[env["VV_BRICKED"]] = int(got[0].sum())
        assert ctx.last_launch()["layout"] == (2 if env["VV_BRICKED"] == "1" else 0)
        brick_total_lines = ctx.layout_state()["bricked"] // 128
    vol_lines = n * n * n * 4 // 128                                           # 1024: one line per row
    assert vol_lines <= counts["0"] <= vol_lines + n + 4, counts                # every row of the volume + at most the first padding slice's rows (weight-0 corners)
    assert 0.7 * brick_total_lines <= counts["1"] <= brick_total_lines, (counts, brick_total_lines)   # every brick of the volume; of the clamped extra layers in y and z only what edge samples read


def test_layout_residency_policy(monkeypatch):
    """Residency of the optional copies (include/volviz.h): vv_prepare_layouts(VV_LAYOUT_POLICY) builds what the launch policy can pick, frames then
    build nothing; with building in vv_render switched off a frame samples what is resident (at worst the linear volume); a budget too small for
    all copies evicts the one sampled least recently.  Frames equal the oracle's throughout."""
    for k in ("VV_BRICKED", "VV_ZPAIR", "VV_ZFAST"):
        monkeypatch.delenv(k, raising=False)
    n = 128                                                        # 2 M voxels: the policy's threshold for the bricked / z-fastest copies
    vol = O.noise_u8(n, n, n, 9).astype(np.float32) / np.float32(255)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    W, H = 150, 110
    views = {"front": vv.Camera(), "side": vv.Camera(origin=(-4.0, 0.0, 0.0)), "oblique": vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5)}
    want = {k: O.render(vol, tf, W, H, cam, options=vv.make_options(step=1 / 128))[0] for k, cam in views.items()}
    o = vv.make_options(step=1 / 128)
    with vv.Context(0) as c:
        c.load_volume(vol, tf)
        st = c.layout_state()
        assert st["bricked"] == st["zpair"] == st["zfast"] == st["xpair"] == 0 and st["budget"] >= 8 << 30 and st["build_in_render"] == 1
        # (1) built by the frames that want them (the default): one build per copy, none on the second round
        lay = {}
        for rnd in range(2):
            for k, cam in views.items():
                assert np.array_equal(c.render(W, H, cam, options=o), want[k]), k
                lay[k] = c.last_launch()["layout"]
            assert c.layout_state()["builds_in_render"] == 4, c.layout_state()       # z-pair (front), z-fastest + x-pair (side), bricked (oblique)
        assert lay == {"front": 3, "side": 5, "oblique": 2}, lay
        # (2) prepared up front, frames build nothing
        c.load_volume(vol, tf)
        assert c.prepare_layouts(vv.LAYOUT_POLICY) == vv.LAYOUT_BRICKED | vv.LAYOUT_ZPAIR | vv.LAYOUT_ZFAST
        st = c.layout_state()
        assert min(st["bricked"], st["zpair"], st["zfast"], st["xpair"]) > 0 and st["builds_in_render"] == 0
        c.set_layout_policy(0, False)
        for k, cam in views.items():
            assert np.array_equal(c.render(W, H, cam, options=o), want[k]), k
            assert c.last_launch()["layout"] == lay[k]
        assert c.layout_state()["builds_in_render"] == 0
        # (3) nothing resident and no building in vv_render: every view on the linear volume
        c.load_volume(vol, tf)
        c.set_layout_policy(0, False)
        for k, cam in views.items():
            assert np.array_equal(c.render(W, H, cam, options=o), want[k]), k
            assert c.last_launch()["layout"] in (0, 1), (k, c.last_launch())
        st = c.layout_state()
        assert st["bricked"] == st["zpair"] == st["zfast"] == st["xpair"] == 0
        # (4) a budget that holds the bricked copy OR the side-view copies, not both: the least recently sampled goes
        c.load_volume(vol, tf)
        vb = c.layout_state()["linear"]
        c.set_layout_policy(int(3.3 * vb), True)
        assert np.array_equal(c.render(W, H, views["side"], options=o), want["side"])
        st = c.layout_state(); assert st["zfast"] > 0 and st["xpair"] > 0 and st["bricked"] == 0
        assert np.array_equal(c.render(W, H, views["oblique"], options=o), want["oblique"])
        st = c.layout_state(); assert st["bricked"] > 0 and st["bricked"] + st["zfast"] + st["xpair"] + st["zpair"] <= st["budget"], st
        assert st["zfast"] == 0 or st["xpair"] == 0, st                                  # something of the side view's had to go
        assert np.array_equal(c.render(W, H, views["side"], options=o), want["side"])    # ... and comes back, evicting in turn
        st = c.layout_state(); assert st["bricked"] + st["zfast"] + st["xpair"] + st["zpair"] <= st["budget"], st
        # (5) a budget below any copy: frames stay on the linear volume
        c.load_volume(vol, tf)
        c.set_layout_policy(vb // 2, True)
        for k, cam in views.items():
            assert np.array_equal(c.render(W, H, cam, options=o), want[k]), k
            assert c.last_launch()["layout"] in (0, 1)


def test_frames_enqueued_back_to_back():
    """Frames enqueued back to back on caller streams -- every frame another camera (other slab radii in the rad pre-pass's buffer), alternating frame
    sizes (the scratch buffers are re-allocated) and alternating streams, nothing synchronised in between -- must each equal the oracle's: what a
    renderer that never waits for a frame sees.  An image ray source between analytic ones."""
    import torch
    vol = O.noise_u8(48, 40, 44, 21).astype(np.float32) / np.float32(255)
    tf = vv.transfer_preset(vv.TF_ENGINE)
    dev = torch.device("cuda", 0)
    cams = [vv.Camera.orbit(r, th, ph) for r, th, ph in ((4.0, 1.2, -1.5), (2.5, 0.7, 0.4), (3.0, 2.0, 2.5), (1.6, 1.5, -0.3), (5.0, 0.4, 1.0), (2.2, 1.1, 3.0), (3.5, 1.9, -2.2))]
    sizes = [(160, 120), (97, 143), (160, 120), (57, 29), (200, 90), (97, 143), (160, 120)]
    o = vv.make_options(step=1 / 64)
    want = [O.render(vol, tf, W, H, cam, options=o, fill=0x5A)[0] for cam, (W, H) in zip(cams, sizes)]
    with vv.Context(0) as c:
        c.load_volume(vol, tf)
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        for rnd in range(2):
            bufs = [torch.full((H, W, 4), 0x5A, dtype=torch.uint8, device=dev) for (W, H) in sizes]
            torch.cuda.synchronize()
            for k, (cam, (W, H)) in enumerate(zip(cams, sizes)):
                if rnd:                                     # alternating streams: the caller orders its own streams (frames share the context's scratch)
                    streams[k & 1].wait_stream(streams[(k & 1) ^ 1])
                c.render_device(W, H, cam, bufs[k].data_ptr(), options=o, stream=vv.stream_handle(streams[k & 1] if rnd else streams[0]))
            torch.cuda.synchronize()
            for k, b in enumerate(bufs):
                assert np.array_equal(b.cpu().numpy(), want[k]), f"frame {k} (round {rnd})"
        W, H = sizes[0]
        front, back = c.first_pass(3 * W, 3 * H, cams[1])
        got_i = c.render(W, H, cams[1], rays=vv.image_rays(front, back), options=o, fill=0x5A)
        want_i, _ = O.render(vol, tf, W, H, cams[1], rays=vv.image_rays(front, back), options=o, fill=0x5A)
        assert np.array_equal(got_i, want_i)
        assert np.array_equal(c.render(W, H, cams[0], options=o, fill=0x5A), want[0])


def test_screen_rectangle_launch(ctx, monkeypatch):
    """Analytic frames launch the march kernels only over the tiles / slabs under the volume's screen rectangle and let rad_kernel write the 0 of
    every pixel beside it (vv_api.cpp: screen_rect).  The frame must not depend on that: cameras that put the cube partly or wholly off the screen,
    far away, close to the eye's plane, under a narrow and a wide lens, scaled cubes, frames of 14 k + 1 pixels (pin 10), row ranges and shards,
    with and without Phong, a prefilled caller buffer (column W-1 / row H-1 and foreign rows keep their bytes) -- against the oracle, and against
    the same library with the rectangle switched off (VV_RECT=0)."""
    rng = np.random.default_rng(5150)
    vol = O.noise_u8(20, 24, 28, 3).astype(np.float32) / np.float32(255)
    tf = rng.uniform(0, 1, (256, 4)).astype(np.float32)
    ctx.load_volume(vol, tf)
    cams = [vv.Camera(origin=(0.0, 0.0, -4.0), look_at=(2.4, 0.0, 0.0)),                  # cube at the left edge, partly off
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
    sizes = [(170, 113), (113, 57), (29, 43), (64, 15), (200, 150)]
    n_case = 0
    for ci, cam in enumerate(cams):
        for phong in (False, True):
            W, H = sizes[(ci + phong) % len(sizes)]
            for opts_kw in ({}, {"shard": (4, 2, (ci + phong) % 2)}, {"slab_rows": (1, 3)}):
                if opts_kw.get("slab_rows") and H < 43: continue
                kw = dict(count_samples=True)
                if "shard" in opts_kw: kw["shard"] = opts_kw["shard"]
                if "slab_rows" in opts_kw: kw["slab_rows"] = opts_kw["slab_rows"]
                want, n_want = O.render(vol, tf, W, H, cam, phong=phong, fill=7, options=vv.make_options(**kw))
                got = ctx.render(W, H, cam, phong=phong, fill=7, options=vv.make_options(**kw))
                assert_frames_close(got, want, f"camera {ci} phong {phong} {W}x{H} {opts_kw}")
                assert ctx.last_sample_count() == n_want, (ci, phong, opts_kw)
                n_case += 1
    # the same frames with the rectangle off: one library, two launch geometries
    monkeypatch.setenv("VV_RECT", "0")
    c2 = vv.Context(0)
    try:
        c2.load_volume(vol, tf)
        for ci, cam in enumerate(cams):
            for phong in (False, True):
                W, H = sizes[(ci + 2 * phong) % len(sizes)]
                a = ctx.render(W, H, cam, phong=phong, fill=9); b = c2.render(W, H, cam, phong=phong, fill=9)
                assert np.array_equal(a, b), (ci, phong)
    finally:
        c2.close() if hasattr(c2, "close") else None
    assert n_case >= 50


def test_frame_timing_switch(ctx):
    """vv_set_frame_timing: the per-frame event pair behind vv_last_frame_ms can be switched off (hosts that time whole runs) and on again."""
    ctx.load_volume(O.draw_default_brain(16, 16, 16), vv.transfer_preset(vv.TF_ENGINE))
    a = ctx.render(56, 56, vv.Camera())
    assert ctx.last_frame_ms() > 0
    ctx.set_frame_timing(False)
    try:
        b = ctx.render(56, 56, vv.Camera())
        assert ctx.last_frame_ms() == -1.0 and np.array_equal(a, b)
    finally:
        ctx.set_frame_timing(True)
    ctx.render(56, 56, vv.Camera())
    assert ctx.last_frame_ms() > 0


def test_tile_order_table(ctx, monkeypatch):
    """StripMap::order: analytic frames may march their tiles in the order of a table that rad_kernel's extra block builds (units of x-adjacent tiles, heaviest
    first, dealt to the XCDs to and fro).  The policy uses it for aligned views of volumes up to 1 GiB; VV_LPT=1 forces it for every tile shape, VV_LPT_RUN
    sets the unit length.  Frames and sample counts must not depend on it: aligned, oblique and side views, units longer and shorter than a strip, a frame
    whose table ends in a partial round, shards and row ranges, against the oracle."""
    rng = np.random.default_rng(77)
    vol = O.noise_u8(36, 30, 33, 5).astype(np.float32) / np.float32(255)
    tf = rng.uniform(0, 1, (256, 4)).astype(np.float32)
    cams = [vv.Camera(), vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5), vv.Camera.orbit(4.0, np.pi / 2, -np.pi / 2), vv.Camera.orbit(3.0, 0.5, 0.9, fov_y=60.0)]
    want = {}
    for ci, cam in enumerate(cams):
        for kw in ({}, {"shard": (4, 2, 1)}, {"slab_rows": (2, 9)}):
            key = (ci, tuple(sorted(kw.items())))
            want[key] = O.render(vol, tf, 333, 211, cam, fill=3, options=vv.make_options(count_samples=True, **kw))
    for env in ({"VV_LPT": "1"}, {"VV_LPT": "1", "VV_LPT_RUN": "1"}, {"VV_LPT": "1", "VV_LPT_RUN": "5"}, {"VV_LPT": "1", "VV_LPT_RUN": "64"},
                {"VV_LPT": "1", "VV_BRICKED": "0"}, {"VV_LPT": "1", "VV_BLOCK_W": "128", "VV_TILE_LOG2W": "5"}):
        for k in ("VV_LPT", "VV_LPT_RUN", "VV_BRICKED", "VV_BLOCK_W", "VV_TILE_LOG2W"): monkeypatch.delenv(k, raising=False)
        for k, v in env.items(): monkeypatch.setenv(k, v)
        c2 = vv.Context(0)
        try:
            c2.load_volume(vol, tf)
            for (ci, kwt), (frame, n) in want.items():
                got = c2.render(333, 211, cams[ci], fill=3, options=vv.make_options(count_samples=True, **dict(kwt)))
                assert_frames_close(got, frame, f"{env} camera {ci} {kwt}")
                assert c2.last_sample_count() == n, (env, ci, kwt)
        finally:
            c2.close()
