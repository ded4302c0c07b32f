"""CPU tests of the product's host side: the C-ABI library loads, exports every symbol
include/volviz.h declares, and the host-only entry points agree with the golden vectors.
No kernel is launched here."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import volviz_amd as vv

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def declared_symbols():
    h = open(os.path.join(REPO, "include", "volviz.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", h)))


def test_library_exports_every_declared_symbol():
    lib = vv.load_library()
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/volviz.h but not exported"
    assert sorted(vv.EXPORTS) == syms


def test_struct_layouts_match_kernel_cuh():
    # kernel.cuh:26-40: 28 / 32 / 8 bytes
    assert C.sizeof(vv.slice_params) == 28
    assert C.sizeof(vv.camera_params) == 32
    assert C.sizeof(vv.shading_params) == 8
    assert vv.camera_params.fovX.offset == 12 and vv.camera_params.scale.offset == 20


@pytest.mark.parametrize("name,preset", [("engine", vv.TF_ENGINE), ("head", vv.TF_HEAD), ("mri", vv.TF_MRI)])
def test_transfer_presets_match_reference_tables(golden_dir, name, preset):
    g = np.fromfile(os.path.join(golden_dir, f"tf_{name}.f32"), "<f4")
    assert np.array_equal(vv.transfer_preset(preset), g)
    with pytest.raises(vv.VolvizError):
        vv.transfer_preset(17)


def test_slice_matrix_matches_reference(golden_dir):
    for case in json.load(open(os.path.join(golden_dir, "slice_matrices.json"))):
        want = np.frombuffer(bytes.fromhex(case["matrix_hex"]), np.float32).reshape(4, 4)
        assert np.array_equal(vv.slice_matrix(*case["params"]), want), case["params"]
    with pytest.raises(vv.VolvizError):          # slicewidget.cpp:149-154 asserts the range
        vv.slice_matrix(0, 0, 0, 3.3, 0, 0)


def test_cut_plane_from_euler_matches_reference(golden_dir):
    """vv_cut_plane_from_euler = the plane Window::renderSlice hands GLWidget::setSlicePro (window.cpp:425-443), bit for bit against planes
    the compiled reference's own operators produced (tests/golden/cut_planes_pro.json, make_fixtures.py cut_planes), and on 300 seeded
    random sliders over a wider angle range (tests/golden/reference_checks.json)."""
    for case in json.load(open(os.path.join(golden_dir, "cut_planes_pro.json"))):
        pt, n = vv.cut_plane_from_euler(*case["params"])
        assert pt.tobytes().hex() == case["point_hex"] and n.tobytes().hex() == case["normal_hex"], case["params"]
    pt, n = vv.cut_plane_from_euler(0, 0, 0, 0, 0, 0)
    assert pt.tolist() == [0.5, 0.5, 0.5] and n.tolist() == [0.0, 0.0, 1.0]            # the sagittal plane through the centre
    pt, n = vv.cut_plane_from_euler(0.25, 0, 0, 0, float(np.float32(np.pi / 2)), 0)      # Ry(90 deg) turns +z into +x
    assert np.allclose(n, [1, 0, 0], atol=1e-6) and pt.tolist() == [0.75, 0.5, 0.5]
    wide = json.load(open(os.path.join(golden_dir, "reference_checks.json")))["cut_planes_pro_wide"]
    assert len(wide) == 300
    for case in wide:
        pt, n = vv.cut_plane_from_euler(*case["params"])
        assert pt.tobytes().hex() == case["point_hex"] and n.tobytes().hex() == case["normal_hex"], case["params"]


def test_t3d_reads_reference_written_file(golden_dir, tmp_path):
    lib = vv.load_library()
    p = os.path.join(golden_dir, "brain_16.t3d").encode()
    nx, ny, nz = C.c_int(), C.c_int(), C.c_int()
    assert lib.vv_t3d_read_header(p, 1, C.byref(nx), C.byref(ny), C.byref(nz)) == 0
    assert (nx.value, ny.value, nz.value) == (16, 16, 16)
    buf = np.zeros(16 ** 3, np.uint8)
    assert lib.vv_t3d_read(p, 1, buf.ctypes.data, buf.size) == 0
    import oracle_lib as O
    assert np.array_equal(buf.reshape(16, 16, 16), O.draw_default_brain(16, 16, 16))
    # write -> byte-identical to what the reference wrote
    q = str(tmp_path / "out.t3d").encode()
    assert lib.vv_t3d_write(q, 1, buf.ctypes.data, 16, 16, 16) == 0
    assert open(q, "rb").read() == open(p, "rb").read()
    # header-less files are 128 x 256 x 256 (volumegenerator.cpp:204-208)
    assert lib.vv_t3d_read_header(q, 0, C.byref(nx), C.byref(ny), C.byref(nz)) == 0
    assert (nx.value, ny.value, nz.value) == (128, 256, 256)
    # errors are codes, never exit()
    assert lib.vv_t3d_read(b"/nonexistent/file.t3d", 1, buf.ctypes.data, buf.size) == -5
    assert lib.vv_t3d_read(p, 1, buf.ctypes.data, 10) == -1
    # the reference reads back what we write: our file is byte-identical to brain_16.t3d, and what the reference's loader returned
    # for that file is recorded in reference_checks.json
    back = json.load(open(os.path.join(golden_dir, "reference_checks.json")))["load_raw_brain_16"]
    assert back["count"] == 16 ** 3 and back["dims"] == [16, 16, 16]
    assert hashlib.sha256(buf.tobytes()).hexdigest() == back["sha256"]


def test_cut_plane_helpers():
    # GLWidget::setSliceCanonical (glwidget.cpp:757-776)
    for o, axis in ((vv.HORIZONTAL, 1), (vv.SAGITTAL, 2), (vv.CORONAL, 0)):
        pt, n = vv.cut_plane_canonical(o, 0.3)
        want = np.zeros(3, np.float32); want[axis] = 1
        assert np.array_equal(n, want) and np.array_equal(pt, want * np.float32(0.3))
    with pytest.raises(vv.VolvizError):
        vv.cut_plane_canonical(vv.FREE_FORM, 0.1)
    # orientation rule of glwidget.cpp:243-252
    sp = vv.cut_plane_to_slice_params(vv.SLICE_PLANE_CUT, (0.1, 0.2, 0.3), (0.0, 0.5, 0.5), flip=False)
    assert sp.type == 1 and list(sp.params) == [np.float32(v) for v in (0.1, 0.2, 0.3, -0.0, -0.5, -0.5)]
    sp = vv.cut_plane_to_slice_params(vv.SLICE_PLANE, (0.1, 0.2, 0.3), (0.0, 0.5, 0.5), flip=True)
    assert list(sp.params)[3:] == [0.0, 0.5, 0.5]
    sp = vv.cut_plane_to_slice_params(vv.SLICE_PLANE, (0, 0, 0), (1.0, -0.5, 0.0), flip=True)
    assert list(sp.params)[3:] == [-1.0, 0.5, -0.0]
    sp = vv.cut_plane_to_slice_params(vv.SLICE_PLANE, (0, 0, 0), (1.0, 1e-7, 0.0), flip=False)   # |n.y| below 1e-6: kept
    assert list(sp.params)[3:] == [1.0, np.float32(1e-7), 0.0]
    assert vv.cut_plane_to_slice_params(vv.SLICE_NONE, (1, 2, 3), (4, 5, 6)).type == -1


def test_slice_to_bgra():
    # slicewidget.cpp:108-121: grey = (unsigned)(f*255), mirrored at bits[size - offset]
    h, w = 4, 4
    buf = np.linspace(0, 1, h * w, dtype=np.float32)
    out = vv.slice_to_bgra(buf, h, w, fill=7)
    assert np.all(out[0] == 7)                               # bits[0] is never written
    for off in range(1, h * w):
        v = int(np.float32(buf[off]) * np.float32(255))
        assert list(out[h * w - off]) == [v, v, v, 255]
    # width < height: offsets beyond the buffer are skipped (the reference reads out of bounds)
    out = vv.slice_to_bgra(np.ones(8, np.float32), 4, 2, fill=9)
    written = {8 - (j * 4 + i) for j in range(4) for i in range(2) if 0 < j * 4 + i < 8}
    for k in range(8):
        assert (list(out[k]) == [255, 255, 255, 255]) == (k in written)


def test_no_gpu_means_loud_failure():
    """Without a HIP device the product must fail, not fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vv.VolvizError) as e:
        vv.Context(0)
    assert e.value.code == -3


def test_product_does_not_reference_the_oracle():
    """The product tree must not include / link / load anything under oracle/."""
    for root, _, files in os.walk(os.path.join(REPO, "volume-viz_amd")):
        if os.sep + "build" in root or os.sep + "lib" in root:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", "Makefile")):
                txt = open(os.path.join(root, f), errors="ignore").read()
                assert "vvo_" not in txt and "libvvoracle" not in txt and "libvvref" not in txt, os.path.join(root, f)


def test_tile_grid_walk():
    """bin/tile_grid_check walks the tile grid of march_kernel / mip_kernel on the CPU through the functions of csrc/vv_tiles.h that the kernels, their launchers
    and rad_kernel's table writer use: over small launches (1 ... 17 tile columns, 1 ... 9 strips, every block and wave-tile shape choose_launch reaches, XCD
    bands, order tables of unit length 1, 5 and 64, sharded bands) every tile of the launch is marched by exactly one block, no block reads beyond the
    order table, and the 256 threads of a block own 256 distinct pixels inside the block's rectangle."""
    import subprocess
    r = subprocess.run([os.path.join(REPO, "volume-viz_amd", "bin", "tile_grid_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout


def _qt_perspective(fov_deg, aspect, n, f):
    c = 1.0 / np.tan(np.radians(fov_deg) / 2.0)
    return np.array([[c / aspect, 0, 0, 0], [0, c, 0, 0], [0, 0, -(f + n) / (f - n), -2 * f * n / (f - n)], [0, 0, -1, 0]])


def _camera_transform(pos, look, up):
    look = look / np.linalg.norm(look)
    side = np.cross(look, up); side /= np.linalg.norm(side)
    upv = np.cross(side, look); upv /= np.linalg.norm(upv)
    R = np.eye(4); R[0, :3] = side; R[1, :3] = upv; R[2, :3] = -look
    T = np.eye(4); T[:3, 3] = -pos
    return R @ T                                              # camera.cpp:78-91


def test_camera_controls_match_matrix_form():
    """glwidget.cpp:426-535, 607-620 restated independently here with 4x4 matrices in double."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        pos = rng.normal(size=3) * 3 + np.array([0.3, 0.2, -4.0])
        dx, dy = int(rng.integers(-300, 300)), int(rng.integers(-300, 300))
        p2, look2 = vv.camera_orbit_drag(pos, dx, dy)
        pf = pos.astype(np.float32).astype(np.float64)
        r = np.linalg.norm(pf)
        theta = np.clip(np.arccos(pf[1] / r) - dy / 200.0, 0.1, np.pi - 0.1)
        phi = np.arctan2(pf[2], pf[0]) + dx / 200.0
        want = r * np.array([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)])
        assert np.allclose(p2, want, rtol=0, atol=2e-5 * max(1.0, r))
        assert np.allclose(look2, -want / np.linalg.norm(want), atol=1e-5)
        assert abs(np.linalg.norm(p2) - r) < 1e-4                       # the orbit keeps the radius

        look = -pos / np.linalg.norm(pos)
        assert np.allclose(vv.camera_zoom(pos, look, 120), pos + look * 0.6, atol=1e-5)
        assert np.array_equal(vv.camera_zoom(pos, look, 0), pos.astype(np.float32))

        aspect = float(rng.uniform(0.8, 2.0))
        press, release = rng.uniform(0.1, 0.9, size=2), rng.uniform(0.1, 0.9, size=2)
        up = np.array([0.0, 1.0, 0.0])
        pt, n, pu, pr = vv.cut_plane_from_drag(pos, look, up, aspect, press, release)
        f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
        inv = np.linalg.inv(_qt_perspective(45.0, f32(aspect), 0.1, 100.0) @ _camera_transform(f32(pos), f32(look), up))
        glc = lambda v: v * 2.0 - 1.0
        pr_, rl_ = f32(press), f32(release)
        front = inv @ np.array([glc(rl_[0]), -glc(rl_[1]), -1.0, 1.0]); front /= front[3]
        back = inv @ np.array([glc(rl_[0]), -glc(rl_[1]), 1.0, 1.0]); back /= back[3]
        side = inv @ np.array([glc(pr_[0]), -glc(pr_[1]), -1.0, 1.0]); side /= side[3]
        a = (back - front); a /= np.linalg.norm(a)
        b = (side - front); b /= np.linalg.norm(b)
        assert np.allclose(pt, (front[:3] + 1.0) / 2.0, atol=1e-5)
        assert np.allclose(n, np.cross(a[:3], b[:3]), atol=2e-4)     # far-plane point amplifies rounding
        assert np.allclose(pu, (inv @ np.array([0.0, -1.0, 0.0, 0.0]))[:3], atol=1e-5)
        assert np.allclose(pr, (inv @ np.array([1.0, 0.0, 0.0, 0.0]))[:3], atol=1e-5)
        # the plane contains the eye ray of the release point and the pressed near-plane point
        assert abs(np.dot(n, back[:3] - front[:3])) < 1e-2 and abs(np.dot(n, side[:3] - front[:3])) < 1e-4

        moved = vv.cut_plane_drag(pt, pu, pr, dx, dy, 1920, 1080)
        assert np.allclose(moved, pt + pr * dx / 1920 * 3.5 + pu * dy / 1080 * 3.5, atol=1e-5)
    with pytest.raises(vv.VolvizError):
        vv.camera_orbit_drag((0, 0, 0), 1, 1)


def test_developer_tools_parse():
    """tools/ holds the developer aids the profiles under profiles/ were taken with (they run on the GPU box).  None of them is part of the product;
    this keeps them from rotting silently: every Python tool compiles, every shell tool passes `bash -n`, and no tool names a `VV_*` knob the library
    does not read (a variant that sets an unknown knob would silently measure the default)."""
    import py_compile, subprocess, re
    tools = os.path.join(REPO, "tools")
    api = open(os.path.join(REPO, "volume-viz_amd", "csrc", "vv_api.cpp")).read() + open(os.path.join(REPO, "volume-viz_amd", "csrc", "vv_aux.hip")).read()
    known = set(re.findall(r'"(VV_[A-Z0-9_]+)"', api))
    known |= {"VV_LIB", "VV_BENCH_NO_EXTRA", "VV_BENCH_SPINUP", "VV_BENCH_SHARE_GPU", "VV_BENCH_SYNC_GATHER", "VV_BENCH_FRAME_SHA", "VV_STATS", "VV_CPU_THREADS",
              "VV_PITCH_PAD", "VV_PITCH_FORCE"}
    src = open(os.path.join(REPO, "volume-viz_amd", "csrc", "vv_api.cpp")).read()
    known |= set(re.findall(r'getenv\("(VV_[A-Z0-9_]+)"\)', src))
    for root, _, files in os.walk(tools):
        if "__pycache__" in root or os.sep + "bin" in root:
            continue
        for f in files:
            path = os.path.join(root, f)
            if f.endswith(".py"):
                py_compile.compile(path, doraise=True)
            elif f.endswith(".sh"):
                assert subprocess.run(["bash", "-n", path]).returncode == 0, path
            else:
                continue
            for name in set(re.findall(r"\b(VV_[A-Z][A-Z0-9_]+)\b", open(path).read())):
                if name.startswith(("VV_BENCH", "VV_GEN_")) or name in ("VV_EXPERIMENTAL", "VV_RAYS_IMAGES", "VV_RAYS_ANALYTIC"):
                    continue
                assert name in known, f"{os.path.relpath(path, REPO)} uses {name}, which nothing reads"


def test_byte_over_255_without_a_division_is_the_ieee_quotient():
    """promote_kernel (csrc/vv_aux.hip: byte_over_255) forms b / 255 as q0 = fl(b c), r = fma(-q0, 255, b), q = fma(r, c, q0) with c = fl(1 / 255).
    The claim that this is the correctly rounded binary32 quotient for every byte is checked here in exact rational arithmetic (the GPU test
    test_promote_is_the_ieee_quotient checks the kernel itself against numpy's division)."""
    from fractions import Fraction

    def rn(fr):                                   # round a rational to binary32, ties to even
        if fr == 0:
            return Fraction(0)
        sgn, a = (1 if fr > 0 else -1), abs(fr)
        e = a.numerator.bit_length() - a.denominator.bit_length()
        while Fraction(2) ** e > a: e -= 1
        while Fraction(2) ** (e + 1) <= a: e += 1
        ulp = Fraction(2) ** (e - 23)
        k = a / ulp
        kf = k.numerator // k.denominator
        rem = k - kf
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and kf % 2 == 1):
            kf += 1
        return sgn * kf * ulp

    c = rn(Fraction(1, 255))
    assert float(c) == float(np.float32(1.0) / np.float32(255.0))
    plain_wrong = 0
    for b in range(256):
        want = rn(Fraction(b, 255))
        assert float(want) == float(np.float32(b) / np.float32(255.0)), b          # the rounding helper agrees with IEEE division
        q0 = rn(b * c)
        r = rn(b - q0 * 255)                      # fma: exact product and sum, one rounding
        q = rn(q0 + r * c)
        assert q == want, b
        plain_wrong += q0 != want
    assert plain_wrong > 100                      # (the plain product b * fl(1 / 255) is off by an ulp for about half the bytes)


def test_screen_rectangle_contains_every_hit_pixel():
    """vv_render marches only under the volume's screen rectangle and writes (0,0,0,0) beside it (csrc/vv_api.cpp: screen_rect), so the rectangle must
    contain every pixel whose ray meets the cube -- as the ORACLE's binary32 ray-box test sees it (analytic_endpoints, the arithmetic ray_endpoints restates).
    Random and adversarial cameras (near, far, long and wide lenses, scaled cubes, eyes beside / above / inside the cube, odd frame sizes): every pixel the
    oracle's first pass marks visible lies inside; where no rectangle is given the whole frame is marched, which needs no check.  Also: the rectangle is not
    vacuous -- for the reference's default camera it is within 3 pixels of the hit pixels' bounding box."""
    import oracle_lib as O
    rng = np.random.default_rng(20251005)
    cams = [vv.Camera(), vv.Camera(origin=(0, 0, -40.0), fov_y=4.0), vv.Camera(origin=(0, 0, -400.0), fov_y=0.4), vv.Camera(origin=(0.3, 0.2, -1.6), fov_y=100.0),
            vv.Camera(origin=(0, 0, -1.0005)), vv.Camera(origin=(0.2, 0.1, 0.3)), vv.Camera(origin=(0, 0, -4.0), look_at=(2.4, 0, 0)),
            vv.Camera(origin=(0, 0, -4.0), look_at=(9.0, 0, 0)), vv.Camera(origin=(1e4, 2e3, -3e4), fov_y=0.005), vv.Camera(origin=(0.0, 1.2, 0.0), up=(0, 0, 1), fov_y=150.0)]
    for _ in range(260):
        r = 10.0 ** rng.uniform(-0.3, 2.5)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        scale = tuple(float(v) for v in 10.0 ** rng.uniform(-1.0, 0.6, 3)) if rng.random() < 0.5 else (1.0, 1.0, 1.0)
        target = tuple(float(v) for v in rng.uniform(-1.5, 1.5, 3)) if rng.random() < 0.5 else (0.0, 0.0, 0.0)
        up = (0.0, 1.0, 0.0) if rng.random() < 0.7 else tuple(float(v) for v in rng.normal(size=3))
        cams.append(vv.Camera(origin=tuple(float(v) for v in d * r), look_at=target, up=up, fov_y=float(10.0 ** rng.uniform(-1.5, 2.1)), scale=scale))
    n_rect = 0
    for ci, cam in enumerate(cams):
        W, H = [(97, 61), (64, 64), (131, 43), (29, 57)][ci % 4]
        try:
            rect = vv.screen_rect(cam, W, H)
        except vv.VolvizError:
            continue                                   # (up parallel to look: vv_render refuses the camera too)
        if rect is None:
            continue
        n_rect += 1
        front, back = O.first_pass(cam, W, H)
        ys, xs = np.nonzero((front[..., 3] > 0) | (back[..., 3] > 0))
        if len(xs):
            assert xs.min() >= rect[0] and xs.max() <= rect[1] and ys.min() >= rect[2] and ys.max() <= rect[3], (ci, cam, rect, xs.min(), xs.max(), ys.min(), ys.max())
        if ci == 0:
            assert xs.min() - rect[0] <= 3 and rect[1] - xs.max() <= 3 and ys.min() - rect[2] <= 3 and rect[3] - ys.max() <= 3, rect
    assert n_rect >= 100, n_rect
