"""The ray march, the MIP frame and the slice sampler held to a second, independent model (tests/witness.py).

CPU half (unmarked): the oracle against the witness, byte for byte, on one list of small cases; the witness's own checks
(its fma against libm's fmaf, the integer texture path against the fma path); and a sensitivity check: the oracle's other
arithmetic models must differ from the witness on the same cases, or the list is too tame to catch a subtly wrong kernel.

GPU half (`gpu`): the HIP kernels against the witness directly, on every layout build.  The oracle appears in no assertion
there."""
from __future__ import annotations

import ast
import ctypes
import ctypes.util
import functools
import math
import os

import numpy as np
import pytest

import oracle_lib as O
import volviz_amd as vv
import witness as Wt

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REPO = os.path.normpath(os.path.join(HERE, ".."))


# ---------------------------------------------------------------------------------------------------------------------
# inputs (numpy's generator, not the oracle's)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volume(name):
    rng = np.random.default_rng(20240917)
    if name == "brain":
        return np.fromfile(os.path.join(GOLDEN, "brain_aniso_20x36x52.u8"), np.uint8).reshape(52, 36, 20)
    if name == "noise":                                         # ragged 17 x 9 x 33
        return rng.integers(0, 256, (33, 9, 17), dtype=np.uint8)
    if name == "white":                                         # 12^3 f32; * 1.3 - 0.1: the index saturates at both ends
        return (rng.random((12, 12, 12), dtype=np.float32) * np.float32(1.3) - np.float32(0.1)).astype(np.float32)
    if name == "thin":                                          # 1 x 7 x 5: both texels of the x axis clamp to one
        return rng.integers(0, 256, (5, 7, 1), dtype=np.uint8)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def table(name):
    rng = np.random.default_rng(77)
    if name == "head":
        return np.fromfile(os.path.join(GOLDEN, "tf_head.f32"), np.float32)
    if name == "random":                                        # opacity up to 1, mostly small: rays run deep before they terminate
        t = rng.random((256, 4), dtype=np.float32)
        t[:, 3] = t[:, 3] ** 4
        t[255, 3] = 1.0
        return t.reshape(1024)
    if name == "wild":                                          # opacities outside [0, 1] (-0.1 .. 1.5): no one-sample shortcut (pin 4)
        t = rng.random((256, 4), dtype=np.float32) * np.float32(1.6) - np.float32(0.3)
        t[:, 3] = rng.random(256, dtype=np.float32) ** 4 * np.float32(1.6) - np.float32(0.1)
        return t.astype(np.float32).reshape(1024)
    raise KeyError(name)


CAMS = {
    "axis": vv.Camera(),                                        # along the memory axis
    "orbit": vv.Camera.orbit(4, math.pi / 3, math.pi / 5),
    "side": vv.Camera.orbit(4, math.pi / 2, math.pi),
    "near": vv.Camera(origin=(0.3, 0.2, -1.2), look_at=(0.0, 0.0, 0.0)),      # radius 1.2: the frustum clips the cube
}
PLANE = dict(point=(.5, .45, .55), normal=(0.3, -0.5, 0.8))
N, P, C = Wt.SLICE_NONE, Wt.SLICE_PLANE, Wt.SLICE_PLANE_CUT
T8, EX = Wt.FILTER_TEX8, Wt.FILTER_EXACT
REF, TRUE = Wt.ERT_REFERENCE, Wt.ERT_TRUE


def case(vol, W, H, cam, scale=(1, 1, 1), sl=N, step=None, filt=T8, ert=REF, thr=0.95, tf="head", phong=False, **extra):
    return dict(vol=vol, W=W, H=H, cam=cam, scale=scale, sl=sl, step=step, filt=filt, ert=ert, thr=thr, tf=tf, phong=phong, **extra)


CASES = [
    case("brain", 30, 17, "axis", phong=True),
    case("noise", 29, 15, "orbit", (1, 1, .8), P, 1 / 37, T8, TRUE, .5, "random"),
    case("white", 16, 15, "side", (1.57, 1, .5), C, None, EX, REF, .5, "wild"),
    case("thin", 2, 2, "axis", tf="random"),
    case("brain", 1, 9, "orbit"),
    case("white", 30, 17, "axis", (1, 1, 1), P, 1 / 37, T8, TRUE, .95, "head", phong=True),
    case("noise", 30, 17, "near", (1, 1, .8), C, None, EX, REF, .95, "wild", phong=True),
    case("white", 29, 15, "orbit", (1, 1, .8), N, None, T8, REF, .5, "random", phong=True),
    case("brain", 16, 15, "side", (1.57, 1, .5), P, None, EX, TRUE, .5, "wild", phong=True),
    case("noise", 30, 17, "orbit", tf="head", images=True),
    case("noise", 16, 72, "orbit", tf="random", shard=(4, 3, 1)),
    case("white", 30, 17, "orbit", (1, 1, .8), tf="random", slab_rows=(1, 2)),
    case("white", 2, 2, "near", (1, 1, 1), N, 1 / 37, T8, TRUE, .95, "random"),
    case("thin", 16, 15, "side", (1, 1, 1), P, None, EX, REF, .5, "head"),
    case("brain", 29, 15, "axis", (1, 1, 1), C, 1 / 37, T8, REF, .95, "random", quantize8=True, phong=True),
    case("white", 1, 9, "axis", (1, 1, 1), N, None, EX, TRUE, .5, "wild"),
    case("noise", 30, 17, "axis", (1, 1, 1), N, None, T8, REF, .95, "random", phong=True),
]
IDS = [f"{i}-{c['vol']}-{c['W']}x{c['H']}-{c['cam']}" for i, c in enumerate(CASES)]
PHONG = [i for i, c in enumerate(CASES) if c["phong"]]
MIP = [1, 6, 7, 14]
FILL = 0x5A


def cam_of(c):
    k = CAMS[c["cam"]]
    return vv.Camera(origin=k.origin, look_at=k.look_at, up=k.up, fov_y=k.fov_y, scale=c["scale"])


@functools.lru_cache(maxsize=None)
def images_of(i):
    """The two first-pass images of an image-sourced case: UNORM8 end points from the witness's own analytic first pass."""
    c = CASES[i]; cam = cam_of(c)
    iw, ih = 3 * c["W"], 3 * c["H"]
    y, x = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
    f, b = Wt.analytic_endpoints(iw, ih, x.ravel(), y.ravel(), cam.origin, cam.look(), cam.up, cam.fov_y, cam.scale, quantize8=True)
    img = lambda p: np.concatenate([np.rint(p * np.float32(255)).astype(np.uint8), np.full((len(p), 1), 255, np.uint8)], 1).reshape(ih, iw, 4).copy()
    return img(f), img(b)


def product_args(i, phong=False, count=True):
    """The case as the oracle and the product take it."""
    c = CASES[i]; cam = cam_of(c)
    kw = dict(slice=vv.make_slice_params(c["sl"], **PLANE),
              options=vv.make_options(step=c["step"], ert_threshold=c["thr"], filter=c["filt"], ert_mode=c["ert"],
                                      slab_rows=c.get("slab_rows", (0, 0)), shard=c.get("shard"), count_samples=count))
    if c.get("images"):
        kw["rays"] = vv.image_rays(*images_of(i), hint=cam)
    else:
        kw["rays"] = vv.analytic_rays(cam, quantize8=bool(c.get("quantize8")))
    return cam, kw


@functools.lru_cache(maxsize=None)
def witness_frame(i, phong=False, mip=False):
    """The witness's frame of case i: computed once, shared, never modified (arrays are made read-only)."""
    c = CASES[i]; cam = cam_of(c)
    both = dict(samples=0, differ=0)
    out = Wt.render(volume(c["vol"]), table(c["tf"]), c["W"], c["H"], cam_origin=cam.origin, look=cam.look(), up=cam.up, fov_y=cam.fov_y,
                    scale=cam.scale, quantize8=bool(c.get("quantize8")), images=images_of(i) if c.get("images") else None,
                    slice_type=c["sl"], plane=(*PLANE["point"], *PLANE["normal"]), phong=phong, step=c["step"], ert_threshold=c["thr"],
                    filt=c["filt"], ert_mode=c["ert"], slab_rows=c.get("slab_rows", (0, 0)), shard=c.get("shard"), fill=FILL, mip=mip,
                    both_paths=both)
    for a in out[:-1]:
        a.setflags(write=False)
    return out + (both,)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


# slice inputs shared by both halves: (height, width) incl. the ragged sizes; offsets / transforms that leave the volume on some elements
SLICE_SIZES = [(8, 4), (4, 8), (1, 7), (7, 1), (33, 40)]
SLICE_VOLS = ["noise", "white"]
SLICE_CANON = [dict(dx=0.1, dy=-0.05, dz=0.3, orientation=o, scale=s, legacy=l)
               for o, s, l in ((Wt.SAGITTAL, (1, 1, 1), False), (Wt.HORIZONTAL, (1, 1, .8), False), (Wt.CORONAL, (1.57, 1, .5), False),
                               (Wt.FREE_FORM, (1, 1, 1), False), (Wt.SAGITTAL, (1, 1, 1), True))]
SLICE_TRANS = np.array([[0.9, -0.2, 0.1, 0.05], [0.25, 0.8, -0.3, 0.2], [0.1, 0.3, 0.85, -0.1], [0, 0, 0, 1]], np.float32)
SLICE_ADV_SCALES = [(1, 1, 1), (1, 1, .8)]


def slice_inputs():
    for v in SLICE_VOLS:
        for filt in (T8, EX):
            for (h, w) in SLICE_SIZES:
                for k, kw in enumerate(SLICE_CANON):
                    yield f"{v}-f{filt}-{h}x{w}-canon{k}", v, filt, h, w, kw, None
                for s in SLICE_ADV_SCALES:
                    yield f"{v}-f{filt}-{h}x{w}-adv{s}", v, filt, h, w, None, s


@functools.lru_cache(maxsize=None)
def witness_slices():
    out = {}
    for name, v, filt, h, w, kw, s in slice_inputs():
        if kw is not None:
            out[name] = Wt.slice_canonical(volume(v), h, w, filt=filt, fill=-3.0, **kw)
        else:
            out[name] = Wt.slice_advanced(volume(v), h, w, SLICE_TRANS, scale=s, filt=filt, fill=-3.0)
        out[name].setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------------------------------
def test_witness_imports_numpy_and_the_standard_library_only():
    tree = ast.parse(open(os.path.join(HERE, "witness.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"oracle_lib", "ctypes", "volviz_amd"}, names
    assert names <= {"__future__", "math", "numpy"}, names


def test_fma_equals_libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3; libm.fmaf.restype = ctypes.c_float
    rng = np.random.default_rng(5)
    n = 100000
    a = (rng.standard_normal(3 * n) * np.exp(rng.uniform(-20, 20, 3 * n))).astype(np.float32)
    b = (rng.standard_normal(3 * n) * np.exp(rng.uniform(-20, 20, 3 * n))).astype(np.float32)
    c = (rng.standard_normal(3 * n) * np.exp(rng.uniform(-20, 20, 3 * n))).astype(np.float32)
    with np.errstate(all="ignore"):
        c[n:2 * n] = -(a[n:2 * n] * b[n:2 * n])                 # full cancellation: the result is the product's rounding error
        k = rng.integers(0, 257, n).astype(np.float32) / np.float32(256)      # the lerps' own shape: w * (b - a) + a with 1.8 weights
        a[2 * n:] = k; b[2 * n:] = rng.integers(-255, 256, n).astype(np.float32) * np.float32(2.0 ** -16) * rng.integers(1, 1 << 16, n)
    got = Wt.fma(a, b, c)
    want = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all() , int((got.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_oracle_equals_witness(i):
    c = CASES[i]; cam, kw = product_args(i)
    want, n_want, _ = witness_frame(i)
    got, n = O.render(volume(c["vol"]), table(c["tf"]), c["W"], c["H"], cam, fill=FILL, **kw)
    same(got, want, IDS[i])
    assert n == n_want
    written = (want != FILL).any(axis=-1)
    if not (c["W"] < 2 or c.get("shard")):
        assert written[:-1, :-1].any()


@pytest.mark.parametrize("i", PHONG, ids=[IDS[i] for i in PHONG])
def test_oracle_equals_witness_phong(i):
    c = CASES[i]; cam, kw = product_args(i)
    want, n_want, _ = witness_frame(i, phong=True)
    got, n = O.render(volume(c["vol"]), table(c["tf"]), c["W"], c["H"], cam, fill=FILL, phong=True, **kw)
    same(got, want, IDS[i])
    assert n == n_want
    assert (want != witness_frame(i)[0]).any(), "Phong changes nothing on this case"


def test_phong_cases_are_at_least_six():
    assert len(PHONG) >= 6


def test_integer_texture_path_equals_the_fma_path():
    samples = 0
    for i, c in enumerate(CASES):
        both = witness_frame(i)[-1]
        if volume(c["vol"]).dtype == np.uint8 and c["filt"] == T8:
            assert both["samples"] > 0
            assert both["differ"] == 0, (IDS[i], both)
            samples += both["samples"]
        else:
            assert both["samples"] == 0
    assert samples > 100000


@pytest.mark.parametrize("i", MIP, ids=[IDS[i] for i in MIP])
def test_mip_oracle_equals_witness(i):
    import mip_oracle as MO
    c = CASES[i]; cam, kw = product_args(i)
    rgba, idx, n, _ = witness_frame(i, mip=True)
    sl = vv.make_slice_params(N if c["sl"] == P else c["sl"], **PLANE)
    okw = dict(step=c["step"], filter=c["filt"], slab_rows=c.get("slab_rows", (0, 0)), shard=c.get("shard"))
    M = MO.sweep(volume(c["vol"]), c["W"], c["H"], cam, slice=sl, rays=kw["rays"], options_kw=okw)
    written = MO.written_mask(volume(c["vol"]), c["W"], c["H"], cam, slice=sl, rays=kw["rays"], options=vv.make_options(**okw))
    want_rgba, want_idx = MO.expect(M, written, table(c["tf"]), FILL)
    same(idx, want_idx, IDS[i] + ": index image")
    same(rgba, want_rgba, IDS[i] + ": rgba")
    assert n == MO.executed_samples(volume(c["vol"]), c["W"], c["H"], cam, slice=sl, rays=kw["rays"], options_kw=okw)
    assert len(np.unique(idx)) >= 20


def test_slices_oracle_equals_witness():
    ws = witness_slices()
    for name, v, filt, h, w, kw, s in slice_inputs():
        if kw is not None:
            got = O.slice(volume(v), h, w, filter=filt, fill=-3.0, **kw)
        else:
            got = O.slice_advanced(volume(v), h, w, SLICE_TRANS, scale=s, filter=filt, fill=-3.0)
        same(got.view(np.uint32), ws[name].view(np.uint32), name)
    assert any((a > 0).any() for a in ws.values())


def test_other_arithmetic_models_differ_from_the_witness():
    """The cases would catch a subtly wrong kernel: each of the oracle's other arithmetic models leaves the witness."""
    lines = ["# pixels (of those the frame writes) on which the oracle built under another arithmetic model differs from tests/witness.py",
             "# written by tests/test_witness.py::test_other_arithmetic_models_differ_from_the_witness",
             "case".ljust(28) + "".join(m.rjust(10) for m in O.MODELS[1:]) + "   pixels"]
    differ = {m: [] for m in O.MODELS[1:]}
    for i, c in enumerate(CASES):
        cam, kw = product_args(i)
        want = witness_frame(i)[0]
        row = []
        for m in O.MODELS[1:]:
            got, _ = O.render(volume(c["vol"]), table(c["tf"]), c["W"], c["H"], cam, fill=FILL, model=m, **kw)
            differ[m].append(int((got != want).any(axis=-1).sum()))
            row.append(differ[m][-1])
        lines.append(IDS[i].ljust(28) + "".join(str(r).rjust(10) for r in row) + str(int((want != FILL).any(axis=-1).sum())).rjust(9))
    try:
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "witness_sensitivity.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                    # a read-only checkout: the assertions below are the test
    for i, c in enumerate(CASES):
        if c["vol"] in ("noise", "white") and c["filt"] == T8:
            assert differ["textrunc"][i] > 0, f"textrunc does not show on {IDS[i]}"
    assert max(differ["fmad"]) > 0 and max(differ["fast"]) > 0, differ


# ---------------------------------------------------------------------------------------------------------------------
# GPU half: the kernels against the witness, no oracle
# ---------------------------------------------------------------------------------------------------------------------
BUILDS = {"default": {}, "bricked": {"VV_BRICKED": "1"}, "zpair": {"VV_ZPAIR": "1"}, "zfast": {"VV_ZFAST": "1"},
          "zfast-nopair": {"VV_ZFAST": "1", "VV_ZPAIR": "0"}, "big": {"VV_FORCE_BIG": "1"}}
KNOBS = ("VV_BRICKED", "VV_ZPAIR", "VV_ZFAST", "VV_FORCE_BIG")
LAYOUTS_SEEN = set()


def forced(ctx, monkeypatch, build):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in BUILDS[build].items():
        monkeypatch.setenv(k, v)


def load(ctx, monkeypatch, build, c):
    forced(ctx, monkeypatch, build)
    ctx.load_volume(volume(c["vol"]), table(c["tf"]))           # the knobs are read at volume load


@pytest.fixture
def knobs_restored(ctx, monkeypatch):
    yield
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    ctx.reread_env()


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_march_kernel_equals_witness(ctx, monkeypatch, knobs_restored, i, build):
    c = CASES[i]; cam, kw = product_args(i)
    want, n_want, _ = witness_frame(i)
    load(ctx, monkeypatch, build, c)
    got = ctx.render(c["W"], c["H"], cam, fill=FILL, **kw)
    n = ctx.last_sample_count()
    LAYOUTS_SEEN.add(ctx.last_launch()["layout"])
    same(got, want, f"{IDS[i]} [{build}]")
    assert n == n_want


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["default", "bricked", "big"])
@pytest.mark.parametrize("i", PHONG, ids=[IDS[i] for i in PHONG])
def test_phong_kernel_equals_witness(ctx, monkeypatch, knobs_restored, i, build):
    c = CASES[i]; cam, kw = product_args(i)
    want, n_want, _ = witness_frame(i, phong=True)
    load(ctx, monkeypatch, build, c)
    got = ctx.render(c["W"], c["H"], cam, fill=FILL, phong=True, **kw)
    n = ctx.last_sample_count()
    same(got, want, f"{IDS[i]} [{build}]")
    assert n == n_want


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("i", MIP, ids=[IDS[i] for i in MIP])
def test_mip_kernel_equals_witness(ctx, monkeypatch, knobs_restored, i, build):
    c = CASES[i]; cam, kw = product_args(i)
    want_rgba, want_idx, n_want, _ = witness_frame(i, mip=True)
    load(ctx, monkeypatch, build, c)
    rgba, idx = ctx.render_mip(c["W"], c["H"], cam, fill=FILL, return_index=True, **kw)
    n = ctx.last_sample_count()
    same(idx, want_idx, f"{IDS[i]} [{build}]: index image")
    same(rgba, want_rgba, f"{IDS[i]} [{build}]: rgba")
    assert n == n_want


@pytest.mark.gpu
def test_every_layout_was_sampled():
    """Runs after the march parametrisation (file order): the forced builds reached every layout code of vv_debug_last_launch."""
    assert LAYOUTS_SEEN >= set(range(6)), sorted(LAYOUTS_SEEN)


@pytest.mark.gpu
@pytest.mark.parametrize("v", SLICE_VOLS)
def test_slice_kernel_equals_witness(ctx, v):
    ws = witness_slices()
    ctx.load_volume(volume(v), table("head"))
    for name, vn, filt, h, w, kw, s in slice_inputs():
        if vn != v:
            continue
        if kw is not None:
            got = ctx.slice(h, w, filter=filt, fill=-3.0, **kw)
        else:
            got = ctx.slice_advanced(h, w, SLICE_TRANS, scale=s, filter=filt, fill=-3.0)
        same(got.view(np.uint32), ws[name].view(np.uint32), name)


@pytest.mark.gpu
def test_sample_count_waits_for_an_enqueued_frame_without_frame_timing(ctx):
    """vv_last_sample_count after an enqueue-only instrumented frame on a non-blocking stream, frame timing off and no other
    synchronisation: the count is the frame's (it used to wait on the timing event, which such a frame does not record)."""
    import time
    import torch
    i = 1
    c = CASES[i]; cam, kw = product_args(i)
    n_want = witness_frame(i)[1]
    ctx.load_volume(volume(c["vol"]), table(c["tf"]))
    dev = torch.device("cuda:0")
    out = torch.zeros(c["H"] * c["W"] * 4, dtype=torch.uint8, device=dev)
    a = torch.randn(4096, 4096, device=dev); b = torch.randn(4096, 4096, device=dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        for _ in range(3):                                      # warm up, then time the chain itself
            a @ b
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            a @ b
        s.synchronize()
        per = (time.perf_counter() - t0) / 10
    reps = max(10, min(2000, int(0.25 / per)))                  # a quarter of a second of queued work ahead of the frame
    ctx.set_frame_timing(False)
    try:
        ctx.render(c["W"], c["H"], cam, **product_args(i, count=False)[1])       # a finished, uninstrumented frame first: counters invalid
        with torch.cuda.stream(s):
            for _ in range(reps):
                a @ b
        ctx.render_device(c["W"], c["H"], cam, out.data_ptr(), stream=vv.stream_handle(s), **kw)
        n = ctx.last_sample_count()
    finally:
        s.synchronize()
        ctx.set_frame_timing(True)
    assert n == n_want
