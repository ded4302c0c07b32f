"""The ray march, the MIP frame and the slice sampler held to a second, independent model (tests/witness.py).

CPU half (unmarked): the oracle against the witness, byte for byte, on one list of small cases; the witness's own checks
(its fma against libm's fmaf, the integer texture path against the fma path); and a sensitivity check: the oracle's other
arithmetic models must differ from the witness on the same cases, or the list is too tame to catch a subtly wrong kernel.

GPU half (`gpu`): the HIP kernels against the witness directly, on every layout build.  The oracle appears in no assertion
there.

The value domain of f32 voxels (include/volviz.h: finite, |v| <= 2^126) is held from both sides: cases on volumes at the ends of the domain and a
table of edge values must be bit-exact like every other case; a planted block of out-of-domain voxels must leave every pixel that cannot see it
unchanged (CPU twin: test_planted_block_leaves_enough_pixels)."""
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

f32 = np.float32

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
    if name in ("ends9", "ends20", "clean20", "planted20a", "planted20b"):
        return ends_volume(name)
    raise KeyError(name)


# f32 voxels at the ends of binary32 (include/volviz.h: finite, |v| <= 2^126).  The kernels fetch the memory neighbour of an edge texel and give it
# weight 0 where this model (and the oracle) clamp the index: with every difference of two voxels finite, fma(0, b - a, a) is a and the two agree.
BIG = [f32(1e30), f32(-1e30), f32(2.0 ** 126), f32(-2.0 ** 126)]


def value_pool():
    q = lambda k: f32(k) / f32(255)
    pool = [f32(0.0), f32(-0.0), np.uint32(1).view(f32), np.uint32(0x007FFFFF).view(f32), np.finfo(f32).tiny,
            f32(1.0), f32(256) / f32(255), f32(-1e-30)] + BIG
    for k in (1, 127, 128, 254, 255):
        pool += [np.nextafter(q(k), f32(-np.inf)), np.nextafter(q(k), f32(np.inf))]
    pool += [q(1)]
    return np.array(pool, f32)


def boundary_parts(shape):
    """Every face, edge and corner of a [nz, ny, nx] volume as a boolean mask."""
    idx = np.indices(shape)
    lo = [idx[a] == 0 for a in range(3)]; hi = [idx[a] == shape[a] - 1 for a in range(3)]
    side = lambda a, s: hi[a] if s else lo[a]
    parts = {}
    for a in range(3):
        for sa in (0, 1):
            parts[f"face{a}{sa}"] = side(a, sa)
            for b in range(a + 1, 3):
                for sb in (0, 1):
                    parts[f"edge{a}{sa}{b}{sb}"] = side(a, sa) & side(b, sb)
    for c in range(8):
        parts[f"corner{c}"] = side(0, c & 1) & side(1, (c >> 1) & 1) & side(2, c >> 2)
    return parts


def ends_volume(name):
    rng = np.random.default_rng({"ends9": 9, "ends20": 20}.get(name, 2020))
    shape = (6, 7, 9) if name == "ends9" else (5, 9, 20)
    if name in ("clean20", "planted20a", "planted20b"):         # in-domain noise; planted: a 2 x 2 x 1 block of out-of-domain voxels, two voxels or more from every face
        v = (rng.random(shape, dtype=np.float32) * f32(1.3) - f32(0.1)).astype(f32)
        if name != "clean20":
            v[PLANT_Z, PLANT_Y:PLANT_Y + 2, PLANT_X:PLANT_X + 2] = np.array(PLANTED[name[-1]], f32)
        return v
    pool = value_pool()
    v = pool[rng.integers(0, len(pool), shape)]
    big = np.array(BIG, f32)[rng.integers(0, len(BIG), shape)]
    parts = boundary_parts(shape)
    surface = parts["face00"] | parts["face01"] | parts["face10"] | parts["face11"] | parts["face20"] | parts["face21"]
    corners = np.zeros(shape, bool)
    for k, m in parts.items():
        if k.startswith("corner"):
            corners |= m
    put = (surface & (rng.random(shape) < 0.5)) | corners       # at least a quarter of every face, edge and corner: test_extreme_volumes_are_as_described
    return np.where(put, big, v).astype(f32)


PLANT_X, PLANT_Y, PLANT_Z = 9, 4, 2                             # the block's lowest voxel
PLANTED = {"a": [[np.inf, -np.inf], [np.nan, 3e38]], "b": [[-3e38, 3e38], [-np.inf, np.nan]]}       # (+-3e38 side by side: their difference overflows)


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
    if name == "edge":                                          # denormal, -0.0 and > 1 colours; opacities at the threshold 1e-6 (binary32) and one ulp to either side
        t = rng.random((256, 4), dtype=np.float32)
        t[:, 3] = t[:, 3] ** 4
        kind = rng.integers(0, 6, (256, 3))
        t[:, :3] = np.select([kind == 0, kind == 1, kind == 2], [f32(1e-40), f32(-0.0), f32(1.5)], t[:, :3])
        eps = f32(1e-6)
        ak = rng.integers(0, 6, 256)
        t[:, 3] = np.select([ak == 0, ak == 1, ak == 2], [eps, np.nextafter(eps, f32(1)), np.nextafter(eps, f32(0))], t[:, 3])
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
# f32 voxels at the range ends (in domain: the kernels must equal the witness bit for bit) ...
N_PLAIN = len(CASES)
for _vi, _vol in enumerate(("ends9", "ends20")):
    for _ci, _cam in enumerate(("axis", "orbit", "side")):
        for _fi, _filt in enumerate((T8, EX)):
            _W, _H = ((30, 17), (16, 15))[(_vi + _ci + _fi) % 2]
            CASES.append(case(_vol, _W, _H, _cam, (1, 1, .8) if _ci == 1 else (1, 1, 1), (N, P, C)[(_ci + _fi) % 3], None, _filt, REF, .95, "random", phong=True))
ENDS = list(range(N_PLAIN, len(CASES)))
# ... and the same frames through a transfer table with denormal, -0.0 and > 1 colours and opacities at kEps +- 1 ulp (unshaded and MIP)
for _i in ENDS:
    CASES.append(dict(CASES[_i], tf="edge", phong=False))
EDGE_TF = list(range(ENDS[-1] + 1, len(CASES)))
IDS = [f"{i}-{c['vol']}-{c['W']}x{c['H']}-{c['cam']}" for i, c in enumerate(CASES)]
PHONG = [i for i, c in enumerate(CASES) if c["phong"]]
MIP = [1, 6, 7, 14]
MIP_ENDS = ENDS + EDGE_TF
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


def test_extreme_volumes_are_as_described():
    """The f32 volumes at the range ends: big enough for interior and edge bricks on every layout build, every value finite and within 2^126, every pool
    value present, and at least a quarter of the voxels of every face, edge and corner of magnitude >= 1e30."""
    for name, shape in (("ends9", (6, 7, 9)), ("ends20", (5, 9, 20))):
        v = volume(name)
        assert v.shape == shape and v.dtype == np.float32
        assert np.isfinite(v).all() and np.abs(v).max() == f32(2.0 ** 126)
        for part, mask in boundary_parts(shape).items():
            assert (np.abs(v[mask]) >= f32(1e30)).mean() >= 0.25, (name, part)
    both = np.concatenate([volume("ends9").ravel(), volume("ends20").ravel()])
    assert set(value_pool().view(np.uint32).tolist()) <= set(both.view(np.uint32).tolist())
    t = table("edge").reshape(256, 4)
    eps = f32(1e-6)
    for a in (eps, np.nextafter(eps, f32(1)), np.nextafter(eps, f32(0))):
        assert (t[:, 3] == a).sum() >= 8
    assert (t[:, :3] > 1).any() and (t[:, :3].view(np.uint32) == 0x80000000).any() and ((t[:, :3] > 0) & (t[:, :3] < np.finfo(f32).tiny)).any()
    assert len(ENDS) == 12 and len(EDGE_TF) == 12
    for want in ("axis", "orbit", "side"):
        for filt in (T8, EX):
            for vol in ("ends9", "ends20"):
                assert any(CASES[i]["cam"] == want and CASES[i]["filt"] == filt and CASES[i]["vol"] == vol for i in ENDS)
    assert {(CASES[i]["W"], CASES[i]["H"]) for i in ENDS} == {(30, 17), (16, 15)}


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


@pytest.mark.parametrize("i", MIP + MIP_ENDS, ids=[IDS[i] for i in MIP + MIP_ENDS])
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
    assert len(np.unique(idx)) >= (20 if i in MIP else 3)         # (voxels at the range ends mostly saturate the index)


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


# Out-of-domain voxels stay local (include/volviz.h: an Inf, a NaN or a |v| > 2^126 makes unspecified the samples within one voxel of it and nothing else).
# Which pixels cannot see the planted block, from the witness's rays in binary64: every sample position of every chunk the ray starts (entries 0 and 31,
# which only a gradient reads, included) lies more than two voxels from each planted voxel along at least one axis -- the trilinear footprint of such a
# sample, the weight-0 neighbour the kernels fetch included, cannot contain the voxel.  (Read as "along all three axes at once" the rule would keep no
# sample of a volume five voxels deep; two voxels along one axis is twice what the footprint needs.)
LOCAL = [dict(cam="axis", filt=T8, scale=(1, 1, 1)), dict(cam="orbit", filt=EX, scale=(1, 1, .8))]
LOCAL_W, LOCAL_H = 30, 17


@functools.lru_cache(maxsize=None)
def far_pixels(k, phong):
    """(kept [H, W], meets [H, W]): pixels whose ray meets the volume, and those of them held to equality."""
    c = LOCAL[k]; kc = CAMS[c["cam"]]
    cam = vv.Camera(origin=kc.origin, look_at=kc.look_at, up=kc.up, fov_y=kc.fov_y, scale=c["scale"])
    W, H = LOCAL_W, LOCAL_H
    nz, ny, nx = volume("clean20").shape
    R = Wt.frame_rays(W, H)
    front, back = Wt.analytic_endpoints(W, H, R["x"], R["y"], cam.origin, cam.look(), cam.up, cam.fov_y, cam.scale)
    step = f32(1) / np.array([nx, ny, nz], f32)
    Wt.setup(R, front, back, cam.origin, step, N, (*PLANE["point"], *PLANE["normal"]))
    o, d, sd = (R[key].astype(np.float64) for key in ("origin", "dir", "sdir"))
    sstep, upper = R["sstep"].astype(np.float64), R["upper"].astype(np.float64)
    inv_scale = 1.0 / np.asarray(c["scale"], np.float64)
    planted = [(PLANT_X + dx, PLANT_Y + dy, PLANT_Z) for dx in (0, 1) for dy in (0, 1)]
    n = len(R["x"])
    with np.errstate(all="ignore"):
        meets = ~R["dead"] & (0.0 < upper) & np.isfinite(d).all(axis=1)
        safe = np.ones(n, bool)
        dist = np.zeros(n)
        while (meets & (dist < upper)).any():
            run = meets & (dist < upper)
            for i in range(32):
                pos = o + d * dist[:, None] + sd * i
                vox = ((pos - 0.5) * inv_scale + 0.5) * np.array([nx, ny, nz], np.float64) - 0.5
                for pv in planted:
                    near = (np.abs(vox - np.array(pv, np.float64)) <= 2.0).all(axis=1)
                    safe &= ~(run & near)
            dist = dist + sstep * 30.0
    if phong:                                                   # the four neighbour rays of the same slab's footprint, held to the same rule
        base = np.arange(n) - (R["sy"] * R["fw"] + R["sx"])
        all_safe = safe.copy()
        for dx, dy in ((-1, 0), (1, 0), (0, 1), (0, -1)):
            sx = np.clip(R["sx"] + dx, 0, R["fw"] - 1); sy = np.clip(R["sy"] + dy, 0, R["fh"] - 1)
            all_safe &= safe[base + sy * R["fw"] + sx]
        safe = all_safe
    own = R["owned"]
    kept = np.zeros((H, W), bool); met = np.zeros((H, W), bool)
    met[R["y"][own], R["x"][own]] = meets[own]
    kept[R["y"][own], R["x"][own]] = meets[own] & safe[own]
    return kept, met


@functools.lru_cache(maxsize=None)
def clean_frame(k, phong=False, mip=False):
    c = LOCAL[k]; kc = CAMS[c["cam"]]
    out = Wt.render(volume("clean20"), table("random"), LOCAL_W, LOCAL_H, cam_origin=kc.origin, look=vv.Camera(origin=kc.origin, look_at=kc.look_at).look(),
                    up=kc.up, fov_y=kc.fov_y, scale=c["scale"], phong=phong, filt=c["filt"], fill=FILL, mip=mip)
    for a in out[:-1]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("phong", [False, True])
@pytest.mark.parametrize("k", range(len(LOCAL)))
def test_planted_block_leaves_enough_pixels(k, phong):
    """Precondition of the GPU tests below, from the witness alone: the block is two voxels or more from every face, the kept pixels are at least 30 % of
    the pixels whose rays meet the volume, some pixels are NOT kept (the block is in view), and the clean frame is not flat on the kept ones."""
    nz, ny, nx = volume("clean20").shape
    assert 2 <= PLANT_X and PLANT_X + 1 <= nx - 3 and 2 <= PLANT_Y and PLANT_Y + 1 <= ny - 3 and 2 <= PLANT_Z <= nz - 3
    for name in ("planted20a", "planted20b"):
        bad = ~np.isfinite(volume(name)) | (np.abs(volume(name)) > f32(2.0 ** 126))
        assert bad.sum() == 4 and bad[PLANT_Z, PLANT_Y:PLANT_Y + 2, PLANT_X:PLANT_X + 2].all()
        assert np.array_equal(volume(name)[~bad], volume("clean20")[~bad])
    kept, met = far_pixels(k, phong)
    assert met.sum() >= 100
    assert kept.sum() >= 0.3 * met.sum(), (int(kept.sum()), int(met.sum()))
    assert (met & ~kept).sum() >= 10
    assert len(np.unique(clean_frame(k, phong=phong)[0][kept], axis=0)) >= 20


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
@pytest.mark.parametrize("i", MIP + MIP_ENDS, ids=[IDS[i] for i in MIP + MIP_ENDS])
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


def local_camera(k):
    c = LOCAL[k]; kc = CAMS[c["cam"]]
    return vv.Camera(origin=kc.origin, look_at=kc.look_at, up=kc.up, fov_y=kc.fov_y, scale=c["scale"])


def written_everywhere(frame, met, what):
    assert not (frame[met] == FILL).all(axis=-1).any(), f"{what}: a pixel whose ray meets the volume was not written"


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("k", range(len(LOCAL)))
def test_out_of_domain_voxels_stay_local(ctx, monkeypatch, knobs_restored, k, variant, build):
    """+-Inf, NaN and +-3e38 planted in a 2 x 2 x 1 block: every pixel that cannot see the block (far_pixels) is byte for byte the clean volume's, unshaded
    and MIP, on every layout build; the clean frame is the witness's.  The other pixels are written, nothing more is asked of them."""
    cam = local_camera(k); kept, met = far_pixels(k, False)
    kw = dict(options=vv.make_options(filter=LOCAL[k]["filt"]))
    forced(ctx, monkeypatch, build)
    frames = {}
    for name in ("clean20", "planted20" + variant):
        ctx.load_volume(volume(name), table("random"))
        rgba = ctx.render(LOCAL_W, LOCAL_H, cam, fill=FILL, **kw)
        mip_rgba, mip_idx = ctx.render_mip(LOCAL_W, LOCAL_H, cam, fill=FILL, return_index=True, **kw)
        frames[name] = (rgba, mip_rgba, mip_idx)
    clean, planted = frames["clean20"], frames["planted20" + variant]
    same(clean[0], clean_frame(k)[0], f"clean [{build}]")
    same(clean[2], clean_frame(k, mip=True)[1], f"clean [{build}]: index image")
    for a, b, what in zip(planted, clean, ("rgba", "MIP rgba", "MIP index")):
        same(a[kept], b[kept], f"{what} [{build}] on the pixels that cannot see the block")
    written_everywhere(planted[0], met, f"rgba [{build}]"); written_everywhere(planted[1], met, f"MIP rgba [{build}]")


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["default", "bricked", "big"])
@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("k", range(len(LOCAL)))
def test_out_of_domain_voxels_stay_local_phong(ctx, monkeypatch, knobs_restored, k, variant, build):
    """The same with Phong shading: a pixel is held to equality when neither its own ray nor one of its four neighbour rays can see the block."""
    cam = local_camera(k); kept, met = far_pixels(k, True)
    kw = dict(options=vv.make_options(filter=LOCAL[k]["filt"]))
    forced(ctx, monkeypatch, build)
    frames = {}
    for name in ("clean20", "planted20" + variant):
        ctx.load_volume(volume(name), table("random"))
        frames[name] = ctx.render(LOCAL_W, LOCAL_H, cam, fill=FILL, phong=True, **kw)
    same(frames["clean20"], clean_frame(k, phong=True)[0], f"clean [{build}]")
    same(frames["planted20" + variant][kept], frames["clean20"][kept], f"Phong [{build}] on the pixels that cannot see the block")
    written_everywhere(frames["planted20" + variant], met, f"Phong [{build}]")
