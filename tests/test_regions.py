"""Region measurements (vv_region_table) against tests/region_model.py, every word exactly.

CPU part: the library and the binding export the call, the structures have the header's sizes and offsets, the model equals scipy.ndimage on the
compact labels, its faces equal a brute-force loop, and the identities of the header's rule 6 hold.  GPU part: compact, table and summary equal the
model on every shape, label source, box, max_regions and aux of the issue, into guarded device buffers prefilled with 0xA5 whose starts move from call
to call, and through the host path; whatever the block order (VV_REGION_BLOCKS), the chunk cap (VV_REGION_CHUNKS), the layout, the pitch and the
load path; every error of rule 8 is refused in order; and the call leaves the context alone.  The labels come from tests/label_model.py or are built
here, so a case does not depend on vv_label_volume unless it says so.

Not tested: the 2^32 - 2 voxel limit and the 64-bit sums near overflow (no volume with 2^32 voxels or a 2^14 axis is loaded here: the largest sum2 of
this file is below 2^40), and the overlap refusals that need the address of the context's volume (no public call tells it)."""
import ctypes as C
import functools

import numpy as np
import pytest

import hist_model as HM
import label_model as LM
import region_model as RM
import test_hist as TH
import test_label as TL
import volume_out as VO
import volviz_amd as vv
from volume_out import GARBAGE, GUARD

f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2
TF = TH.TF
CHUNK = 1024                                               # kRegionMinChunk of csrc/vv_kernels.h: the shortest chunk a wave walks
FG = TL.FG
LAYOUT_KNOBS = TH.LAYOUT_KNOBS + ("VV_REGION_CHUNKS",)     # (VV_REGION_BLOCKS is left to whoever runs the suite: every test must pass under 1, 8 and unset)
ROW = 184


def _freeze(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name == "built:board":                                  # a 3-D checkerboard: every foreground voxel is its own component under 6
        z, y, x = np.indices((20, 40, 70))
        return _freeze(np.where((x + y + z) % 2 == 0, FG, 0).astype(np.uint8))
    if name.startswith("row:"):                                # one row of random bytes
        nx = int(name[4:])
        return _freeze(np.random.default_rng(nx).integers(0, 256, (1, 1, nx), dtype=np.uint8))
    if name == "specials":                                     # 12 x 10 x 8 f32 with every special value; the cell x < 4, y < 5 is all NaN
        rng = np.random.default_rng(31)
        v = rng.uniform(-0.2, 1.2, (8, 10, 12)).astype(f32)
        sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 0.00392156, 0.00392157, 0.99999994, 1.0], f32)
        flat = v.ravel()
        flat[rng.choice(flat.size, 5 * len(sp), replace=False)] = np.tile(sp, 5)
        v[:, :5, :4] = np.nan
        v[0, 0, 0] = np.array([0xFFC00001], np.uint32).view(f32)[0]        # a NaN of another pattern
        return _freeze(v)
    return TL._volume(name)


def _partition_labels(cell):
    """Canonical labels of a partition: `cell` gives every voxel its set (any integers, 0 = background); the label is 1 + the set's least index."""
    flat = np.asarray(cell).ravel()
    least = {}
    for i, c in enumerate(flat):
        if c and c not in least:
            least[c] = i + 1
    return np.array([least.get(c, 0) for c in flat], np.uint32).reshape(np.shape(cell))


def _run_labels(fg):
    """Canonical labels of the runs of a row's foreground (its components under any connectivity)."""
    fg = np.asarray(fg, bool).ravel()
    start = fg & ~np.concatenate(([False], fg[:-1]))
    first = np.maximum.accumulate(np.where(start, np.arange(fg.size), 0))
    return np.where(fg, first + 1, 0).astype(np.uint32).reshape(1, 1, -1)


def _summary_tuple(s):
    return (int(s.regions), int(s.written), int(s.foreground), int(s.stray))


def _check_rows(got, want, what):
    assert got.dtype == vv.REGION_DTYPE and len(got) == len(want), (what, len(got), len(want))
    bad = RM.same_rows(got, want)
    if len(bad):
        k = int(bad[0])
        fields = [n for n in RM.DTYPE.names if np.asarray(got[n][k]).tobytes() != np.asarray(want[n][k]).tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} rows differ, first row {k} in {fields}: {got[k]} vs {want[k]}")


def _check_volume(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    VO.report(got, want, np.argwhere(got != want), what)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_region_call():
    lib = vv.load_library()
    assert "vv_region_table" in vv.EXPORTS and "vv_region_table" in vv._NEWER_EXPORTS and hasattr(lib, "vv_region_table"), "vv_region_table is not exported"
    for name in ("regions", "regions_device", "measure"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert callable(vv.region_properties)
    assert (vv.REGION_LABELS, vv.REGION_NONZERO) == (0, 1) == (RM.LABELS, RM.NONZERO)
    assert (C.sizeof(vv.vv_regions), C.sizeof(vv.vv_region), C.sizeof(vv.vv_region_summary), C.alignment(vv.vv_region)) == (32, ROW, 32, 8)
    d, s = vv.vv_regions, vv.vv_region_summary
    assert (d.box_lo.offset, d.box_hi.offset, d.source.offset, d.max_regions.offset) == (0, 12, 24, 28)
    assert (s.regions.offset, s.written.offset, s.foreground.offset, s.stray.offset) == (0, 8, 16, 24)
    want = dict(label=0, reserved=4, voxels=8, lo=16, hi=28, sum=40, sum2=64, bin_min=112, bin_max=116, bin_sum=120, bin_sum2=128, vmin=136, vmax=140,
                faces=144, aux_sum=168, aux_argmax=176, aux_max=180)
    assert {n: getattr(vv.vv_region, n).offset for n in want} == want
    assert vv.REGION_DTYPE.itemsize == RM.DTYPE.itemsize == ROW and vv.REGION_DTYPE.names == RM.DTYPE.names
    for n in want:
        assert vv.REGION_DTYPE.fields[n][1] == RM.DTYPE.fields[n][1] == want[n] and vv.REGION_DTYPE.fields[n][0] == RM.DTYPE.fields[n][0], n
    assert want["aux_argmax"] % 8 == 0 and want["aux_max"] == want["aux_argmax"] + 4           # one 8-byte slot, the maximum in its high word


CPU_CASES = [("r70_u8", (0, 78), 6, None), ("r70_u8", (0, 24), 26, ((3, 5, 1), (61, 33, 17))), ("r70_f32", (0, 34), 18, None), ("aniso", (60, 100), 6, None),
             ("built:comb", (FG, FG), 6, ((0, 0, 0), (69, 40, 20))), ("special_f32", (0, 0), 26, None)]


@pytest.mark.parametrize("volname,bins,conn,box", CPU_CASES)
def test_model_equals_scipy(volname, bins, conn, box):
    ndimage = pytest.importorskip("scipy.ndimage")
    vol = _volume(volname)
    labels = TL._want(volname, bins, conn, box)[0]
    rng = np.random.default_rng(5)
    aux = rng.integers(0, 50, labels.shape).astype(np.uint32)
    t, compact, s = RM.region_table(vol, labels, aux, box=box)
    K = s.regions
    assert K == len(t) == int(compact.max()) and s.stray == 0 and K > 0
    index = np.arange(1, K + 1)
    sub = HM.crop(vol, box)
    lo = (0, 0, 0) if box is None else box[0]
    # the compact labels are the canonical ones ranked
    assert np.array_equal(np.unique(labels[labels > 0]), t["label"]) and np.array_equal(t["label"][compact[labels > 0].astype(np.int64) - 1], labels[labels > 0])
    ones = np.ones(labels.shape, np.int64)
    assert np.array_equal(t["voxels"], np.asarray(ndimage.sum_labels(ones, compact, index), np.int64))
    z, y, x = np.indices(labels.shape)
    for a, c in enumerate((x + lo[0], y + lo[1], z + lo[2])):
        assert np.array_equal(t["sum"][:, a], np.asarray(ndimage.sum_labels(c.astype(np.float64), compact, index)).astype(np.uint64))
        assert np.array_equal(t["lo"][:, a], np.asarray(ndimage.minimum(c, compact, index)).astype(np.int32))
        assert np.array_equal(t["hi"][:, a], np.asarray(ndimage.maximum(c, compact, index)).astype(np.int32) + 1)
    for k, sl in enumerate(ndimage.find_objects(compact.astype(np.int32))):
        assert tuple(t["lo"][k]) == tuple(sl[2 - a].start + lo[a] for a in range(3)) and tuple(t["hi"][k]) == tuple(sl[2 - a].stop + lo[a] for a in range(3))
    com = np.asarray(ndimage.center_of_mass(ones, compact, index))[:, ::-1] + np.asarray(lo)
    assert np.allclose(t["sum"] / t["voxels"][:, None].astype(np.float64), com, rtol=1e-12, atol=0)
    bins_arr = HM.bins(sub).astype(np.float64)
    assert np.array_equal(t["bin_sum"], np.asarray(ndimage.sum_labels(bins_arr, compact, index)).astype(np.uint64))
    assert np.array_equal(t["bin_min"], np.asarray(ndimage.minimum(bins_arr, compact, index)).astype(np.uint32))
    assert np.array_equal(t["bin_max"], np.asarray(ndimage.maximum(bins_arr, compact, index)).astype(np.uint32))
    assert np.array_equal(t["aux_sum"], np.asarray(ndimage.sum_labels(aux.astype(np.float64), compact, index)).astype(np.uint64))
    assert np.array_equal(t["aux_max"], np.asarray(ndimage.maximum(aux, compact, index)).astype(np.uint32))
    assert np.array_equal(aux.ravel()[t["aux_argmax"]], t["aux_max"]) and np.array_equal(compact.ravel()[t["aux_argmax"]], index)
    for k in range(0, K, max(K // 40, 1)):                          # the least index among the maxima
        assert t["aux_argmax"][k] == np.flatnonzero((compact.ravel() == k + 1) & (aux.ravel() == t["aux_max"][k]))[0], k
    if sub.dtype == np.uint8:
        assert np.array_equal(t["vmin"], t["bin_min"].astype(f32)) and np.array_equal(t["vmax"], t["bin_max"].astype(f32))
    else:
        for k in range(0, K, max(K // 40, 1)):
            v = sub[compact == k + 1]
            got = (t["vmin"][k:k + 1].view(np.uint32)[0], t["vmax"][k:k + 1].view(np.uint32)[0])
            assert got == tuple(int(np.asarray(w, f32).view(np.uint32)) for w in HM.value_range(v)), k


def test_model_faces_equal_a_brute_force_loop():
    rng = np.random.default_rng(9)
    cell = rng.integers(0, 4, (4, 5, 6))
    labels = _partition_labels(cell)
    vol = rng.integers(0, 256, cell.shape, dtype=np.uint8)
    for source in (RM.LABELS, RM.NONZERO):
        t, compact, s = RM.region_table(vol, labels, source=source)
        want = np.zeros((len(t), 3), np.uint64)
        nz, ny, nx = cell.shape
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    me = compact[z, y, x]
                    if not me:
                        continue
                    for a, (dx, dy, dz) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                        for sgn in (1, -1):
                            X, Y, Z = x + sgn * dx, y + sgn * dy, z + sgn * dz
                            inside = 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz
                            if not inside or compact[Z, Y, X] != me:
                                want[me - 1, a] += 1
        assert np.array_equal(t["faces"], want), source
        assert s.regions == (3 if source == RM.LABELS else 1)


def test_model_identities():
    # rule 6 on the model's own labels: voxels are the sizes, regions the components, the rows sum to foreground - stray
    for conn, bins in TL.PERCOLATION:
        labels, sizes, stats = TL._want("r70_u8", bins, conn)
        t, compact, s = RM.region_table(_volume("r70_u8"), labels)
        assert np.array_equal(t["voxels"], sizes.ravel()[t["label"].astype(np.int64) - 1]) and s.regions == stats.components == len(t)
        assert int(t["voxels"].sum()) == s.foreground - s.stray == stats.foreground and s.stray == 0
        assert (np.diff(t["label"].astype(np.int64)) > 0).all() and np.array_equal(compact != 0, labels != 0)
        short = RM.region_table(_volume("r70_u8"), labels, max_regions=7)
        assert len(short[0]) == 7 == short[2].written and short[0].tobytes() == t[:7].tobytes() and np.array_equal(short[1], compact)
    # a solid a x b x c block: faces (2bc, 2ac, 2ab), whatever surrounds it
    vol = np.zeros((9, 8, 11), np.uint8)
    a, b, c = 5, 3, 4
    vol[2:2 + c, 1:1 + b, 3:3 + a] = 9
    for fill in (0, 1):
        cell = np.where(vol > 0, 2, fill)
        t, _, s = RM.region_table(vol, _partition_labels(cell))
        row = t[-1] if fill else t[0]
        assert tuple(row["faces"]) == (2 * b * c, 2 * a * c, 2 * a * b) and row["voxels"] == a * b * c and s.regions == 1 + fill
        assert tuple(row["lo"]) == (3, 1, 2) and tuple(row["hi"]) == (3 + a, 1 + b, 2 + c)
    # the whole box as one region: only the box's sides count
    t, _, _ = RM.region_table(vol, np.ones(vol.shape, np.uint32))
    assert tuple(t[0]["faces"]) == (2 * 8 * 9, 2 * 11 * 9, 2 * 11 * 8) and t[0]["label"] == 1
    # strays: labels at or above the voxel count, labels that point at background, at a non-root, above their own index
    n = vol.size
    lab = np.zeros(n, np.uint32)
    lab[5] = 6                                                    # a root
    lab[9] = 6                                                    # owned
    lab[2] = 6                                                    # owned, above its own index
    lab[7] = 10                                                   # points at a non-root (voxel 9)
    lab[8] = 1                                                    # points at background (voxel 0)
    lab[11], lab[12], lab[13] = n, n + 1, 0xFFFFFFFF              # voxel n - 1 is background; beyond the box
    t, compact, s = RM.region_table(vol, lab.reshape(vol.shape))
    assert _summary_tuple(s) == (1, 1, 8, 5) and t[0]["voxels"] == 3 and t[0]["label"] == 6
    assert np.array_equal(np.flatnonzero(compact.ravel()), [2, 5, 9])
    # NONZERO: one region whatever the words are
    t, compact, s = RM.region_table(vol, lab.reshape(vol.shape), source=RM.NONZERO)
    assert _summary_tuple(s) == (1, 1, 8, 0) and t[0]["label"] == 3 and t[0]["voxels"] == 8 and (compact.ravel()[lab != 0] == 1).all()
    t, compact, s = RM.region_table(vol, np.zeros(vol.shape, np.uint32), source=RM.NONZERO)
    assert _summary_tuple(s) == (0, 0, 0, 0) and len(t) == 0 and not compact.any()


def test_region_properties_agree_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    vol = _volume("r70_u8")
    labels = TL._want("r70_u8", (0, 78), 6)[0]
    aux = np.random.default_rng(3).integers(0, 400, labels.shape).astype(np.uint32)
    t, compact, s = RM.region_table(vol, labels, aux)
    spacing = (0.5, 1.25, 2.0)
    p = vv.region_properties(t.astype(vv.REGION_DTYPE), spacing)
    index = np.arange(1, s.regions + 1)
    ones = np.ones(labels.shape)
    com = np.asarray(ndimage.center_of_mass(ones, compact, index))[:, ::-1] * np.asarray(spacing)
    assert np.allclose(p["centroid"], com, rtol=1e-12, atol=1e-12)
    assert np.array_equal(p["voxels"], np.asarray(ndimage.sum_labels(ones, compact, index)).astype(np.uint64))
    assert np.allclose(p["mean_bin"], ndimage.mean(vol.astype(np.float64), compact, index), rtol=1e-12)
    assert np.allclose(p["inscribed_radius"], np.sqrt(np.asarray(ndimage.maximum(aux, compact, index), np.float64)), rtol=1e-15)
    faces = RM.face_counts(np.where(compact > 0, compact.astype(np.int64), -1))
    area = sum(np.asarray(ndimage.sum_labels(faces[a].astype(np.float64), compact, index)) * np.prod([spacing[b] for b in range(3) if b != a]) for a in range(3))
    assert np.allclose(p["surface_area"], area, rtol=1e-12)
    big = int(np.argmax(t["voxels"]))
    z, y, x = np.nonzero(compact == big + 1)
    pts = np.stack([x * spacing[0], y * spacing[1], z * spacing[2]])
    assert np.allclose(p["covariance"][big], np.cov(pts, bias=True), rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _load(ctx, monkeypatch, vol):
    VO.load(ctx, monkeypatch, LAYOUT_KNOBS, _volume(vol) if isinstance(vol, str) else vol, TF)


class RegionOut(VO.GuardedOuts):
    """The guarded device buffer of a region call: compact at a start that moves by 4 bytes from call to call, table and summary by 8 (every call;
    every second call); the rows that are not written must survive like the guards."""

    def __init__(self, voxels, rows):
        super().__init__(4 * voxels + ROW * rows + 32 + 4 * GUARD + 64, 8)
        self.voxels, self.rows = voxels, rows

    def run(self, call, shape, max_regions, written, table=True, summary=True, what=""):
        """call(compact_ptr, capacity, table_ptr, summary_ptr), complete on return -> compact, the written rows, the summary tuple or None"""
        n = int(np.prod(shape)) * 4
        assert n <= 4 * self.voxels and max_regions <= self.rows
        outs = [VO.Out(n), VO.Out(ROW * max_regions, ROW * written, align=8, present=table), VO.Out(32, align=8, digit=2, present=summary)]
        c, t, s = self.run_outs(lambda p: call(p[0], n, p[1], p[2]), outs, what)
        return (c.view(np.uint32).reshape(shape), t.view(vv.REGION_DTYPE) if table else None,
                _summary_tuple(vv.RegionSummary.from_bytes(s)) if summary else None)


def _run_case(ctx, dev, what, vol, labels, aux=None, source=RM.LABELS, box=None, max_regions=None, host=True):
    """One case through the guarded device buffers and, with `host`, through host pointers.  max_regions None: one row per region."""
    want_t, want_c, want_s = RM.region_table(vol, labels, aux, source, box, max_regions)
    rows = want_s.regions if max_regions is None else max_regions
    what = f"{what} source {source} box {box} max_regions {rows}"
    lab_t = dev.upload(labels)
    aux_t = dev.upload(aux) if aux is not None else None
    gc, gt, gs = dev.run(lambda cp, cap, tp, sp: ctx.regions_device(lab_t.data_ptr(), cp, cap, tp if rows else 0, rows, aux_ptr=aux_t.data_ptr() if aux is not None else 0,
                                                                     summary_ptr=sp, source=source, box=box),
                         labels.shape, rows, want_s.written, what=what)
    _check_volume(gc, want_c, what + " compact")
    _check_rows(gt, want_t, what + " table")
    assert gs == _summary_tuple(want_s), (what, gs, want_s)
    if not host:
        return want_t, want_c, want_s
    k = dev.calls % 2
    got = ctx.regions(labels, aux, source, box, rows, return_compact=True, return_summary=bool(k), prefill=GARBAGE if k else 0x11)
    _check_rows(got[0][:want_s.written], want_t, what + " host table")
    assert (got[0][want_s.written:].view(np.uint8) == (GARBAGE if k else 0x11)).all(), what + ": a row beyond `written` was touched"
    _check_volume(got[1], want_c, what + " host compact")
    if k:
        assert _summary_tuple(got[2]) == _summary_tuple(want_s), (what, got[2], want_s)
    return want_t, want_c, want_s


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["1x1x1", "2x1x3", "1x40x1"])
def test_region_small_shapes(ctx, shape, monkeypatch):
    for kind in ("u8", "f32"):
        name = f"{kind}:{shape}"
        _load(ctx, monkeypatch, name)
        vol = _volume(name)
        dev = RegionOut(vol.size, vol.size)
        for conn in (6, 26):
            for bins in ((0, 100), (128, 255), (0, 255), (77, 77)):
                labels = TL._want(name, bins, conn)[0]
                _run_case(ctx, dev, f"{name} bins {bins} conn {conn}", vol, labels, aux=labels)
                _run_case(ctx, dev, f"{name} bins {bins} conn {conn}", vol, labels, source=RM.NONZERO, max_regions=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty", "full", "snake", "comb", "corner", "edge", "board"])
def test_region_built_shapes(ctx, name, monkeypatch):
    """No region; one region that takes every atomic; one-voxel-wide paths through every chunk; teeth; pairs of voxels; and a region per voxel."""
    volname = "built:" + name
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    for conn in ((6,) if name in ("empty", "full", "board") else (6, 26)):
        labels = LM.label(vol, (FG, FG), conn)[0] if name == "board" else TL._want(volname, (FG, FG), conn)[0]
        K = len(np.unique(labels[labels > 0]))
        dev = RegionOut(vol.size, K + 3)
        t, c, s = _run_case(ctx, dev, f"{volname} conn {conn}", vol, labels, aux=(labels % 977).astype(np.uint32))
        if name == "empty":
            assert _summary_tuple(s) == (0, 0, 0, 0)
        if name == "full":
            assert _summary_tuple(s) == (1, 1, vol.size, 0) and tuple(t[0]["faces"]) == (2 * 40 * 20, 2 * 70 * 20, 2 * 70 * 40) and t[0]["voxels"] == vol.size
        if name == "board":
            assert s.regions == vol.size // 2 and (t["voxels"] == 1).all() and (t["faces"] == 2).all()
        if name in ("snake", "comb") and conn == 6:
            assert s.regions == 1
            back = LM.label(vol, (0, 0), 6)
            _run_case(ctx, RegionOut(vol.size, back[2].components), f"{volname} background", vol, back[0], host=False)


def _row_case(nx):
    """A row whose chunk boundaries carry roots: voxels 0, CHUNK - 1, CHUNK, 2 CHUNK - 1 and 2 CHUNK (where they exist) start a run of their own."""
    labels = _run_labels(np.random.default_rng(nx + 1).random(nx) < 0.6)
    flat = labels.ravel()
    for p in (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, nx - 1):
        if p < nx:
            flat[p] = p + 1                                       # (the rest of its run keeps pointing at the run's first voxel, still a root)
    return labels


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, "3"])
def test_region_chunk_boundaries(ctx, chunks, monkeypatch):
    """Single rows of CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 voxels with roots on the first and the last voxel of a chunk; the same with the chunk
    cap lowered to 3, under which the 70 x 40 x 20 noise is three long chunks."""
    try:
        for nx in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
            name = f"row:{nx}"
            _load(ctx, monkeypatch, name)
            if chunks:
                monkeypatch.setenv("VV_REGION_CHUNKS", chunks)
                ctx.reread_env()
            labels = _row_case(nx)
            flat = labels.ravel()
            K = int((flat == np.arange(1, nx + 1)).sum())
            dev = RegionOut(nx, K + 3)
            _run_case(ctx, dev, f"row of {nx}, chunks {chunks}", _volume(name), labels, aux=np.arange(nx, dtype=np.uint32).reshape(labels.shape) % 7)
            _run_case(ctx, dev, f"row of {nx}, chunks {chunks}", _volume(name), labels, max_regions=K + 3, host=False)
            _run_case(ctx, dev, f"row of {nx}, chunks {chunks}", _volume(name), labels, source=RM.NONZERO, max_regions=1)
        _load(ctx, monkeypatch, "r70_u8")
        if chunks:
            monkeypatch.setenv("VV_REGION_CHUNKS", chunks)
            ctx.reread_env()
        labels = TL._want("r70_u8", (0, 78), 6)[0]
        _run_case(ctx, RegionOut(56000, TL._want("r70_u8", (0, 78), 6)[2].components), f"noise, chunks {chunks}", _volume("r70_u8"), labels, aux=labels)
    finally:
        monkeypatch.delenv("VV_REGION_CHUNKS", raising=False)
        ctx.reread_env()


@pytest.mark.gpu
@pytest.mark.parametrize("conn,bins", TL.PERCOLATION)
@pytest.mark.parametrize("volname", ["r70_u8", "r70_f32"])
def test_region_noise(ctx, volname, conn, bins, monkeypatch):
    """70 x 40 x 20 random foreground at the percolation thresholds: thousands of regions of every size, one of them through most chunks."""
    _load(ctx, monkeypatch, volname)
    labels, sizes, stats = TL._want(volname, bins, conn)
    aux = np.random.default_rng(conn).integers(0, 1 << 20, labels.shape).astype(np.uint32)
    t, c, s = _run_case(ctx, RegionOut(56000, stats.components), volname, _volume(volname), labels, aux)
    assert s.regions == stats.components and np.array_equal(t["voxels"], sizes.ravel()[t["label"].astype(np.int64) - 1])


@pytest.mark.gpu
def test_region_f32_specials(ctx, monkeypatch):
    """NaN, +-Inf, -0.0 and denormals in vmin / vmax and the bins; one region is all NaN: +Inf / -Inf, bins 0."""
    _load(ctx, monkeypatch, "specials")
    vol = _volume("specials")
    z, y, x = np.indices(vol.shape)
    labels = _partition_labels(1 + x // 4 + 3 * (y // 5))
    dev = RegionOut(vol.size, 9)
    t, c, s = _run_case(ctx, dev, "specials", vol, labels)
    assert s.regions == 6 and t[0]["label"] == 1 and t[0]["voxels"] == 4 * 5 * 8
    assert t[0:1]["vmin"].view(np.uint32)[0] == 0x7F800000 and t[0:1]["vmax"].view(np.uint32)[0] == 0xFF800000 and t[0]["bin_max"] == 0 and t[0]["bin_sum"] == 0
    bits = set(int(b) for b in np.concatenate([t["vmin"].view(np.uint32), t["vmax"].view(np.uint32)]))
    assert 0xFF800000 in bits and 0x7F800000 in bits
    _run_case(ctx, dev, "specials, one region", vol, labels, source=RM.NONZERO, max_regions=1)
    _load(ctx, monkeypatch, "special_f32")
    vol = _volume("special_f32")
    for conn, bins in ((6, (0, 0)), (26, (255, 255)), (18, (1, 254))):
        labels = TL._want("special_f32", bins, conn)[0]
        _run_case(ctx, RegionOut(vol.size, vol.size), f"special_f32 {bins}", vol, labels, aux=labels)


@pytest.mark.gpu
def test_region_boxes(ctx, monkeypatch):
    """Boxes off the origin (the sums and the bounding boxes are in volume coordinates) and a box that cuts a region (its sides count as faces)."""
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    dev = RegionOut(56000, 12000)
    boxes = [((3, 5, 1), (70, 40, 20)), ((17, 9, 9), (18, 10, 10)), ((1, 1, 1), (69, 39, 19)), ((15, 7, 7), (34, 17, 17)), ((5, 0, 3), (6, 40, 4))]
    for k, box in enumerate(boxes):
        conn, bins = TL.PERCOLATION[k % 4]
        labels = TL._want("r70_u8", bins, conn, box)[0]
        t, c, s = _run_case(ctx, dev, "r70_u8", vol, labels, aux=labels, box=box)
        assert (t["lo"] >= np.asarray(box[0])).all() and (t["hi"] <= np.asarray(box[1])).all()
    _load(ctx, monkeypatch, "built:full")
    box = ((10, 4, 2), (60, 30, 18))
    ones = np.ones((16, 26, 50), np.uint32)
    t, c, s = _run_case(ctx, dev, "full, cut by the box", _volume("built:full"), ones, box=box)
    assert tuple(t[0]["faces"]) == (2 * 26 * 16, 2 * 50 * 16, 2 * 50 * 26) and tuple(t[0]["lo"]) == box[0] and tuple(t[0]["hi"]) == box[1]
    assert t[0]["sum"][0] == sum(range(10, 60)) * 26 * 16


def _arbitrary_labels(n, seed):
    """Random words: roots, owned voxels (below and above their root), labels that point at non-roots, at background, beyond the box."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.int64)
    lab = np.zeros(n, np.int64)
    kind = rng.integers(0, 10, n)
    roots = np.flatnonzero(kind == 0)
    lab[roots] = roots + 1
    own = np.flatnonzero((kind >= 1) & (kind <= 4))
    lab[own] = rng.choice(roots, len(own)) + 1                     # owned: half of them above their own index
    anyw = np.flatnonzero(kind == 5)
    lab[anyw] = rng.integers(1, n + 1, len(anyw))                  # anywhere in the box: mostly non-roots and background
    far = np.flatnonzero(kind == 6)
    lab[far] = rng.choice(np.array([n + 1, n + 2, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], np.int64), len(far))
    chain = np.flatnonzero(kind == 7)
    lab[chain] = rng.choice(own, len(chain)) + 1                   # at an owned voxel, which is no root
    assert (lab[own] - 1 > own).any() and (lab[own] - 1 < own).any() and len(idx) == n
    return lab.astype(np.uint32)


@pytest.mark.gpu
def test_region_arbitrary_labels_and_block_order(ctx, monkeypatch):
    """Labels that are arbitrary words: the ownership test is made on `labels` alone, so `stray` and every output equal the model whichever block runs
    first: VV_REGION_BLOCKS = 1, 8 and as the suite was started; and a second run gives the same bytes."""
    _load(ctx, monkeypatch, "r70_f32")
    vol = _volume("r70_f32")
    labels = _arbitrary_labels(vol.size, 12).reshape(vol.shape)
    aux = np.random.default_rng(13).integers(0, 2 ** 32, vol.shape, dtype=np.uint64).astype(np.uint32)
    K = RM.region_table(vol, labels)[2].regions
    dev = RegionOut(vol.size, K)
    try:
        for blocks in ("1", "8", None):
            if blocks is not None:
                monkeypatch.setenv("VV_REGION_BLOCKS", blocks)
            else:
                monkeypatch.undo()
            ctx.reread_env()
            t, c, s = _run_case(ctx, dev, f"VV_REGION_BLOCKS={blocks} arbitrary", vol, labels, aux)
            assert s.stray > 10000 and s.regions > 3000 and int(t["voxels"].sum()) == s.foreground - s.stray
            first = ctx.regions(labels, aux, return_compact=True, prefill=GARBAGE)
            second = ctx.regions(labels, aux, return_compact=True, prefill=0)
            assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes(), "a second run differs"
            _run_case(ctx, dev, f"VV_REGION_BLOCKS={blocks} arbitrary", vol, labels, aux, source=RM.NONZERO, max_regions=1, host=False)
    finally:
        monkeypatch.undo()
        ctx.reread_env()


@pytest.mark.gpu
def test_region_max_regions(ctx, monkeypatch):
    """max_regions 0 with table NULL, 1, K - 1, K and K + 3: compact and the summary do not depend on it, the rows beyond `written` keep the garbage."""
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    labels, sizes, stats = TL._want("r70_u8", (0, 78), 6)
    K = stats.components
    dev = RegionOut(vol.size, K + 3)
    for m in (0, 1, K - 1, K, K + 3):
        t, c, s = _run_case(ctx, dev, "max_regions", vol, labels, aux=labels, max_regions=m)
        assert _summary_tuple(s) == (K, min(K, m), stats.foreground, 0)
    # a table pointer with max_regions 0 is not written either
    lab_t = dev.upload(labels)
    gc, gt, gs = dev.run(lambda cp, cap, tp, sp: ctx.regions_device(lab_t.data_ptr(), cp, cap, tp, 0, summary_ptr=sp), labels.shape, 0, 0, what="max_regions 0, table given")
    assert gs == (K, 0, stats.foreground, 0)


@pytest.mark.gpu
def test_region_aux(ctx, monkeypatch):
    """Ties for the maximum (the least index wins), values near 2^32 - 1, the squared distances of vv_distance_volume, and no aux at all."""
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    labels, sizes, stats = TL._want("r70_u8", (0, 78), 6)
    dev = RegionOut(vol.size, stats.components)
    rng = np.random.default_rng(41)
    ties = rng.integers(0, 3, vol.shape).astype(np.uint32)
    t, c, s = _run_case(ctx, dev, "aux ties", vol, labels, ties)
    big = int(np.argmax(t["voxels"]))
    assert t[big]["aux_max"] == 2 and (ties.ravel()[c.ravel() == big + 1] == 2).sum() > 1
    assert t[big]["aux_argmax"] == np.flatnonzero((c.ravel() == big + 1) & (ties.ravel() == 2))[0]
    high = (np.uint32(0xFFFFFFFF) - rng.integers(0, 3, vol.shape).astype(np.uint32)).astype(np.uint32)
    t, c, s = _run_case(ctx, dev, "aux near 2^32", vol, labels, high)
    assert t[big]["aux_max"] == 0xFFFFFFFF and t[big]["aux_sum"] > (int(t[big]["voxels"]) - 1) * (2 ** 32 - 3) > 2 ** 32
    dist = ctx.distance(labels=labels, invert=True, spacing=(1, 2, 1))
    t, c, s = _run_case(ctx, dev, "aux from vv_distance_volume", vol, labels, dist)
    assert (t["aux_max"] >= 1).all()
    t, c, s = _run_case(ctx, dev, "no aux", vol, labels)
    assert not t["aux_sum"].any() and not t["aux_max"].any() and not t["aux_argmax"].any()


@pytest.mark.gpu
def test_region_nonzero_source(ctx, monkeypatch):
    """A morphology result (0 / 1 words) and an all-zero volume measured as one region."""
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    opened = ctx.morphology(vv.MORPH_OPEN, 1.5, bins=(60, 255))
    assert set(np.unique(opened)) == {0, 1} and opened.any()
    dev = RegionOut(vol.size, 4)
    dist = ctx.distance(labels=opened, invert=True)
    t, c, s = _run_case(ctx, dev, "morphology result", vol, opened, dist, source=RM.NONZERO, max_regions=1)
    assert _summary_tuple(s) == (1, 1, int(opened.sum()), 0) and t[0]["label"] == 1 + np.flatnonzero(opened.ravel())[0] and np.array_equal(c, opened)
    _run_case(ctx, dev, "morphology result, no row", vol, opened, source=RM.NONZERO, max_regions=0)
    _run_case(ctx, dev, "morphology result, spare rows", vol, opened, source=RM.NONZERO, max_regions=4)
    zeros = np.zeros(vol.shape, np.uint32)
    for m in (0, 1):
        t, c, s = _run_case(ctx, dev, "all zero", vol, zeros, source=RM.NONZERO, max_regions=m)
        assert _summary_tuple(s) == (0, 0, 0, 0)
    # under LABELS the same words are one region (voxel 0 is its root if set) or all strays
    _run_case(ctx, dev, "0 / 1 words as labels", vol, opened, max_regions=2)


@pytest.mark.gpu
@VO.layout_sweep
def test_region_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume and the 64-bit addressing build, as test_label.py sweeps them.  The volume holds no zero: bin_min is 0 only if padding is
    read as data."""
    with VO.layout_context(kind, nx, knobs, monkeypatch, LAYOUT_KNOBS, TF) as (c, vol):
        nz, ny, _ = vol.shape
        dev = RegionOut(vol.size, vol.size)
        for conn, bins, box in ((6, (1, 100), None), (18, (200, 255), ((1, 0, 1), (nx - 1, ny, nz - 1))), (26, (0, 40), None)):
            labels = LM.label(vol, bins, conn, box)[0]
            t, _, s = _run_case(c, dev, f"layout {kind} {knobs}", vol, labels, aux=labels, box=box)
            assert s.regions > 0 and (t["bin_min"] > 0).all(), "padding was read as data"
        whole = np.ones(vol.shape, np.uint32)
        t, _, _ = _run_case(c, dev, f"layout {kind} {knobs}, every voxel", vol, whole)
        assert t[0]["bin_min"] == HM.bins(vol).min() > 0 and t[0]["bin_sum"] == int(HM.bins(vol).astype(np.int64).sum())


@pytest.mark.gpu
def test_region_load_paths_and_streams(ctx, monkeypatch):
    """A volume that came from a device buffer and one promoted by the streamed upload; then label, distance and region calls enqueued on one torch
    stream, synchronised by the stream alone."""
    import torch
    tdev = torch.device("cuda", 0)
    vol8 = _volume("u8:37x21x13")
    dev = RegionOut(vol8.size, vol8.size)
    labels = TL._want("u8:37x21x13", (0, 100), 18)[0]
    for what, loaded in VO.load_paths(ctx, monkeypatch, LAYOUT_KNOBS, vol8, TF):
        _run_case(ctx, dev, what, loaded, labels, aux=labels)
    # enqueue only
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    conn, bins = 6, (0, 78)
    want_l, sizes, stats = TL._want("r70_u8", bins, conn)
    n, K = want_l.size, stats.components
    ts = torch.cuda.Stream(device=tdev)
    lab_t, aux_t, com_t = (torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev) for _ in range(3))
    tab_t = torch.full((ROW * (K + 1),), GARBAGE, dtype=torch.uint8, device=tdev)
    sum_t = torch.full((4,), -1, dtype=torch.int64, device=tdev)
    assert tab_t.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    with torch.cuda.stream(ts):
        h = vv.stream_handle(ts)
        ctx.label_device(lab_t.data_ptr(), n * 4, bins, conn, stream=h)
        ctx.distance_device(aux_t.data_ptr(), n * 4, invert=True, labels_ptr=lab_t.data_ptr(), stream=h)
        assert ctx.regions_device(lab_t.data_ptr(), com_t.data_ptr(), n * 4, tab_t.data_ptr(), K + 1, aux_ptr=aux_t.data_ptr(), summary_ptr=sum_t.data_ptr(), stream=h) == (70, 40, 20)
    ts.synchronize()
    _check_volume(lab_t.cpu().numpy().view(np.uint32).reshape(want_l.shape), want_l, "enqueue-only labels")
    aux = aux_t.cpu().numpy().view(np.uint32).reshape(want_l.shape)
    want_t, want_c, want_s = RM.region_table(vol, want_l, aux)
    raw = tab_t.cpu().numpy()
    _check_rows(raw[:ROW * K].view(vv.REGION_DTYPE), want_t, "enqueue-only table")
    assert (raw[ROW * K:] == GARBAGE).all()
    _check_volume(com_t.cpu().numpy().view(np.uint32).reshape(want_l.shape), want_c, "enqueue-only compact")
    assert _summary_tuple(vv.RegionSummary.from_bytes(sum_t.cpu().numpy().tobytes())) == _summary_tuple(want_s) == (K, K, stats.foreground, 0)


@pytest.mark.gpu
def test_measure_composes_label_distance_and_regions(ctx, monkeypatch):
    """ctx.measure equals the three calls made by hand (rule 6 on the library's own labels), and region_properties on its table agrees with scipy."""
    ndimage = pytest.importorskip("scipy.ndimage")
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    for bins, conn, box, spacing in (((60, 100), 6, None, (1, 1, 1)), ((80, 255), 26, ((2, 3, 4), (19, 30, 45)), (1, 2, 3))):
        labels, sizes, stats = ctx.label(bins, conn, box, sizes=True, stats=True)
        _check_volume(labels, LM.label(vol, bins, conn, box)[0], "labels for measure")
        dist = ctx.distance(labels=labels, invert=True, spacing=spacing, box=box)
        by_hand, compact, summary = ctx.regions(labels, dist, box=box, return_compact=True, return_summary=True, prefill=GARBAGE)
        want_t, want_c, want_s = RM.region_table(vol, labels, dist, box=box)
        _check_rows(by_hand, want_t, "regions by hand")
        assert np.array_equal(by_hand["voxels"], sizes.ravel()[by_hand["label"].astype(np.int64) - 1]) and summary.regions == stats.components == len(by_hand)
        assert int(by_hand["voxels"].sum()) == summary.foreground - summary.stray == stats.foreground
        got = ctx.measure(bins, conn, box, spacing, thickness=True)
        _check_rows(got, want_t, f"measure {bins} {conn} {box}")
        thin = ctx.measure(bins, conn, box)
        _check_rows(thin, RM.region_table(vol, labels, box=box)[0], "measure without thickness")
        p = vv.region_properties(got, spacing)
        index = np.arange(1, len(got) + 1)
        lo = (0, 0, 0) if box is None else box[0]
        com = (np.asarray(ndimage.center_of_mass(np.ones(labels.shape), compact, index))[:, ::-1] + np.asarray(lo)) * np.asarray(spacing)
        assert np.allclose(p["centroid"], com, rtol=1e-12, atol=1e-12)
        assert np.allclose(p["inscribed_radius"], np.sqrt(np.asarray(ndimage.maximum(dist, compact, index), np.float64)), rtol=1e-15)
        assert np.allclose(p["volume"], np.asarray(ndimage.sum_labels(np.ones(labels.shape), compact, index)) * np.prod(spacing), rtol=1e-15)


@pytest.mark.gpu
def test_region_errors_and_state(ctx, monkeypatch):
    import torch
    tdev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h

    def mk(lo=(0, 0, 0), hi=(0, 0, 0), source=0, max_regions=4):
        d = vv.vv_regions()
        d.box_lo[:], d.box_hi[:] = lo, hi
        d.source, d.max_regions = source, max_regions
        return d

    with vv.Context(0) as empty:                                    # before a load: behind the NULL checks, before a bad descriptor
        out = np.full(1024, GARBAGE, np.uint8)
        p = out.ctypes.data
        assert lib.vv_region_table(empty.h, C.byref(mk(source=9)), p, None, p + 256, 256, p + 512, 256, None, 0, None) == ERR_NO_VOLUME
        assert lib.vv_region_table(empty.h, None, p, None, p + 256, 256, p + 512, 256, None, 0, None) == ERR_INVALID
        assert (out == GARBAGE).all()
        with pytest.raises(vv.VolvizError) as e:
            empty.regions(np.ones((1, 1, 1), np.uint32), box=((0, 0, 0), (1, 1, 1)))
        assert e.value.code == ERR_NO_VOLUME
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    nz, ny, nx = vol.shape
    n = vol.size
    before = VO.Untouched(ctx)

    # one buffer each on the host and on the device: labels | aux | compact | table (8 rows) | summary, GUARD apart
    L0, A0, C0 = 0, n * 4 + GUARD, 2 * (n * 4 + GUARD)
    T0 = 3 * (n * 4 + GUARD)
    S0 = T0 + 8 * ROW + GUARD
    total = S0 + 32 + GUARD
    assert T0 % 8 == 0 and S0 % 8 == 0
    host = np.full(total, GARBAGE, np.uint8)
    raw = torch.full((total,), GARBAGE, dtype=torch.uint8, device=tdev)
    torch.cuda.synchronize()
    hp, dp = host.ctypes.data, raw.data_ptr()
    assert dp % 8 == 0 and hp % 8 == 0

    def call(p, dev, d, labels=L0, aux=A0, compact=C0, ccap=None, table=T0, tcap=8 * ROW, summary=S0):
        f = lambda off: None if off is None else p + off
        return lib.vv_region_table(hnd, C.byref(d) if d is not None else None, f(labels), f(aux), f(compact), n * 4 if ccap is None else ccap, f(table), tcap, f(summary), dev, None)

    def both(d, **kw):
        rc = [call(p, dev, d, **kw) for p, dev in ((hp, 0), (dp, 1))]
        assert rc[0] == rc[1], rc
        return rc[0]

    def said(word):
        return word in lib.vv_last_error(hnd).decode()

    good = mk()
    # NULL checks
    assert lib.vv_region_table(None, C.byref(good), hp, None, hp + C0, n * 4, hp + T0, 8 * ROW, None, 0, None) == ERR_INVALID
    assert both(None) == ERR_INVALID and both(good, labels=None) == ERR_INVALID and both(good, compact=None) == ERR_INVALID
    # the box
    bad_boxes = (((-1, 0, 0), (nx, ny, nz)), ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny, nz + 1)), ((3, 0, 0), (3, ny, nz)), ((0, 5, 0), (nx, 4, nz)), ((1, 0, 0), (0, 0, 0)))
    for lo, hi in bad_boxes:
        assert both(mk(lo, hi)) == ERR_INVALID and said("box"), (lo, hi)
    for source in (-1, 2, 7):
        assert both(mk(source=source)) == ERR_INVALID and said("source")
    assert both(good, table=None) == ERR_INVALID and said("table is NULL")
    # the order: the box before the source before the table before the capacities (compact, then table) before the alignment before the overlaps
    steps = ((dict(), dict(), "box"), (dict(lo=(0, 0, 0)), dict(), "source"), (dict(lo=(0, 0, 0), source=1), dict(), "table is NULL"),
             (dict(lo=(0, 0, 0), source=1), dict(table=T0), "compact capacity"), (dict(lo=(0, 0, 0), source=1), dict(table=T0, ccap=n * 4), "table capacity"),
             (dict(lo=(0, 0, 0), source=1), dict(table=T0, ccap=n * 4, tcap=8 * ROW), "aligned"),
             (dict(lo=(0, 0, 0), source=1), dict(table=T0, ccap=n * 4, tcap=8 * ROW, labels=L0), "overlaps"))
    for fix, args, word in steps:
        kw = dict(lo=(1, 0, 0), hi=(0, 0, 0), source=5, max_regions=8)
        kw.update(fix)
        a = dict(labels=L0 + 2, compact=L0 + 8, table=None, ccap=n * 4 - 1, tcap=8 * ROW - 1)
        a.update(args)
        assert call(dp, 1, mk(**kw), **a) == ERR_INVALID and said(word), (word, lib.vv_last_error(hnd))
    # capacities on both paths: one byte short, 184 * max_regions formed in 64 bits
    assert both(good, ccap=n * 4 - 1) == ERR_INVALID and said("compact capacity")
    assert both(mk(max_regions=8), tcap=8 * ROW - 1) == ERR_INVALID and said("table capacity")
    assert both(mk(max_regions=0xFFFFFFFF), tcap=(ROW * 0xFFFFFFFF) % (1 << 32)) == ERR_INVALID and said("table capacity")
    # alignment (device only)
    for off in (1, 2, 3):
        assert call(dp, 1, good, labels=L0 + off) == ERR_INVALID and said("aligned")
        assert call(dp, 1, good, aux=A0 + off) == ERR_INVALID and said("aligned")
        assert call(dp, 1, good, compact=C0 + off, ccap=n * 4 + GUARD) == ERR_INVALID and said("aligned")
    for off in (1, 4, 7):
        assert call(dp, 1, good, table=T0 + off) == ERR_INVALID and said("aligned")
        assert call(dp, 1, good, summary=S0 + off) == ERR_INVALID and said("aligned")
    # overlaps (device only): compact with labels, aux and table; table with labels and aux
    for coff in (L0, L0 + n * 4 - 4, A0 + 4, A0 - 4):
        assert call(dp, 1, good, compact=coff) == ERR_INVALID and said("compact overlaps"), coff
    assert call(dp, 1, good, compact=T0 - n * 4 + 8, labels=L0, aux=None) == ERR_INVALID and said("compact overlaps")
    assert call(dp, 1, good, table=L0 + 16) == ERR_INVALID and said("table overlaps")
    assert call(dp, 1, good, table=A0 + 8) == ERR_INVALID and said("table overlaps")
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # exactly the needed capacities are enough, on both paths
    labels = TL._want("aniso", (60, 100), 18)[0]
    aux = (labels % 1013).astype(np.uint32)
    want_t, want_c, want_s = RM.region_table(vol, labels, aux, max_regions=8)
    host[L0:L0 + n * 4] = labels.view(np.uint8).ravel()
    host[A0:A0 + n * 4] = aux.view(np.uint8).ravel()
    raw.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    assert both(mk(max_regions=8)) == 0
    for name, got in (("host", host), ("device", raw.cpu().numpy())):
        _check_volume(got[C0:C0 + n * 4].view(np.uint32).reshape(labels.shape), want_c, name + " compact, exact capacity")
        _check_rows(got[T0:T0 + want_s.written * ROW].view(vv.REGION_DTYPE), want_t, name + " table, exact capacity")
        assert _summary_tuple(vv.RegionSummary.from_bytes(got[S0:S0 + 32])) == _summary_tuple(want_s)
        keep = np.ones(total, bool)
        for o, m in ((L0, n * 4), (A0, n * 4), (C0, n * 4), (T0, 8 * ROW), (S0, 32)):
            keep[o:o + m] = False
        assert (got[keep] == GARBAGE).all(), name
    # a device call allocates no device memory: the device's free bytes stay what they were
    def calls():
        for source in (0, 1):
            assert call(dp, 1, mk(source=source, max_regions=8)) == 0

    VO.free_memory_unchanged(calls)
    # the context is still usable and untouched: volume, layout copies, residency, scratch, frame time, histogram, frames
    before.check()
