"""Segmentation (vv_label_volume / vv_mask_volume) against tests/label_model.py, every word and voxel exactly.

CPU part: the library and the binding export the calls, the structures have the header's sizes, the model equals scipy.ndimage.label relabelled by
each component's least index, and the model's own identities hold.  GPU part: labels, sizes and stats equal the model on every shape, volume,
bin range, connectivity and box of the issue, into a guarded device buffer prefilled with 0xA5 whose start moves by 4 bytes from call to call, and
through the host path; whatever the block order (VV_LABEL_BLOCKS), the layout, the pitch and the load path; the mask equals the model for every keep
mode, inversion, type pair and fill; every error of both rule lists is refused in order; and the calls leave the context alone.

Not tested: the refusals that need the address of the context's volume (no public call tells it) and the 2^32 - 2 voxel limit (no volume that large
is loaded here).  VV_KEEP_MIN_SIZE is never fed labels above the voxel count: its bound check is held by reading mask_kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

import derive_model as DM
import hist_model as HM
import label_model as LM
import test_hist as TH
import volume_out as VO
import volviz_amd as vv
from volume_out import GARBAGE, GUARD

f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2
TF = TH.TF
TILE = (16, 8, 8)                                          # label_local_kernel's tile in (x, y, z): kLbTX, kLbTY, kLbTZ of csrc/vv_label.hip
CONNS = LM.CONNECTIVITIES
LAYOUT_KNOBS = TH.LAYOUT_KNOBS + ("VV_DERIVE_BLOCKS", "VV_LABEL_BLOCKS")
FG = 200                                                   # the built shapes: foreground byte on a background of 0
# random foreground near the percolation thresholds of the three neighbourhoods (a uniform byte below k has probability k / 256), and 0.6 under 6
PERCOLATION = ((6, (0, 78)), (18, (0, 34)), (26, (0, 24)), (6, (0, 153)))
SHAPES = ("1x1x1", "2x1x3", "1x40x1") + tuple("x".join(str(t + d) for t in TILE) for d in (0, 1, -1)) + ("37x21x13",)


def _built(name):
    """The built shapes, u8, as [nz, ny, nx]."""
    tx, ty, tz = TILE
    if name == "serpentine":                                   # one tile: a path that visits every second row of every second slice
        v = np.zeros((tz, ty, tx), np.uint8)
        for z in range(0, tz, 2):
            for y in range(0, ty, 2):
                v[z, y, :] = FG
                if y + 2 < ty:
                    v[z, y + 1, tx - 1 if (y // 2) % 2 == 0 else 0] = FG
            if z + 2 < tz:
                v[z + 1, ty - 2, tx - 1 if ((ty - 2) // 2) % 2 == 0 else 0] = FG
        return v
    v = np.zeros((20, 40, 70), np.uint8)
    if name == "snake":                                        # one voxel wide, through every tile of the volume: rows joined at alternating ends, slices at one row
        for z in range(0, 20, 2):
            rows = list(range(0, 40, 2))
            if (z // 2) % 2:
                rows.reverse()
            for k, y in enumerate(rows):
                v[z, y, :] = FG
                if k + 1 < len(rows):
                    v[z, (y + rows[k + 1]) // 2, 69 if k % 2 == 0 else 0] = FG
            if z + 2 < 20:
                v[z + 1, rows[-1], 69 if len(rows) % 2 == 1 else 0] = FG
    elif name == "comb":                                       # teeth along x in every second row and slice, joined only by a spine in the last tile
        v[::2, ::2, :] = FG
        v[:, :, 69] = FG
    elif name == "corner":                                     # two voxels that touch only across a tile corner
        v[tz - 1, ty - 1, tx - 1] = v[tz, ty, tx] = FG
    elif name == "edge":                                       # ... only across a tile edge
        v[tz - 1, ty - 1, 3] = v[tz, ty, 3] = FG
    elif name == "full":
        v[...] = FG
    else:
        assert name == "empty"
    return v


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name.startswith("built:"):
        v = _built(name[6:])
    elif name in ("r70_u8", "r70_f32"):
        rng = np.random.default_rng(700)
        v = rng.integers(0, 256, (20, 40, 70), dtype=np.uint8) if name == "r70_u8" else rng.random((20, 40, 70), dtype=f32)
    elif ":" in name and name.split(":")[0] in ("u8", "f32"):  # "u8:17x9x9": random bytes / in-domain f32
        kind, shape = name.split(":")
        nx, ny, nz = (int(s) for s in shape.split("x"))
        rng = np.random.default_rng(900 + nx * 7 + ny * 3 + nz)
        v = rng.integers(0, 256, (nz, ny, nx), dtype=np.uint8) if kind == "u8" else rng.random((nz, ny, nx), dtype=f32)
    else:
        return TH._volume(name)
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want(volname, bins, conn, box=None):
    """The model's (labels, sizes, stats) of one case: computed once, shared by the tests, never changed."""
    labels, sizes, stats = LM.label(_volume(volname), bins, conn, box)
    labels.setflags(write=False)
    sizes.setflags(write=False)
    return labels, sizes, stats


def _stats_tuple(s):
    return (int(s.foreground), int(s.components), int(s.largest_size), int(s.largest_label), int(s.reserved))


def _check(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    VO.report(got, want, LM.same(got, want), what)


def _scipy_labels(fg, conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    lab, n = ndimage.label(fg, ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]))
    out = np.zeros(fg.shape, np.uint32)
    if n:
        least = ndimage.minimum(np.arange(fg.size).reshape(fg.shape), lab, np.arange(1, n + 1))
        out[lab > 0] = np.asarray(least, np.int64)[lab[lab > 0] - 1] + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_label_calls():
    lib = vv.load_library()
    for name in ("vv_label_volume", "vv_mask_volume"):
        assert name in vv.EXPORTS and name in vv._NEWER_EXPORTS and hasattr(lib, name), f"{name} is not exported"
    for name in ("label", "label_device", "mask", "mask_device", "keep_component"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    assert (vv.KEEP_LABEL, vv.KEEP_FOREGROUND, vv.KEEP_MIN_SIZE) == (0, 1, 2) == (LM.KEEP_LABEL, LM.KEEP_FOREGROUND, LM.KEEP_MIN_SIZE)
    assert (C.sizeof(vv.vv_label), C.sizeof(vv.vv_label_stats), C.sizeof(vv.vv_mask)) == (36, 32, 48)
    assert (vv.vv_label.bin_lo.offset, vv.vv_label.connectivity.offset) == (24, 32)
    s, m = vv.vv_label_stats, vv.vv_mask
    assert (s.foreground.offset, s.components.offset, s.largest_size.offset, s.largest_label.offset, s.reserved.offset) == (0, 8, 16, 24, 28)
    assert (m.out_type.offset, m.keep.offset, m.invert.offset, m.label.offset, m.min_size.offset, m.fill.offset) == (24, 28, 32, 36, 40, 44)


@pytest.mark.parametrize("volname,bins", [("r70_u8", (0, 78)), ("r70_u8", (0, 24)), ("aniso", (60, 100)), ("built:snake", (FG, FG)), ("built:serpentine", (FG, FG)),
                                          ("built:comb", (FG, FG)), ("special_f32", (0, 0)), ("u8:17x9x9", (0, 127))])
def test_model_equals_scipy(volname, bins):
    fg = LM.foreground(_volume(volname), bins)
    for conn in CONNS:
        want = _scipy_labels(fg, conn)
        labels, sizes, stats = _want(volname, bins, conn)
        assert np.array_equal(labels, want), (volname, bins, conn)
        assert np.array_equal(sizes.ravel()[labels[labels > 0].astype(np.int64) - 1], np.bincount(want.ravel())[want[want > 0]])
        assert stats.components == len(np.unique(want[want > 0]))


def test_model_identities():
    vol = _volume("r70_u8")
    for conn, bins in PERCOLATION:
        labels, sizes, stats = _want("r70_u8", bins, conn)
        fg = LM.foreground(vol, bins)
        assert int(sizes.sum()) == stats.foreground == int(fg.sum()) and np.array_equal(labels != 0, fg)
        assert stats.components == int((sizes > 0).sum()) == len(np.unique(labels[fg])) > 100
        assert stats.largest_size == int(sizes.max()) and sizes.ravel()[stats.largest_label - 1] == stats.largest_size
        assert np.array_equal(np.flatnonzero(sizes.ravel()) + 1, np.unique(labels[fg]))          # sizes sit at the least voxels
        assert (labels.ravel()[fg.ravel()] <= np.flatnonzero(fg.ravel()) + 1).all()
    # refinement: 6 inside 18 inside 26 (equal labels under the finer stay equal under the coarser)
    l6, l18, l26 = (_want("r70_u8", (0, 34), c)[0].ravel().astype(np.int64) for c in CONNS)
    fgi = np.flatnonzero(l6)
    for fine, coarse in ((l6, l18), (l18, l26)):
        assert np.array_equal(coarse[fine[fgi] - 1], coarse[fgi]) and (coarse[fgi] <= fine[fgi]).all()
    assert len(np.unique(l6)) > len(np.unique(l18)) > len(np.unique(l26))
    # every bin: one component with label 1
    labels, sizes, stats = _want("aniso", (0, 255), 6)
    assert (labels == 1).all() and sizes.ravel()[0] == labels.size == sizes.sum() and _stats_tuple(stats) == (labels.size, 1, labels.size, 1, 0)
    # the checkerboard: one component per voxel under 6, one under 18 and 26
    z, y, x = np.indices((5, 6, 7))
    board = (x + y + z) % 2 == 0
    l6, s6, st6 = LM.components(board, 6)
    assert np.array_equal(l6, np.where(board, np.arange(board.size).reshape(board.shape) + 1, 0)) and st6.components == board.sum() and st6.largest_label == 1
    for conn in (18, 26):
        l, s, st = LM.components(board, conn)
        assert st.components == 1 and (l[board] == 1).all() and st.largest_size == board.sum()
    # no foreground
    l, s, st = LM.components(np.zeros((3, 4, 5), bool), 26)
    assert not l.any() and not s.any() and _stats_tuple(st) == (0, 0, 0, 0, 0)
    # the built pairs: the corner joins under 26 only, the edge under 18 and 26
    assert [_want("built:corner", (FG, FG), c)[2].components for c in CONNS] == [2, 2, 1]
    assert [_want("built:edge", (FG, FG), c)[2].components for c in CONNS] == [2, 1, 1]
    for name in ("snake", "serpentine", "comb"):
        assert _want("built:" + name, (FG, FG), 6)[2].components == 1, name
    assert _want("built:comb", (FG, FG), 6, ((0, 0, 0), (69, 40, 20)))[2].components == 200           # without the spine: 10 x 20 teeth


def test_model_mask_identities():
    for volname in ("r37_u8", "rand_f32", "special_f32"):
        vol = _volume("u8:37x21x13") if volname == "r37_u8" else _volume(volname)
        box = ((1, 2, 3), (9, 8, 10))
        ones = np.ones(HM.crop(vol, box).shape, np.uint32)
        for out_type in (LM.U8, LM.F32):
            got = LM.mask(vol, ones, LM.KEEP_FOREGROUND, box=box, out_type=out_type, fill=3.0)
            assert len(DM.same(got, DM.derive(vol, box, 1, DM.MEAN, out_type))) == 0, (volname, out_type)
            none = LM.mask(vol, ones, LM.KEEP_FOREGROUND, invert=True, box=box, out_type=out_type, fill=0.37)
            assert len(np.unique(none.view(np.uint32 if none.dtype == f32 else np.uint8))) == 1
    import resample_model as RM
    for fill in (0.0, 93.5, 0.37, 0.49999997, 0.5, 254.5, 300.0, -1.0, 1.0, 2.0 ** -10):
        for dt in (np.uint8, np.float32):
            for out_type in (LM.U8, LM.F32):
                a, b = LM.fill_stage(fill, dt, out_type), RM.finish(np.full(1, fill, f32), dt, out_type)[0]
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (fill, dt, out_type)
    assert LM.fill_stage(93.5, np.uint8, LM.U8) == 94


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _load(ctx, monkeypatch, volname):
    VO.load(ctx, monkeypatch, LAYOUT_KNOBS, _volume(volname), TF)


class LabelOut(VO.GuardedOuts):
    """The guarded device buffer of a label call: labels and sizes at a start that moves by 4 bytes (from call to call; every fourth call), stats by 8."""

    def __init__(self, voxels):
        super().__init__(2 * (4 * voxels + 16) + 32 + 16 + 4 * GUARD, 8)
        self.voxels = voxels

    def run(self, call, shape, sizes=True, stats=True, what=""):
        """call(labels_ptr, capacity, sizes_ptr, stats_ptr), complete on return -> labels, sizes or None, stats tuple or None"""
        n = int(np.prod(shape)) * 4
        assert n <= 4 * self.voxels
        outs = [VO.Out(n), VO.Out(n, digit=4, present=sizes), VO.Out(32, align=8, present=stats)]
        l, s, t = self.run_outs(lambda p: call(p[0], n, p[1], p[2]), outs, what)
        return (l.view(np.uint32).reshape(shape), s.view(np.uint32).reshape(shape) if sizes else None,
                _stats_tuple(vv.LabelStats.from_bytes(t)) if stats else None)


def _run_case(ctx, dev, what, want, bins, conn, box=None, host=True):
    """One case through the device buffer (labels, sizes and stats) and, with `host`, through host pointers (every combination of the optional outputs
    over the calls, by the device buffer's call count)."""
    labels, sizes, stats = want
    what = f"{what} bins {bins} connectivity {conn} box {box}"
    gl, gs, gt = dev.run(lambda lp, cap, sp, tp: ctx.label_device(lp, cap, bins, conn, box, sizes_ptr=sp, stats_ptr=tp), labels.shape, what=what)
    _check(gl, labels, what + " labels")
    _check(gs, sizes, what + " sizes")
    assert gt == _stats_tuple(stats), (what, gt, stats)
    if not host:
        return
    k = dev.calls % 4
    got = ctx.label(bins, conn, box, sizes=bool(k & 1), stats=bool(k & 2), prefill=GARBAGE if k < 2 else 0)
    got = got if isinstance(got, tuple) else (got,)
    _check(got[0], labels, what + " host labels")
    if k & 1:
        _check(got[1], sizes, what + " host sizes")
    if k & 2:
        model = stats if k & 1 else LM.stats_without_sizes(stats)
        assert _stats_tuple(got[-1]) == _stats_tuple(model), (what, got[-1], model)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_label_shapes(ctx, shape, monkeypatch):
    """1 x 1 x 1, 2 x 1 x 3, 1 x 40 x 1, the tile, one voxel more and one less on every axis, 37 x 21 x 13: u8 and in-domain f32."""
    nvox = int(np.prod([int(s) for s in shape.split("x")]))
    dev = LabelOut(nvox)
    for kind in ("u8", "f32"):
        name = f"{kind}:{shape}"
        _load(ctx, monkeypatch, name)
        for conn in CONNS:
            for bins in ((0, 100), (128, 255), (0, 255), (77, 77)):
                _run_case(ctx, dev, name, _want(name, bins, conn), bins, conn)


@pytest.mark.gpu
@pytest.mark.parametrize("conn,bins", PERCOLATION)
@pytest.mark.parametrize("volname", ["r70_u8", "r70_f32"])
def test_label_percolation(ctx, volname, conn, bins, monkeypatch):
    """70 x 40 x 20 random foreground at about 0.31 (6), 0.137 (18), 0.097 (26) and 0.6 (6): thousands of components that cross tiles."""
    _load(ctx, monkeypatch, volname)
    want = _want(volname, bins, conn)
    if volname == "r70_u8":
        assert want[2].components > (100 if bins[1] > 100 else 900) and want[2].largest_size > 100
    _run_case(ctx, LabelOut(56000), volname, want, bins, conn)


@pytest.mark.gpu
def test_label_aniso_and_the_bin_rule(ctx, monkeypatch):
    """The committed brain (its shells), and the f32 volume with NaN, +-Inf and values below 1 / 255: bin 0 holds the NaNs, bin 255 +Inf."""
    dev = LabelOut(52 * 36 * 20)
    _load(ctx, monkeypatch, "aniso")
    for conn in CONNS:
        for bins in ((60, 60), (80, 120), (1, 255), (0, 0)):
            _run_case(ctx, dev, "aniso", _want("aniso", bins, conn), bins, conn)
    _load(ctx, monkeypatch, "special_f32")
    vol = _volume("special_f32")
    assert LM.foreground(vol, (0, 0))[np.isnan(vol)].all() and LM.foreground(vol, (255, 255))[vol == np.inf].all() and LM.foreground(vol, (0, 0))[vol == -np.inf].all()
    for conn in CONNS:
        for bins in ((0, 0), (255, 255), (1, 254), (0, 255), (1, 1)):
            _run_case(ctx, dev, "special_f32", _want("special_f32", bins, conn), bins, conn)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["serpentine", "snake", "comb", "corner", "edge", "full", "empty"])
def test_label_built_shapes(ctx, name, monkeypatch):
    """The smallest shapes at which each phase can go wrong: the in-tile path, merges that chain through every tile, teeth that join in the last
    tile, contacts across a tile corner and a tile edge, all and no foreground."""
    volname = "built:" + name
    _load(ctx, monkeypatch, volname)
    dev = LabelOut(_volume(volname).size)
    for conn in CONNS:
        want = _want(volname, (FG, FG), conn)
        _run_case(ctx, dev, volname, want, (FG, FG), conn)
        if name == "empty":
            assert _stats_tuple(want[2]) == (0, 0, 0, 0, 0) and not want[0].any() and not want[1].any()
        if name in ("snake", "serpentine", "full"):
            assert want[2].components == 1
    if name == "snake":                                          # the snake's background: many voxels, few components
        _run_case(ctx, dev, volname + " background", _want(volname, (0, 0), 6), (0, 0), 6)


@pytest.mark.gpu
def test_label_boxes(ctx, monkeypatch):
    """Boxes that are not tile-aligned, one voxel, and a box that cuts a component in two: the result for a box is not the crop of the whole."""
    _load(ctx, monkeypatch, "r70_u8")
    dev = LabelOut(56000)
    boxes = [((3, 5, 1), (70, 40, 20)), ((17, 9, 9), (18, 10, 10)), ((1, 1, 1), (69, 39, 19)), ((15, 7, 7), (34, 17, 17)), ((0, 0, 0), (16, 8, 8)), ((5, 0, 3), (6, 40, 4))]
    for k, box in enumerate(boxes):
        conn, bins = PERCOLATION[k % 4]
        _run_case(ctx, dev, "r70_u8", _want("r70_u8", bins, conn, box), bins, conn, box)
    _load(ctx, monkeypatch, "built:comb")
    whole, cut = _want("built:comb", (FG, FG), 6), _want("built:comb", (FG, FG), 6, ((0, 0, 0), (69, 2, 3)))
    assert whole[2].components == 1 and cut[2].components == 2 and len(np.unique(cut[0])) == 3
    _run_case(ctx, dev, "comb cut", cut, (FG, FG), 6, ((0, 0, 0), (69, 2, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("volname,conn,bins", [("r70_u8", 6, (0, 78)), ("r70_u8", 26, (0, 24)), ("built:snake", 6, (FG, FG)), ("built:comb", 18, (FG, FG))])
def test_label_block_order(ctx, volname, conn, bins, monkeypatch):
    """VV_LABEL_BLOCKS = 1, 8 and unset: one block takes every tile in turn, eight share them, one block per tile; the same words, and the same
    words from a second run."""
    _load(ctx, monkeypatch, volname)
    want = _want(volname, bins, conn)
    dev = LabelOut(56000)
    try:
        for blocks in ("1", "8", None):
            if blocks is None:
                monkeypatch.delenv("VV_LABEL_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("VV_LABEL_BLOCKS", blocks)
            ctx.reread_env()
            _run_case(ctx, dev, f"VV_LABEL_BLOCKS={blocks} {volname}", want, bins, conn)
            first = ctx.label(bins, conn, sizes=True, stats=True, prefill=GARBAGE)
            second = ctx.label(bins, conn, sizes=True, stats=True, prefill=0)
            assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2], "a second run differs"
            out = ctx.mask(first[0], vv.KEEP_MIN_SIZE, min_size=5, sizes=first[1], fill=7.0, prefill=GARBAGE)
            _check(out, LM.mask(_volume(volname), want[0], LM.KEEP_MIN_SIZE, min_size=5, sizes=want[1], fill=7.0), f"mask under VV_LABEL_BLOCKS={blocks}")
    finally:
        monkeypatch.delenv("VV_LABEL_BLOCKS", raising=False)
        ctx.reread_env()


@pytest.mark.gpu
@VO.layout_sweep
def test_label_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume (32 bytes of zeros behind every row, with and without an extra row of zeros per slice) and the 64-bit addressing build.
    The volume holds no zero: bin 0 is empty unless padding is read as data."""
    with VO.layout_context(kind, nx, knobs, monkeypatch, LAYOUT_KNOBS, TF) as (c, vol):
        nz, ny, _ = vol.shape
        dev = LabelOut(vol.size)
        for conn, bins, box in ((6, (1, 100), None), (18, (200, 255), ((1, 0, 1), (nx - 1, ny, nz - 1))), (26, (0, 40), None), (6, (0, 0), None)):
            want = LM.label(vol, bins, conn, box)
            _run_case(c, dev, f"layout {kind} {knobs}", want, bins, conn, box)
            out = c.mask(want[0], vv.KEEP_MIN_SIZE, min_size=3, sizes=want[1], fill=1.0, box=box, prefill=GARBAGE)
            _check(out, LM.mask(vol, want[0], LM.KEEP_MIN_SIZE, min_size=3, sizes=want[1], fill=1.0, box=box), f"mask, layout {kind} {knobs}")
        assert c.label((0, 0), 6, stats=True)[1].foreground == 0, "padding was read as data"


@pytest.mark.gpu
def test_label_load_paths_and_streams(ctx, monkeypatch):
    """A volume that came from a device buffer and one promoted by the streamed upload; then an enqueue-only call on a torch stream, synchronised
    by the stream alone."""
    import torch
    tdev = torch.device("cuda", 0)
    vol8 = _volume("u8:37x21x13")
    dev = LabelOut(vol8.size)
    for (what, vol), conn in zip(VO.load_paths(ctx, monkeypatch, LAYOUT_KNOBS, vol8, TF), (18, 26)):
        _run_case(ctx, dev, what, _want("u8:37x21x13", (0, 100), 18) if vol is vol8 else LM.label(vol, (0, 100), 26), (0, 100), conn)
    assert np.array_equal(HM.bins(vol), vol8)
    # enqueue only
    _load(ctx, monkeypatch, "r70_u8")
    conn, bins = 6, (0, 78)
    labels, sizes, stats = _want("r70_u8", bins, conn)
    ts = torch.cuda.Stream(device=tdev)
    n = labels.size
    lab_t = torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    siz_t = torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    st_t = torch.full((4,), -1, dtype=torch.int64, device=tdev)
    out_t = torch.full((n + GUARD,), GARBAGE, dtype=torch.uint8, device=tdev)
    torch.cuda.synchronize()
    with vv.Context(0) as second:
        with torch.cuda.stream(ts):
            h = vv.stream_handle(ts)
            assert ctx.label_device(lab_t.data_ptr(), n * 4, bins, conn, sizes_ptr=siz_t.data_ptr(), stats_ptr=st_t.data_ptr(), stream=h) == (70, 40, 20)
            ctx.mask_device(out_t.data_ptr(), n, lab_t.data_ptr(), vv.KEEP_LABEL, label=stats.largest_label, fill=0.0, stream=h)
            second.load_volume_device(out_t.data_ptr(), vv.VOXEL_U8, 70, 40, 20, TF, stream=h)
        ts.synchronize()
        _check(lab_t.cpu().numpy().view(np.uint32).reshape(labels.shape), labels, "enqueue-only labels")
        _check(siz_t.cpu().numpy().view(np.uint32).reshape(labels.shape), sizes, "enqueue-only sizes")
        assert _stats_tuple(vv.LabelStats.from_bytes(st_t.cpu().numpy().tobytes())) == _stats_tuple(stats)
        want_vol = LM.mask(_volume("r70_u8"), labels, LM.KEEP_LABEL, label=stats.largest_label)
        raw = out_t.cpu().numpy()
        assert np.array_equal(raw[:n].reshape(labels.shape), want_vol) and (raw[n:] == GARBAGE).all()
        # "render only this structure": the loaded result re-histogrammed has the model's counts
        TH._same(second.histogram(prefill=GARBAGE), HM.histogram(want_vol), "histogram of the masked volume")


MASK_VOLUMES = ("u8:37x21x13", "f32:37x21x13", "special_f32")


@pytest.mark.gpu
@pytest.mark.parametrize("volname", MASK_VOLUMES)
def test_mask_matches_model(ctx, volname, monkeypatch):
    """All three keep modes, both inversions, all four type pairs (two per volume), fills 0 and 93.5 / 0.37; labels from the call, labels that are
    arbitrary values in 0..voxels, and labels above the voxel count under VV_KEEP_LABEL; through the guarded device buffer and the host path."""
    import torch
    tdev = torch.device("cuda", 0)
    _load(ctx, monkeypatch, volname)
    vol = _volume(volname)
    n = vol.size
    dev = VO.DeviceOut(n * 4)
    rng = np.random.default_rng(77)
    fills = (0.0, 93.5 if vol.dtype == np.uint8 else 0.37)
    box = ((2, 1, 3), (vol.shape[2] - 1, vol.shape[1], vol.shape[0] - 2))
    called = ctx.label((0, 110), 18, sizes=True, prefill=GARBAGE)
    _check(called[0], _want(volname, (0, 110), 18)[0], "labels for the mask")
    boxed = ctx.label((0, 110), 6, box, sizes=True)
    arbitrary = (rng.integers(0, n + 1, vol.shape).astype(np.uint32), rng.integers(0, 9, vol.shape).astype(np.uint32))
    above = rng.choice(np.array([0, 1, 5, n, n + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 2], np.uint32), vol.shape)
    some = int(called[0][called[0] > 0][len(called[0][called[0] > 0]) // 2]) if called[0].any() else 1
    cases = [(called[0], called[1], None, dict(keep=vv.KEEP_LABEL, label=some)), (called[0], called[1], None, dict(keep=vv.KEEP_FOREGROUND)),
             (called[0], called[1], None, dict(keep=vv.KEEP_MIN_SIZE, min_size=4)), (called[0], called[1], None, dict(keep=vv.KEEP_MIN_SIZE, min_size=0)),
             (boxed[0], boxed[1], box, dict(keep=vv.KEEP_MIN_SIZE, min_size=2)), (boxed[0], None, box, dict(keep=vv.KEEP_LABEL, label=int(boxed[0].max()))),
             (arbitrary[0], arbitrary[1], None, dict(keep=vv.KEEP_MIN_SIZE, min_size=3)), (arbitrary[0], None, None, dict(keep=vv.KEEP_LABEL, label=0)),
             (above, None, None, dict(keep=vv.KEEP_LABEL, label=2 ** 32 - 1)), (above, None, None, dict(keep=vv.KEEP_LABEL, label=n + 1)),
             (above, None, None, dict(keep=vv.KEEP_FOREGROUND))]
    k = 0
    for labels, sizes, bx, kw in cases:
        lab_t = torch.from_numpy(labels.view(np.int32).copy()).to(tdev)
        siz_t = torch.from_numpy(sizes.view(np.int32).copy()).to(tdev) if sizes is not None else None
        for invert in (False, True):
            for out_type in (vv.VOXEL_U8, vv.VOXEL_F32):
                k += 1
                fill = fills[k % 2]
                want = LM.mask(vol, labels, sizes=sizes, invert=invert, fill=fill, box=bx, out_type=out_type, **kw)
                what = f"{volname} {kw} invert {invert} out_type {out_type} fill {fill} box {bx}"
                got = dev.run(lambda p, cap: ctx.mask_device(p, cap, lab_t.data_ptr(), sizes_ptr=siz_t.data_ptr() if sizes is not None else 0, invert=invert, fill=fill,
                                                             box=bx, out_type=out_type, **kw), want.shape, want.dtype.type, what)
                _check(got, want, what)
                if k % 3 == 0:
                    _check(ctx.mask(labels, sizes=sizes, invert=invert, fill=fill, box=bx, out_type=out_type, prefill=GARBAGE, **kw), want, what + " host")
    # the derive identity: the labels of bins 0..255 under VV_KEEP_FOREGROUND
    for bx in (None, box):
        ones = ctx.label((0, 255), 6, bx)
        assert (ones == 1).all()
        for out_type in (vv.VOXEL_U8, vv.VOXEL_F32):
            assert ctx.mask(ones, vv.KEEP_FOREGROUND, fill=5.0, box=bx, out_type=out_type, prefill=GARBAGE).tobytes() == \
                ctx.derive(bx, 1, out_type=out_type, prefill=0).tobytes(), (volname, bx, out_type)


@pytest.mark.gpu
def test_keep_component_is_the_seeded_region_grow(ctx, monkeypatch):
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    conn, bins = 6, (0, 78)
    labels, sizes, stats = _want("r70_u8", bins, conn)
    order = np.argsort(sizes.ravel())[::-1][:3]                 # the three largest components: seeds at their least voxel and at their last one
    for r in order:
        members = np.argwhere(labels == r + 1)
        for z, y, x in (members[0], members[-1]):
            got = ctx.keep_component((int(x), int(y), int(z)), bins, conn, fill=255.0)
            _check(got, LM.mask(vol, labels, LM.KEEP_LABEL, label=int(r) + 1, fill=255.0), f"keep_component, seed {(x, y, z)}")
            assert int((got != 255).sum()) == sizes.ravel()[r]
    z, y, x = np.argwhere(labels == 0)[0]
    with pytest.raises(ValueError):
        ctx.keep_component((int(x), int(y), int(z)), bins, conn)
    box = ((10, 4, 2), (60, 30, 18))
    bl = _want("r70_u8", bins, 26, box)[0]
    z, y, x = np.argwhere(bl == bl.max())[0]
    got = ctx.keep_component((int(x) + 10, int(y) + 4, int(z) + 2), bins, 26, box=box, out_type=vv.VOXEL_F32, invert=True, fill=0.37)
    _check(got, LM.mask(vol, bl, LM.KEEP_LABEL, label=int(bl.max()), invert=True, fill=0.37, box=box, out_type=LM.F32), "keep_component in a box")
    with pytest.raises(ValueError):
        ctx.keep_component((0, 0, 0), bins, 26, box=box)


@pytest.mark.gpu
def test_label_and_mask_errors_and_state(ctx, monkeypatch):
    import torch
    tdev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h

    def mk(lo=(0, 0, 0), hi=(0, 0, 0), bin_lo=0, bin_hi=100, conn=6):
        d = vv.vv_label()
        d.box_lo[:], d.box_hi[:] = lo, hi
        d.bin_lo, d.bin_hi, d.connectivity = bin_lo, bin_hi, conn
        return d

    def mm(lo=(0, 0, 0), hi=(0, 0, 0), out_type=vv.VOXEL_U8, keep=vv.KEEP_FOREGROUND, invert=0, label=0, min_size=0, fill=0.0):
        d = vv.vv_mask()
        d.box_lo[:], d.box_hi[:] = lo, hi
        d.out_type, d.keep, d.invert, d.label, d.min_size, d.fill = out_type, keep, invert, label, min_size, fill
        return d

    with vv.Context(0) as empty:                                    # before a load: behind the NULL checks, before a bad descriptor
        out = np.full(256, GARBAGE, np.uint8)
        assert lib.vv_label_volume(empty.h, C.byref(mk(conn=7)), out.ctypes.data, out.nbytes, None, None, 0, None) == ERR_NO_VOLUME
        assert lib.vv_label_volume(empty.h, None, out.ctypes.data, out.nbytes, None, None, 0, None) == ERR_INVALID
        assert lib.vv_mask_volume(empty.h, C.byref(mm(keep=9)), out.ctypes.data, None, out.ctypes.data, out.nbytes, 0, None) == ERR_NO_VOLUME
        assert lib.vv_mask_volume(empty.h, C.byref(mm()), None, None, out.ctypes.data, out.nbytes, 0, None) == ERR_INVALID
        assert (out == GARBAGE).all()
        with pytest.raises(vv.VolvizError) as e:
            empty.label((0, 1))
        assert e.value.code == ERR_NO_VOLUME
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    nz, ny, nx = vol.shape
    n = vol.size
    before = VO.Untouched(ctx)

    host = np.full(2 * n * 4 + 64 + GUARD, GARBAGE, np.uint8)
    raw = torch.full((2 * n * 4 + 64 + GUARD,), GARBAGE, dtype=torch.uint8, device=tdev)
    torch.cuda.synchronize()
    hp, dp = host.ctypes.data, raw.data_ptr()
    assert dp % 8 == 0

    def both(d, sizes=True, stats=True):
        """The status of a host-output and of a device-output call (ample capacity) for one descriptor: they must agree."""
        rc = [lib.vv_label_volume(hnd, C.byref(d), p, n * 4, p + n * 4 if sizes else None, p + 2 * n * 4 if stats else None, dev, None) for p, dev in ((hp, 0), (dp, 1))]
        assert rc[0] == rc[1], rc
        return rc[0]

    def mboth(d, sizes=True):
        rc = [lib.vv_mask_volume(hnd, C.byref(d), p, p + n * 4 if sizes else None, p + 2 * n * 4, 64 + GUARD, dev, None) for p, dev in ((hp, 0), (dp, 1))]
        assert rc[0] == rc[1], rc
        return rc[0]

    good = mk()
    assert lib.vv_label_volume(None, C.byref(good), hp, n * 4, None, None, 0, None) == ERR_INVALID
    assert lib.vv_label_volume(hnd, None, hp, n * 4, None, None, 0, None) == ERR_INVALID
    assert lib.vv_label_volume(hnd, C.byref(good), None, n * 4, None, None, 0, None) == ERR_INVALID
    bad_boxes = (((-1, 0, 0), (nx, ny, nz)), ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny, nz + 1)), ((3, 0, 0), (3, ny, nz)), ((0, 5, 0), (nx, 4, nz)), ((1, 0, 0), (0, 0, 0)))
    for lo, hi in bad_boxes:
        assert both(mk(lo, hi)) == ERR_INVALID, (lo, hi)
    for bin_lo, bin_hi in ((-1, 5), (0, 256), (7, 6), (300, 400)):
        assert both(mk(bin_lo=bin_lo, bin_hi=bin_hi)) == ERR_INVALID
    for conn in (0, 4, 8, 27, -6):
        assert both(mk(conn=conn)) == ERR_INVALID
    # the order: the box before the bins before the connectivity before the capacity (each leaves its message)
    for fix, word in ((dict(), "box"), (dict(lo=(0, 0, 0)), "bins"), (dict(lo=(0, 0, 0), bin_lo=0), "connectivity")):
        kw = dict(lo=(1, 0, 0), hi=(0, 0, 0), bin_lo=9, bin_hi=3, conn=5)
        kw.update(fix)
        assert lib.vv_label_volume(hnd, C.byref(mk(**kw)), dp, 0, None, None, 1, None) == ERR_INVALID
        assert word in lib.vv_last_error(hnd).decode(), (word, lib.vv_last_error(hnd))
    # capacity, alignment, overlap of labels and sizes
    for p, dev in ((hp, 0), (dp, 1)):
        assert lib.vv_label_volume(hnd, C.byref(good), p, n * 4 - 1, None, None, dev, None) == ERR_INVALID
        assert "capacity" in lib.vv_last_error(hnd).decode()
    assert lib.vv_label_volume(hnd, C.byref(good), dp + 2, 0, None, None, 1, None) == ERR_INVALID and "capacity" in lib.vv_last_error(hnd).decode()
    for off in (1, 2, 3):
        assert lib.vv_label_volume(hnd, C.byref(good), dp + off, n * 4, None, None, 1, None) == ERR_INVALID
        assert lib.vv_label_volume(hnd, C.byref(good), dp, n * 4, dp + n * 4 + off, None, 1, None) == ERR_INVALID
    assert lib.vv_label_volume(hnd, C.byref(good), dp, n * 4, None, dp + n * 4 + 4, 1, None) == ERR_INVALID and "stats" in lib.vv_last_error(hnd).decode()
    for soff in (0, 4, n * 4 - 4):
        assert lib.vv_label_volume(hnd, C.byref(good), dp + 4 * 8, n * 4, dp + soff, None, 1, None) == ERR_INVALID and "overlap" in lib.vv_last_error(hnd).decode()
    # the mask: NULLs, then the descriptor in order, then sizes, capacity, alignment, overlap
    assert lib.vv_mask_volume(None, C.byref(mm()), hp, None, hp + 2 * n * 4, n, 0, None) == ERR_INVALID
    assert lib.vv_mask_volume(hnd, None, hp, None, hp + 2 * n * 4, n, 0, None) == ERR_INVALID
    assert lib.vv_mask_volume(hnd, C.byref(mm()), None, None, hp + 2 * n * 4, n, 0, None) == ERR_INVALID
    assert lib.vv_mask_volume(hnd, C.byref(mm()), hp, None, None, n, 0, None) == ERR_INVALID
    for lo, hi in bad_boxes:
        assert mboth(mm(lo, hi)) == ERR_INVALID
    for kw in (dict(out_type=2), dict(out_type=-1), dict(keep=3), dict(keep=-1), dict(invert=2), dict(invert=-1), dict(fill=np.nan), dict(fill=np.inf), dict(fill=-np.inf)):
        assert mboth(mm(**kw)) == ERR_INVALID, kw
    assert mboth(mm(keep=vv.KEEP_MIN_SIZE), sizes=False) == ERR_INVALID and "sizes" in lib.vv_last_error(hnd).decode()
    for fix, word in ((dict(), "box"), (dict(lo=(0, 0, 0)), "out_type"), (dict(lo=(0, 0, 0), out_type=0), "keep"), (dict(lo=(0, 0, 0), out_type=0, keep=2), "invert"),
                      (dict(lo=(0, 0, 0), out_type=0, keep=2, invert=0), "fill"), (dict(lo=(0, 0, 0), out_type=0, keep=2, invert=0, fill=0.0), "sizes"),
                      (dict(lo=(0, 0, 0), out_type=0, keep=1, invert=0, fill=0.0), "capacity")):
        kw = dict(lo=(1, 0, 0), hi=(0, 0, 0), out_type=9, keep=9, invert=9, fill=np.nan)
        kw.update(fix)
        assert lib.vv_mask_volume(hnd, C.byref(mm(**kw)), dp, None, dp + 2 * n * 4, 64, 1, None) == ERR_INVALID
        assert word in lib.vv_last_error(hnd).decode(), (word, lib.vv_last_error(hnd))
    small = mm((1, 2, 3), (5, 6, 7))                               # 64 voxels
    for off in (1, 2, 3):
        assert lib.vv_mask_volume(hnd, C.byref(small), dp + off, None, dp + 2 * n * 4, 64, 1, None) == ERR_INVALID
        assert lib.vv_mask_volume(hnd, C.byref(small), dp, dp + 256 + off, dp + 2 * n * 4, 64, 1, None) == ERR_INVALID
        assert lib.vv_mask_volume(hnd, C.byref(mm((1, 2, 3), (5, 6, 7), out_type=vv.VOXEL_F32)), dp, None, dp + 2 * n * 4 + off, 256, 1, None) == ERR_INVALID
    assert lib.vv_mask_volume(hnd, C.byref(small), dp, None, dp + 2 * n * 4, 63, 1, None) == ERR_INVALID
    for ooff in (0, 255, 256 + 255):                               # out inside labels, inside sizes
        assert lib.vv_mask_volume(hnd, C.byref(small), dp, dp + 256, dp + ooff, 64, 1, None) == ERR_INVALID and "overlap" in lib.vv_last_error(hnd).decode()
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # exactly the needed capacity is enough
    box = ((1, 2, 3), (19, 30, 40))
    bl, bs, bt = _want("aniso", (60, 100), 18, box)
    need = bl.size * 4
    assert lib.vv_label_volume(hnd, C.byref(mk(*box, bin_lo=60, bin_hi=100, conn=18)), hp, need, hp + need, hp + 2 * need, 0, None) == 0
    _check(host[:need].view(np.uint32).reshape(bl.shape), bl, "exact capacity, labels")
    _check(host[need:2 * need].view(np.uint32).reshape(bl.shape), bs, "exact capacity, sizes")
    assert _stats_tuple(vv.LabelStats.from_bytes(host[2 * need:2 * need + 32])) == _stats_tuple(bt) and (host[2 * need + 32:] == GARBAGE).all()
    # a device-output call allocates no device memory: the device's free bytes stay what they were
    lab_t = torch.empty(n, dtype=torch.int32, device=tdev)
    siz_t = torch.empty(n, dtype=torch.int32, device=tdev)
    st_t = torch.empty(4, dtype=torch.int64, device=tdev)
    out_t = torch.empty(n * 4, dtype=torch.uint8, device=tdev)

    def calls():
        for conn in CONNS:
            ctx.label_device(lab_t.data_ptr(), n * 4, (60, 100), conn, sizes_ptr=siz_t.data_ptr(), stats_ptr=st_t.data_ptr())
            for out_type in (vv.VOXEL_U8, vv.VOXEL_F32):
                ctx.mask_device(out_t.data_ptr(), n * 4, lab_t.data_ptr(), vv.KEEP_MIN_SIZE, min_size=10, sizes_ptr=siz_t.data_ptr(), out_type=out_type)

    VO.free_memory_unchanged(calls, "a device-output call")
    # the context is still usable and untouched: volume, layout copies, residency, scratch, frame time, histogram, frames
    _check(ctx.label((60, 100), 6, prefill=GARBAGE), _want("aniso", (60, 100), 6)[0], "a good call after the refused ones")
    before.check()
