"""Surface meshes (vv_surface_mesh) against tests/mesh_model.py, every word exactly, floats as bit patterns.

CPU part: the library and the binding export the two calls, the structures have the header's sizes and offsets, the vectorised model equals the naive
per-cell loop on tiny volumes (u8 and f32, both caps, all four sources), the identities of the header's rule 8 hold on the model (8 (b) also against
region_model's faces), every crossing lies strictly inside its edge, and the host helpers (mesh_triangles, mesh_area_volume, write_obj) are held by
closed forms and a read-back parse.  GPU part: index, vertices, normals, quads and summary equal the model on every shape, source, cap, box and
capacity of the issue, into guarded device buffers prefilled with 0xA5 whose starts move from call to call, and through the host path; whatever the
chunk cap (VV_MESH_CHUNKS), the block order (VV_MESH_BLOCKS), the layout, the pitch and the load path; every error of rule 11 is refused in order; and
the call leaves the context alone.  The labels come from tests/label_model.py or are built here, so a case does not depend on vv_label_volume unless it
says so.  Every test must also pass under VV_MESH_BLOCKS=1, =8 and unset (left to whoever runs the suite, as test_regions.py does).

Not tested: the 2^32 - 2 limits on voxels and sites (no such volume is loaded here), the overlap refusals that need the address of the context's volume
(no public call tells it), and anything about the kernels' instructions."""
import ctypes as C

import numpy as np
import pytest

import hist_model as HM
import label_model as LM
import mesh_model as MM
import region_model as RM
import test_hist as TH
import test_label as TL
import test_regions as TR
import volume_out as VO
import volviz_amd as vv
from volume_out import GARBAGE, GUARD

f32 = np.float32
ERR_INVALID, ERR_NO_VOLUME = -1, -2
TF = TH.TF
CHUNK = 1024                                               # kMeshMinChunk of csrc/vv_kernels.h: the shortest chunk a wave walks
FG = TL.FG
LAYOUT_KNOBS = TH.LAYOUT_KNOBS + ("VV_MESH_CHUNKS",)       # (VV_MESH_BLOCKS is left to whoever runs the suite)
_cache = {}


def _volume(name):
    if name == "ramp":                                         # 70 x 40 x 20: two blobs whose bytes fall off with the distance, so levels cut smooth closed surfaces
        if name not in _cache:
            z, y, x = np.indices((20, 40, 70)).astype(np.float64)
            d = np.minimum(np.sqrt((x - 20.3) ** 2 + (y - 19.6) ** 2 + (z - 9.4) ** 2), 1.2 * np.sqrt((x - 49.7) ** 2 + (y - 17.1) ** 2 + ((z - 10.2) * 1.5) ** 2))
            _cache[name] = TR._freeze(np.clip(260.0 - 17.0 * d, 0, 255).astype(np.uint8))
        return _cache[name]
    return TR._volume(name)


def _same_mesh(a, b):
    return (a.index.tobytes() == b.index.tobytes() and a.index.shape == b.index.shape and a.vertices.tobytes() == b.vertices.tobytes() and
            a.normals.tobytes() == b.normals.tobytes() and a.quads.tobytes() == b.quads.tobytes() and a.summary == b.summary)


def _model(vol, src, cap, box=None, max_vertices=None, max_quads=None):
    """src: dict(level=) | dict(bins=) | dict(labels=, label=) | dict(labels=): the model's mesh of the case."""
    source = MM.INDEX if "level" in src else MM.BINS if "bins" in src else MM.LABEL if src.get("label") is not None else MM.NONZERO
    g, level = MM.field(vol, source, src.get("level"), src.get("bins"), src.get("labels"), src.get("label"), box)
    return MM.surface_mesh(g, level, cap, (0, 0, 0) if box is None else box[0], max_vertices, max_quads)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_mesh_calls():
    lib = vv.load_library()
    for name in ("vv_mesh_dims", "vv_surface_mesh"):
        assert name in vv.EXPORTS and name in vv._NEWER_EXPORTS and hasattr(lib, name), f"{name} is not exported"
    for name in ("surface", "surface_device", "mesh_dims"):
        assert callable(getattr(vv.Context, name, None)), f"Context.{name} is missing"
    for name in ("mesh_triangles", "mesh_area_volume", "write_obj"):
        assert callable(getattr(vv, name, None)), f"{name} is missing"
    assert (vv.MESH_INDEX, vv.MESH_BINS, vv.MESH_LABEL, vv.MESH_NONZERO) == (0, 1, 2, 3) == (MM.INDEX, MM.BINS, MM.LABEL, MM.NONZERO)


def test_structure_sizes_offsets_and_alignments():
    assert (C.sizeof(vv.vv_mesh), C.sizeof(vv.vv_mesh_vertex), C.sizeof(vv.vv_mesh_normal), C.sizeof(vv.vv_mesh_summary)) == (56, 16, 16, 32)
    assert (C.alignment(vv.vv_mesh), C.alignment(vv.vv_mesh_vertex), C.alignment(vv.vv_mesh_normal), C.alignment(vv.vv_mesh_summary)) == (4, 4, 4, 8)
    want = dict(box_lo=0, box_hi=12, source=24, level=28, bin_lo=32, bin_hi=36, label=40, cap=44, max_vertices=48, max_quads=52)
    assert {n: getattr(vv.vv_mesh, n).offset for n in want} == want
    assert [getattr(vv.vv_mesh_vertex, n).offset for n in ("x", "y", "z", "site")] == [0, 4, 8, 12]
    assert [getattr(vv.vv_mesh_normal, n).offset for n in ("g", "edges")] == [0, 12]
    assert [getattr(vv.vv_mesh_summary, n).offset for n in ("vertices", "quads", "written_vertices", "written_quads")] == [0, 8, 16, 24]
    for mine, theirs in ((vv.MESH_VERTEX_DTYPE, MM.VERTEX_DTYPE), (vv.MESH_NORMAL_DTYPE, MM.NORMAL_DTYPE)):
        assert mine.itemsize == theirs.itemsize == 16 and mine.names == theirs.names
        assert all(mine.fields[n][:2] == theirs.fields[n][:2] for n in mine.names)


def _tiny_cases():
    rng = np.random.default_rng(77)
    u8 = rng.integers(0, 256, (4, 5, 6), dtype=np.uint8)
    fl = rng.uniform(-0.1, 1.1, (4, 5, 6)).astype(f32)
    fl[1, 2, 3], fl[0, 0, 0], fl[3, 4, 5] = np.nan, np.inf, -np.inf
    labels = rng.integers(0, 3, (4, 5, 6)).astype(np.uint32)
    for vol in (u8, fl):
        for cap in (0, 1):
            for src in (dict(level=1), dict(level=77), dict(level=255), dict(bins=(40, 180)), dict(labels=labels, label=2), dict(labels=labels)):
                yield vol, src, cap


def test_vectorised_model_equals_the_loop_model():
    seen = 0
    for vol, src, cap in _tiny_cases():
        for box in (None, ((1, 0, 1), (5, 5, 4))):
            s = dict(src)
            if "labels" in s and box is not None:
                s["labels"] = np.ascontiguousarray(HM.crop(s["labels"], box))
            source = MM.INDEX if "level" in s else MM.BINS if "bins" in s else MM.LABEL if s.get("label") is not None else MM.NONZERO
            g, level = MM.field(vol, source, s.get("level"), s.get("bins"), s.get("labels"), s.get("label"), box)
            lo = (0, 0, 0) if box is None else box[0]
            fast, slow = MM.surface_mesh(g, level, cap, lo), MM.surface_mesh_loop(g, level, cap, lo)
            assert _same_mesh(fast, slow), (vol.dtype, src.keys(), cap, box)
            assert fast.dims == MM.dims(g.shape, cap)
            seen += fast.V
    assert seen > 2000


def test_rule_8_on_the_model():
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (9, 10, 11))
    ramp = _volume("ramp").astype(np.int64)
    most = 0
    for g, level in ((noise, 128), (noise, 40), (noise > 99, 1), (ramp, 128), (ramp, 255), (ramp[:, 5:30, 10:40], 100)):
        g = np.asarray(g, np.int64)
        closed, opened = MM.surface_mesh(g, level, 1), MM.surface_mesh(g, level, 0)
        # (a) closed, consistently oriented, no undirected edge more than 4 times
        most = max(most, MM.closed_and_oriented(closed.quads))
        assert MM.closed_and_oriented(closed.quads) <= 4
        # every quad has four distinct vertex numbers below V; with cap = 1 every vertex is used
        for mesh in (closed, opened):
            q = np.sort(mesh.quads.astype(np.int64), axis=1)
            assert (np.diff(q, axis=1) > 0).all() and (q < mesh.V).all()
        assert np.array_equal(np.unique(closed.quads), np.arange(closed.V))
        # (b) binary fields: Q is the number of boundary faces
        if level == 1:
            assert closed.Q == MM.boundary_faces(g >= 1)
        # (c) the open mesh is the sub-mesh on the sites whose corners are all real
        mz, my, mx = closed.index.shape
        inner = np.zeros((mz, my, mx), bool)
        inner[1:-1, 1:-1, 1:-1] = True
        keep = inner.ravel()[closed.vertices["site"]]
        assert opened.V == int(keep.sum())
        for n in "xyz":
            assert np.array_equal(closed.vertices[n][keep].view(np.uint32), opened.vertices[n].view(np.uint32))
        assert np.array_equal(closed.normals[keep], opened.normals)
        renumber = np.cumsum(keep) - 1
        sub = closed.quads[keep[closed.quads].all(axis=1)]
        assert np.array_equal(renumber[sub].astype(np.uint32), opened.quads)
    assert most == 4                                                # (the noise has ambiguous cells)
    # the smooth blobs are spheres: Euler characteristic 2 each, every undirected edge used exactly twice
    mesh = MM.surface_mesh(ramp, 128, 1)
    d = MM.directed_edges(mesh.quads)
    assert MM.closed_and_oriented(mesh.quads) == 2 and mesh.V - len(d) // 2 + mesh.Q == 4
    # (d) a box entirely inside
    for shape in ((2, 2, 2), (1, 1, 1), (3, 1, 4), (5, 4, 3)):
        bz, by, bx = shape
        full = MM.surface_mesh(np.ones(shape, np.int64), 1, 1)
        assert full.V == (bx + 1) * (by + 1) * (bz + 1) - (bx - 1) * (by - 1) * (bz - 1) and full.Q == 2 * (bx * by + by * bz + bx * bz)
        assert MM.surface_mesh(np.ones(shape, np.int64), 1, 0).summary == (0, 0, 0, 0)
    one, cube = MM.surface_mesh(np.ones((1, 1, 1), np.int64), 1, 1), MM.surface_mesh(np.ones((2, 2, 2), np.int64), 1, 1)
    assert (one.V, one.Q, cube.V, cube.Q) == (8, 6, 26, 24)
    # capacities: the written records are the first ones, the index and the counts do not change
    short = MM.surface_mesh(noise, 128, 1, max_vertices=7, max_quads=3)
    whole = MM.surface_mesh(noise, 128, 1)
    assert short.summary == (whole.V, whole.Q, 7, 3) and short.vertices.tobytes() == whole.vertices[:7].tobytes() and np.array_equal(short.quads, whole.quads[:3])


def test_rule_8b_against_the_region_model():
    vol = _volume("r70_u8")
    labels = LM.label(vol, (0, 153), 6)[0]
    row = RM.region_table(vol, labels, source=RM.NONZERO)[0][0]
    assert _model(vol, dict(labels=labels), 1).Q == int(row["faces"].sum()) > 0
    box = ((3, 5, 1), (61, 33, 17))
    sub = np.ascontiguousarray(HM.crop(labels, box))
    assert _model(vol, dict(labels=sub), 1, box).Q == int(RM.region_table(vol, sub, source=RM.NONZERO, box=box)[0][0]["faces"].sum())


def test_every_crossing_lies_strictly_inside_its_edge():
    gp, gq = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for level in range(1, 256):
        act = (gp >= level) != (gq >= level)
        t = (2 * level - 1 - 2 * gp[act]).astype(f32) / (2 * (gq[act] - gp[act])).astype(f32)
        assert t.dtype == f32 and (t > 0).all() and (t < 1).all(), level
    for a, b in ((0, 1), (1, 0)):
        assert f32(2 - 1 - 2 * a) / f32(2 * (b - a)) == f32(0.5)


def test_host_helpers(tmp_path):
    q = np.array([[0, 1, 2, 3], [4, 7, 6, 5]], np.uint32)
    assert np.array_equal(vv.mesh_triangles(q), [[0, 1, 2], [0, 2, 3], [4, 7, 6], [4, 6, 5]])
    # a single inside voxel under cap = 1: each of the eight cells around it has three crossings at 1/2, whose mean lies 1/6 from the voxel on every
    # axis: the mesh is the cube of side 1/3 around the voxel
    one = MM.surface_mesh(np.ones((1, 1, 1), np.int64), 1, 1)
    mesh = vv.Mesh(np.stack([one.vertices[n] for n in "xyz"], axis=1), one.vertices["site"], one.quads, one.normals.astype(vv.MESH_NORMAL_DTYPE))
    area, volume = vv.mesh_area_volume(mesh)
    assert np.isclose(area, 6.0 / 9.0, rtol=1e-6) and np.isclose(volume, 1.0 / 27.0, rtol=1e-6)       # (the coordinates are binary32)
    area, volume = vv.mesh_area_volume(mesh, (2.0, 3.0, 0.5))
    assert np.isclose(area, 2 * (6.0 + 1.5 + 1.0) / 9.0, rtol=1e-6) and np.isclose(volume, 3.0 / 27.0, rtol=1e-6)
    ramp = MM.surface_mesh(_volume("ramp").astype(np.int64), 128, 1)
    big = vv.Mesh(np.stack([ramp.vertices[n] for n in "xyz"], axis=1), ramp.vertices["site"], ramp.quads, ramp.normals.astype(vv.MESH_NORMAL_DTYPE))
    area, volume = vv.mesh_area_volume(big)
    inside = int((_volume("ramp") >= 128).sum())
    assert volume > 0 and abs(volume - inside) < 0.1 * inside and area > 0
    # OBJ: parse it back
    for m, spacing in ((mesh, (1, 1, 1)), (big, (0.5, 1.25, 2.0)), (vv.Mesh(big.vertices, big.sites, big.quads), (1, 1, 1))):
        path = tmp_path / "mesh.obj"
        vv.write_obj(str(path), m, spacing)
        v, vn, faces = [], [], []
        for line in path.read_text().splitlines():
            w = line.split()
            if w and w[0] == "v":
                v.append([float(t) for t in w[1:]])
            elif w and w[0] == "vn":
                vn.append([float(t) for t in w[1:]])
            elif w and w[0] == "f":
                faces.append([int(t.split("/")[0]) for t in w[1:]])
                assert all(t.split("/")[-1] == t.split("/")[0] for t in w[1:])
        assert np.allclose(v, m.vertices.astype(np.float64) * np.asarray(spacing), rtol=1e-8, atol=0)
        assert np.array_equal(np.asarray(faces) - 1, m.quads.astype(np.int64))
        if m.normals is None:
            assert not vn
        else:
            vn = np.asarray(vn)
            assert len(vn) == len(v) and np.allclose((vn * vn).sum(axis=1), 1.0, rtol=1e-7)
            want = m.normals["g"].astype(np.float64) / np.asarray(spacing)
            nz = (want * want).sum(axis=1) > 0
            assert np.allclose(vn[nz], want[nz] / np.sqrt((want[nz] ** 2).sum(axis=1))[:, None], atol=1e-7)
            # the normals point out of the inside: along the winding's face normals on the smooth mesh, summed per vertex
            if m is big:
                p = m.vertices.astype(np.float64)
                t = vv.mesh_triangles(m.quads).astype(np.int64)
                fn = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
                acc = np.zeros_like(p)
                for k in range(3):
                    np.add.at(acc, t[:, k], fn)
                assert ((acc * m.normals["g"]).sum(axis=1) > 0).mean() > 0.99


def test_model_dims_include_zeros():
    assert MM.dims((1, 1, 5), 0) == (4, 0, 0) and MM.dims((1, 1, 5), 1) == (6, 2, 2) and MM.dims((3, 2, 1), 0) == (0, 1, 2)
    empty = MM.surface_mesh(np.ones((1, 1, 5), np.int64), 1, 0)
    assert empty.summary == (0, 0, 0, 0) and empty.index.size == 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _load(ctx, monkeypatch, vol):
    VO.load(ctx, monkeypatch, LAYOUT_KNOBS, _volume(vol) if isinstance(vol, str) else vol, TF)


def _summary_tuple(s):
    return (int(s.vertices), int(s.quads), int(s.written_vertices), int(s.written_quads))


def _align(v, a):
    return (v + a - 1) // a * a


class MeshOut(VO.GuardedOuts):
    """The guarded device buffer of a mesh call: index at a start that moves by 4 bytes from call to call, the records by 16 (vertices every call,
    normals every second, quads every fourth), the summary by 8; the records that are not written must survive like the guards."""

    def __init__(self, sites, rows_v, rows_q):
        super().__init__(4 * sites + 32 * rows_v + 16 * rows_q + 32 + 6 * GUARD + 160, 16)
        self.sites, self.rows_v, self.rows_q = sites, rows_v, rows_q

    def run(self, call, dims, max_v, max_q, written, normals=True, summary=True, index=True, what=""):
        """call(index_ptr, index_capacity, vertices_ptr, normals_ptr, quads_ptr, summary_ptr), complete on return -> index, the written vertex, normal
        and quad records, the summary tuple (None where the output was not asked for)"""
        n = int(np.prod(dims)) * 4
        wv, wq = written
        assert n <= 4 * self.sites and max_v <= self.rows_v and max_q <= self.rows_q
        outs = [VO.Out(n, present=index), VO.Out(16 * max_v, 16 * wv, align=16, present=max_v > 0),
                VO.Out(16 * max_v, 16 * wv, align=16, digit=2, present=normals and max_v > 0), VO.Out(16 * max_q, 16 * wq, align=16, digit=4, present=max_q > 0),
                VO.Out(32, align=8, present=summary)]
        i, v, nr, q, s = self.run_outs(lambda p: call(p[0], n if index else 0, p[1], p[2], p[3], p[4]), outs, what)
        none = np.zeros(0, np.uint8)                                # (an output without a record to write: nothing of it was written)
        return (i.view(np.uint32).reshape(dims[::-1]) if index else None, (none if v is None else v).view(vv.MESH_VERTEX_DTYPE),
                (none if nr is None else nr).view(vv.MESH_NORMAL_DTYPE) if normals else None, (none if q is None else q).view(np.uint32).reshape(-1, 4),
                _summary_tuple(vv.MeshSummary.from_bytes(s)) if summary else None)


def _check_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        a, b = np.frombuffer(got.tobytes(), np.uint32).reshape(-1, 4), np.frombuffer(want.tobytes(), np.uint32).reshape(-1, 4)
        bad = np.flatnonzero((a != b).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} records differ, first record {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}")


def _check_volume(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    VO.report(got, want, np.argwhere(got != want), what)


def _host_call(ctx, d, labels, want, fill, normals, summary):
    """vv_surface_mesh on host arrays prefilled with the byte `fill`: index, vertices, normals, quads (all rows of the capacity), summary."""
    mx, my, mz = want.dims
    index = np.full(max(mx * my * mz, 1), fill * 0x01010101, np.uint32)
    vert = np.full(16 * max(d.max_vertices, 1), fill, np.uint8)
    norm = np.full(16 * max(d.max_vertices, 1), fill, np.uint8)
    quads = np.full(16 * max(d.max_quads, 1), fill, np.uint8)
    st = vv.vv_mesh_summary()
    C.memset(C.byref(st), fill, C.sizeof(st))
    rc = ctx.lib.vv_surface_mesh(ctx.h, C.byref(d), labels.ctypes.data if labels is not None else None, index.ctypes.data, 4 * mx * my * mz,
                                 vert.ctypes.data if d.max_vertices else None, 16 * d.max_vertices, norm.ctypes.data if normals and d.max_vertices else None,
                                 quads.ctypes.data if d.max_quads else None, 16 * d.max_quads, C.addressof(st) if summary else None, 0, None)
    assert rc == 0, ctx.lib.vv_last_error(ctx.h)
    return index[:mx * my * mz].reshape(mz, my, mx), vert, norm, quads, st


def _run_case(ctx, dev, what, vol, src, cap, box=None, max_vertices=None, max_quads=None, normals=True, summary=True, host=True):
    """One case through the guarded device buffers and, with `host`, through host pointers.  A maximum of None: one record per vertex / quad."""
    want = _model(vol, src, cap, box, max_vertices, max_quads)
    mv, mq = want.V if max_vertices is None else max_vertices, want.Q if max_quads is None else max_quads
    what = f"{what} {sorted(k for k in src)} {src.get('level', src.get('bins', src.get('label')))} cap {cap} box {box} max {mv} {mq}"
    labels = np.ascontiguousarray(src["labels"], np.uint32) if "labels" in src else None
    lab_t = dev.upload(labels) if labels is not None else None
    kw = dict(level=src.get("level"), bins=src.get("bins"), label=src.get("label"), labels_ptr=lab_t.data_ptr() if labels is not None else 0, cap=cap, box=box)
    assert ctx.mesh_dims(cap, box) == want.dims
    gi, gv, gn, gq, gs = dev.run(lambda ip, icap, vp, np_, qp, sp: ctx.surface_device(ip, icap, vp, mv, qp, mq, normals_ptr=np_, summary_ptr=sp, **kw),
                                 want.dims, mv, mq, want.summary[2:], normals=normals, summary=summary, what=what)
    _check_volume(gi, want.index, what + " index")
    _check_records(gv, want.vertices, what + " vertices")
    if normals:
        _check_records(gn, want.normals, what + " normals")
    assert np.array_equal(gq, want.quads), what + " quads"
    if summary:
        assert gs == want.summary, (what, gs, want.summary)
    if not host:
        return want
    fill = GARBAGE if dev.calls % 2 else 0x11
    d = ctx._mesh(src.get("level"), src.get("bins"), labels is not None, src.get("label"), cap, box, mv, mq)
    hi, hv, hn, hq, hs = _host_call(ctx, d, labels, want, fill, normals, summary)
    wv, wq = want.summary[2:]
    _check_volume(hi, want.index, what + " host index")
    _check_records(hv[:16 * wv].view(vv.MESH_VERTEX_DTYPE), want.vertices, what + " host vertices")
    assert (hv[16 * wv:] == fill).all() and (hq[16 * wq:] == fill).all(), what + ": a host record beyond `written` was touched"
    if normals:
        _check_records(hn[:16 * wv].view(vv.MESH_NORMAL_DTYPE), want.normals, what + " host normals")
        assert (hn[16 * wv:] == fill).all()
    else:
        assert (hn == fill).all()
    assert np.array_equal(hq[:16 * wq].view(np.uint32).reshape(-1, 4), want.quads), what + " host quads"
    if summary:
        assert _summary_tuple(hs) == want.summary, (what, _summary_tuple(hs), want.summary)
    return want


def _dev_for(vol, cap_extra=7):
    nz, ny, nx = vol.shape
    sites = (nx + 1) * (ny + 1) * (nz + 1)
    return MeshOut(sites, sites + cap_extra, 3 * sites + cap_extra)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["built:board", "ramp"])
def test_mesh_board_and_phantom(ctx, name, monkeypatch):
    """70 x 40 x 20: m_x is 69 and 71, so rows of sites wrap inside a 64-lane step and the sites span dozens of chunks.  Every cell of the board is
    ambiguous; the ramp's levels cut smooth closed surfaces."""
    _load(ctx, monkeypatch, name)
    vol = _volume(name)
    dev = _dev_for(vol)
    for cap in (1, 0):
        for src in ((dict(level=FG), dict(level=1), dict(bins=(FG, FG)), dict(bins=(0, 0))) if name == "built:board" else
                    (dict(level=128), dict(level=255), dict(level=1), dict(bins=(100, 200)))):
            want = _run_case(ctx, dev, name, vol, src, cap)
            if cap:
                assert MM.closed_and_oriented(want.quads) <= 4
        assert want.V > 0
    got = ctx.surface(level=128 if name == "ramp" else FG, normals=True, return_index=True)
    want = _model(vol, dict(level=128 if name == "ramp" else FG), 1)
    assert np.array_equal(got.vertices.view(np.uint32), np.stack([want.vertices[n] for n in "xyz"], axis=1).view(np.uint32)) and np.array_equal(got.sites, want.vertices["site"])
    assert np.array_equal(got.quads, want.quads) and got.normals.tobytes() == want.normals.tobytes() and np.array_equal(got.index, want.index)
    if name == "ramp":
        area, volume = vv.mesh_area_volume(got)
        assert volume > 0 and MM.closed_and_oriented(got.quads) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 1025])
def test_mesh_rows(ctx, nx, monkeypatch):
    """1 x 1 x N volumes: with cap = 1 the site grid is (N + 1) x 2 x 2, rows of 2, 64, 65, 66 and 1026 sites; with cap = 0 it has no site at all,
    which is a valid call with V = Q = 0."""
    name = f"row:{nx}"
    _load(ctx, monkeypatch, name)
    vol = _volume(name)
    dev = _dev_for(vol)
    med = max(int(np.median(vol)), 1)
    for src in (dict(level=med), dict(level=1), dict(bins=(0, 127)), dict(labels=TR._run_labels(vol.ravel() < 150))):
        want = _run_case(ctx, dev, name, vol, src, 1)
        assert want.dims == (nx + 1, 2, 2)
        empty = _run_case(ctx, dev, name, vol, src, 0, max_vertices=3, max_quads=2)
        assert empty.dims == (nx - 1, 0, 0) and empty.summary == (0, 0, 0, 0)
    assert ctx.mesh_dims(False) == (nx - 1, 0, 0)
    got = ctx.surface(level=med, cap=False, normals=True, return_index=True)
    assert got.vertices.shape == (0, 3) and got.quads.shape == (0, 4) and got.index.shape == (0, 0, nx - 1)


@pytest.mark.gpu
def test_mesh_small_boxes(ctx, monkeypatch):
    """Boxes of 1 x 1 x 1 and 2 x 2 x 2 voxels, one of extent 2 on x only (m_x = 1 without the cap), thin boxes on the other axes, and boxes off the
    origin: the coordinates are in volume voxel coordinates."""
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    dev = _dev_for(vol)
    boxes = [((17, 9, 9), (18, 10, 10)), ((5, 6, 7), (7, 8, 9)), ((30, 2, 3), (32, 38, 17)), ((3, 5, 1), (70, 7, 20)), ((1, 1, 4), (69, 39, 5)), ((3, 5, 1), (61, 33, 17))]
    for k, box in enumerate(boxes):
        for cap in (1, 0):
            want = _run_case(ctx, dev, "r70_u8", vol, dict(level=int(HM.crop(vol, box).max())), cap, box)
            _run_case(ctx, dev, "r70_u8", vol, dict(bins=(0, 90 + 20 * k)), cap, box)
        if k == 2:
            assert MM.dims(HM.crop(vol, box).shape, 0)[0] == 1
    want = _run_case(ctx, dev, "r70_u8 one voxel", vol, dict(bins=(0, 255)), 1, boxes[0])
    assert (want.V, want.Q) == (8, 6)
    want = _run_case(ctx, dev, "r70_u8 entirely inside", vol, dict(bins=(0, 255)), 1, boxes[1])
    assert (want.V, want.Q) == (26, 24)
    assert _run_case(ctx, dev, "r70_u8 entirely inside", vol, dict(bins=(0, 255)), 0, boxes[5]).summary == (0, 0, 0, 0)


@pytest.mark.gpu
def test_mesh_f32_specials_and_noise(ctx, monkeypatch):
    """NaN (g = 0), +-Inf, -0.0 and denormals under VV_MESH_INDEX at levels 1, 128 and 255; f32 and u8 noise at their median levels."""
    _load(ctx, monkeypatch, "specials")
    vol = _volume("specials")
    dev = _dev_for(vol)
    for level in (1, 128, 255):
        for cap in (1, 0):
            want = _run_case(ctx, dev, "specials", vol, dict(level=level), cap)
            assert want.V > 0
    _run_case(ctx, dev, "specials", vol, dict(bins=(0, 0)), 1)
    for name in ("r70_u8", "r70_f32"):
        _load(ctx, monkeypatch, name)
        vol = _volume(name)
        dev = _dev_for(vol)
        level = int(np.median(HM.bins(vol)))
        for cap in (1, 0):
            want = _run_case(ctx, dev, name, vol, dict(level=level), cap)
            assert want.V > 30000
        assert MM.closed_and_oriented(_model(vol, dict(level=level), 1).quads) == 4


@pytest.mark.gpu
def test_mesh_cap_does_not_see_outside_the_box(ctx, monkeypatch):
    """A sub-box strictly inside a volume whose outside is all 255: the cap's virtual voxels are 0, whatever lies beside the box."""
    rng = np.random.default_rng(61)
    vol = np.full((14, 17, 23), 255, np.uint8)
    box = ((3, 2, 4), (19, 13, 11))
    vol[4:11, 2:13, 3:19] = rng.integers(0, 200, (7, 11, 16), dtype=np.uint8)
    for v in (vol, (vol.astype(f32) / f32(255)).astype(f32)):
        _load(ctx, monkeypatch, v)
        dev = _dev_for(v)
        for src in (dict(level=100), dict(level=255), dict(bins=(100, 255))):
            for cap in (1, 0):
                want = _run_case(ctx, dev, "255 outside", v, src, cap, box)
            if src.get("level") == 255:
                assert want.summary == (0, 0, 0, 0) and _model(v, src, 1, box).summary == (0, 0, 0, 0)


@pytest.mark.gpu
def test_mesh_label_sources_and_compositions(ctx, monkeypatch):
    """VV_MESH_LABEL and VV_MESH_NONZERO on the model's labels; ctx.label -> ctx.surface(labels, label); ctx.morphology -> ctx.surface(labels), whose
    quad count is the face count of ctx.regions (rule 8 (b))."""
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    dev = _dev_for(vol)
    labels, sizes, stats = TL._want("r70_u8", (0, 78), 6)
    for cap in (1, 0):
        _run_case(ctx, dev, "labels", vol, dict(labels=labels, label=stats.largest_label), cap)
        _run_case(ctx, dev, "labels", vol, dict(labels=labels), cap)
        _run_case(ctx, dev, "labels", vol, dict(labels=labels, label=0), cap)             # the background as a set
        _run_case(ctx, dev, "labels", vol, dict(labels=labels, label=0xFFFFFFFF), cap)    # no such label: nothing
    box = ((3, 5, 1), (61, 33, 17))
    sub = TL._want("r70_u8", (0, 153), 6, box)[0]
    _run_case(ctx, dev, "labels in a box", vol, dict(labels=sub, label=int(sub.max())), 1, box)
    _run_case(ctx, dev, "labels in a box", vol, dict(labels=sub), 0, box)
    # composed with vv_label_volume
    got_l, _, got_stats = ctx.label((0, 78), 6, sizes=True, stats=True)
    TR._check_volume(got_l, labels, "labels for surface")
    mesh = ctx.surface(labels=got_l, label=got_stats.largest_label, normals=True)
    want = _model(vol, dict(labels=labels, label=stats.largest_label), 1)
    assert np.array_equal(mesh.vertices.view(np.uint32), np.stack([want.vertices[n] for n in "xyz"], axis=1).view(np.uint32)) and np.array_equal(mesh.quads, want.quads)
    assert mesh.normals.tobytes() == want.normals.tobytes() and MM.closed_and_oriented(mesh.quads) <= 4
    # composed with the morphology: rule 8 (b) through vv_region_table
    _load(ctx, monkeypatch, "aniso")
    aniso = _volume("aniso")
    opened = ctx.morphology(vv.MORPH_OPEN, 1.5, bins=(60, 255))
    mesh = ctx.surface(labels=opened)
    row = ctx.regions(opened, source=vv.REGION_NONZERO, max_regions=1)[0]
    assert len(mesh.quads) == int(row["faces"].sum()) > 0
    want = _model(aniso, dict(labels=opened), 1)
    assert np.array_equal(mesh.quads, want.quads) and np.array_equal(mesh.sites, want.vertices["site"])
    assert vv.mesh_area_volume(mesh)[1] > 0


@pytest.mark.gpu
def test_mesh_capacities_and_count_only(ctx, monkeypatch):
    """max_vertices and max_quads in {0, 1, K - 1, K, K + 7}, independently: index and the summary do not depend on them, the records beyond `written`
    keep the garbage; with and without normals and summary; a count-only call with NULL outputs gives the same summary."""
    _load(ctx, monkeypatch, "ramp")
    vol = _volume("ramp")
    dev = _dev_for(vol)
    src = dict(level=150)
    whole = _model(vol, src, 1)
    V, Q = whole.V, whole.Q
    k = 0
    for mv in (0, 1, V - 1, V, V + 7):
        for mq in (0, 1, Q - 1, Q, Q + 7):
            k += 1
            want = _run_case(ctx, dev, "capacities", vol, src, 1, max_vertices=mv, max_quads=mq, normals=k % 3 != 0, summary=k % 4 != 0, host=k % 5 == 0)
            assert want.summary == (V, Q, min(V, mv), min(Q, mq))
    for cap in (1, 0):
        want = _model(vol, src, cap)
        _, _, _, _, gs = dev.run(lambda ip, icap, vp, np_, qp, sp: ctx.surface_device(0, 0, summary_ptr=sp, cap=cap, **src), want.dims, 0, 0, (0, 0), index=False, what="count only")
        assert gs == (want.V, want.Q, 0, 0)
        st = vv.vv_mesh_summary()
        d = ctx._mesh(150, None, False, None, cap, None)
        assert ctx.lib.vv_surface_mesh(ctx.h, C.byref(d), None, None, 0, None, 0, None, None, 0, C.addressof(st), 0, None) == 0
        assert _summary_tuple(st) == (want.V, want.Q, 0, 0)
        assert ctx.lib.vv_surface_mesh(ctx.h, C.byref(d), None, None, 0, None, 0, None, None, 0, None, 0, None) == 0    # nothing to write at all


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["3", "1", "40"])
def test_mesh_chunk_cap_and_block_order(ctx, chunks, monkeypatch):
    """The chunk cap lowered: the 71 x 41 x 21 sites are 3 long chunks, one chunk, 40 chunks (several waves of a block share the work differently);
    each under VV_MESH_BLOCKS = 1, 8 and as the suite was started, and a second run gives the same bytes."""
    _load(ctx, monkeypatch, "r70_f32")
    vol = _volume("r70_f32")
    dev = _dev_for(vol)
    labels = TL._want("r70_f32", (0, 34), 18)[0]
    try:
        for blocks in ("1", "8", None):
            monkeypatch.setenv("VV_MESH_CHUNKS", chunks)
            if blocks is not None:
                monkeypatch.setenv("VV_MESH_BLOCKS", blocks)
            ctx.reread_env()
            for cap in (1, 0):
                _run_case(ctx, dev, f"chunks {chunks} blocks {blocks}", vol, dict(level=128), cap, host=False)
                _run_case(ctx, dev, f"chunks {chunks} blocks {blocks}", vol, dict(labels=labels), cap, host=False)
            first, second = ctx.surface(level=128, normals=True, return_index=True), ctx.surface(level=128, normals=True, return_index=True)
            for n in ("vertices", "sites", "quads", "normals", "index"):
                assert getattr(first, n).tobytes() == getattr(second, n).tobytes(), "a second run differs"
            monkeypatch.undo()
    finally:
        monkeypatch.undo()
        ctx.reread_env()


@pytest.mark.gpu
@VO.layout_sweep
def test_mesh_layouts(kind, nx, knobs, monkeypatch):
    """A re-pitched volume and the 64-bit addressing build, as test_regions.py sweeps them.  The volume holds no zero: with bins (0, 0) the mesh is
    empty unless padding is read as data."""
    with VO.layout_context(kind, nx, knobs, monkeypatch, LAYOUT_KNOBS, TF) as (c, vol):
        nz, ny, _ = vol.shape
        dev = _dev_for(vol)
        for src, box in ((dict(level=128), None), (dict(bins=(1, 100)), ((1, 0, 1), (nx - 1, ny, nz - 1))), (dict(level=40), ((0, 3, 2), (nx, 9, 8)))):
            for cap in (1, 0):
                assert _run_case(c, dev, f"layout {kind} {knobs}", vol, src, cap, box).V > 0
        assert _run_case(c, dev, f"layout {kind} {knobs}, no zero", vol, dict(bins=(0, 0)), 1).summary == (0, 0, 0, 0), "padding was read as data"
        labels = LM.label(vol, (1, 100), 6)[0]
        _run_case(c, dev, f"layout {kind} {knobs}, labels", vol, dict(labels=labels), 1)


@pytest.mark.gpu
def test_mesh_load_paths_and_streams(ctx, monkeypatch):
    """A volume that came from a device buffer and one promoted by the streamed upload; then label and mesh calls enqueued on one torch stream,
    synchronised by the stream alone."""
    import torch
    tdev = torch.device("cuda", 0)
    vol8 = _volume("u8:37x21x13")
    dev = _dev_for(vol8)
    for (what, loaded), cap in zip(VO.load_paths(ctx, monkeypatch, LAYOUT_KNOBS, vol8, TF), (1, 0)):
        _run_case(ctx, dev, what, loaded, dict(level=128), cap)
    _run_case(ctx, dev, what, loaded, dict(bins=(0, 100)), 1)
    # enqueue only: count, then the full call, behind the labels they read
    _load(ctx, monkeypatch, "r70_u8")
    vol = _volume("r70_u8")
    conn, bins = 6, (0, 153)
    want_l = TL._want("r70_u8", bins, conn)[0]
    want = _model(vol, dict(labels=want_l), 1)
    n, sites = want_l.size, int(np.prod(want.dims))
    ts = torch.cuda.Stream(device=tdev)
    lab_t = torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    idx_t = torch.full((sites,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=tdev)
    ver_t, nor_t = (torch.full((16 * (want.V + 1),), GARBAGE, dtype=torch.uint8, device=tdev) for _ in range(2))
    qua_t = torch.full((16 * (want.Q + 1),), GARBAGE, dtype=torch.uint8, device=tdev)
    sum_t = torch.full((8,), -1, dtype=torch.int64, device=tdev)
    assert ver_t.data_ptr() % 16 == 0 and nor_t.data_ptr() % 16 == 0 and qua_t.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    with torch.cuda.stream(ts):
        h = vv.stream_handle(ts)
        ctx.label_device(lab_t.data_ptr(), n * 4, bins, conn, stream=h)
        assert ctx.surface_device(0, 0, summary_ptr=sum_t.data_ptr(), labels_ptr=lab_t.data_ptr(), stream=h) == want.dims
        assert ctx.surface_device(idx_t.data_ptr(), sites * 4, ver_t.data_ptr(), want.V + 1, qua_t.data_ptr(), want.Q + 1, normals_ptr=nor_t.data_ptr(),
                                  summary_ptr=sum_t.data_ptr() + 32, labels_ptr=lab_t.data_ptr(), stream=h) == want.dims
    ts.synchronize()
    _check_volume(idx_t.cpu().numpy().view(np.uint32).reshape(want.index.shape), want.index, "enqueue-only index")
    raw_v, raw_n, raw_q = ver_t.cpu().numpy(), nor_t.cpu().numpy(), qua_t.cpu().numpy()
    _check_records(raw_v[:16 * want.V].view(vv.MESH_VERTEX_DTYPE), want.vertices, "enqueue-only vertices")
    _check_records(raw_n[:16 * want.V].view(vv.MESH_NORMAL_DTYPE), want.normals, "enqueue-only normals")
    assert np.array_equal(raw_q[:16 * want.Q].view(np.uint32).reshape(-1, 4), want.quads)
    assert (raw_v[16 * want.V:] == GARBAGE).all() and (raw_n[16 * want.V:] == GARBAGE).all() and (raw_q[16 * want.Q:] == GARBAGE).all()
    s = sum_t.cpu().numpy()
    assert tuple(int(v) for v in s[:4]) == (want.V, want.Q, 0, 0) and tuple(int(v) for v in s[4:]) == (want.V, want.Q, want.V, want.Q)


@pytest.mark.gpu
def test_mesh_errors_and_state(ctx, monkeypatch):
    import torch
    tdev = torch.device("cuda", 0)
    lib, hnd = ctx.lib, ctx.h

    def mk(lo=(0, 0, 0), hi=(0, 0, 0), source=0, level=128, bins=(0, 0), label=0, cap=1, max_vertices=8, max_quads=8):
        d = vv.vv_mesh()
        d.box_lo[:], d.box_hi[:] = lo, hi
        d.source, d.level, d.bin_lo, d.bin_hi, d.label, d.cap, d.max_vertices, d.max_quads = source, level, bins[0], bins[1], label, cap, max_vertices, max_quads
        return d

    with vv.Context(0) as empty:                                    # before a load: behind the NULL checks, before a bad descriptor
        out = np.full(4096, GARBAGE, np.uint8)
        p = out.ctypes.data
        assert lib.vv_surface_mesh(empty.h, C.byref(mk(source=9)), None, p, 1024, p + 1024, 128, None, p + 2048, 128, None, 0, None) == ERR_NO_VOLUME
        assert lib.vv_surface_mesh(empty.h, None, None, p, 1024, p + 1024, 128, None, p + 2048, 128, None, 0, None) == ERR_INVALID
        m = (C.c_int * 3)(7, 7, 7)
        assert lib.vv_mesh_dims(empty.h, C.byref(mk()), C.byref(m)) == ERR_NO_VOLUME and lib.vv_mesh_dims(empty.h, None, C.byref(m)) == ERR_INVALID
        assert (out == GARBAGE).all() and tuple(m) == (7, 7, 7)
        with pytest.raises(vv.VolvizError) as e:
            empty.surface(level=3)
        assert e.value.code == ERR_NO_VOLUME
    _load(ctx, monkeypatch, "aniso")
    vol = _volume("aniso")
    nz, ny, nx = vol.shape
    n = vol.size
    sites = (nx + 1) * (ny + 1) * (nz + 1)
    before = VO.Untouched(ctx)
    assert ctx.mesh_dims() == (nx + 1, ny + 1, nz + 1) and ctx.mesh_dims(False) == (nx - 1, ny - 1, nz - 1) and ctx.mesh_dims(False, ((1, 2, 3), (2, 5, 9))) == (0, 2, 5)
    m = (C.c_int * 3)(7, 7, 7)
    assert lib.vv_mesh_dims(hnd, C.byref(mk(cap=2)), C.byref(m)) == ERR_INVALID and lib.vv_mesh_dims(hnd, C.byref(mk(lo=(1, 0, 0))), C.byref(m)) == ERR_INVALID
    assert lib.vv_mesh_dims(hnd, C.byref(mk()), None) == ERR_INVALID and tuple(m) == (7, 7, 7)

    # one buffer each on the host and on the device: labels | index | vertices (8) | normals (8) | quads (8) | summary, GUARD apart
    L0 = 0
    I0 = _align(n * 4 + GUARD, 16)
    V0 = _align(I0 + sites * 4 + GUARD, 16)
    N0, Q0 = V0 + 128 + GUARD, V0 + 2 * (128 + GUARD)
    S0 = Q0 + 128 + GUARD
    total = S0 + 32 + GUARD
    host = np.full(total + 16, GARBAGE, np.uint8)
    raw = torch.full((total,), GARBAGE, dtype=torch.uint8, device=tdev)
    torch.cuda.synchronize()
    hp, dp = host.ctypes.data, raw.data_ptr()
    hp += -hp % 16
    host = host[hp - host.ctypes.data:][:total]
    assert dp % 16 == 0 and hp % 16 == 0 and host.ctypes.data == hp

    def call(p, dev, d, labels=None, index=I0, icap=None, vertices=V0, vcap=128, normals=N0, quads=Q0, qcap=128, summary=S0):
        f = lambda off: None if off is None else p + off
        return lib.vv_surface_mesh(hnd, C.byref(d) if d is not None else None, f(labels), f(index), sites * 4 if icap is None else icap, f(vertices), vcap, f(normals),
                                   f(quads), qcap, f(summary), dev, None)

    def both(d, **kw):
        rc = [call(p, dev, d, **kw) for p, dev in ((hp, 0), (dp, 1))]
        assert rc[0] == rc[1], rc
        return rc[0]

    def said(word):
        return word in lib.vv_last_error(hnd).decode()

    good = mk()
    assert lib.vv_surface_mesh(None, C.byref(good), None, hp + I0, sites * 4, hp + V0, 128, None, hp + Q0, 128, None, 0, None) == ERR_INVALID
    assert both(None) == ERR_INVALID
    bad_boxes = (((-1, 0, 0), (nx, ny, nz)), ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny, nz + 1)), ((3, 0, 0), (3, ny, nz)), ((0, 5, 0), (nx, 4, nz)), ((1, 0, 0), (0, 0, 0)))
    for lo, hi in bad_boxes:
        assert both(mk(lo, hi)) == ERR_INVALID and said("box"), (lo, hi)
    for source in (-1, 4, 9):
        assert both(mk(source=source)) == ERR_INVALID and said("source")
    for level in (0, -1, 256):
        assert both(mk(level=level)) == ERR_INVALID and said("level")
        assert both(mk(source=vv.MESH_BINS, level=level), icap=0, index=None, vertices=None, quads=None) == ERR_INVALID and said("index is NULL")    # (ignored there)
    for bins in ((-1, 5), (6, 5), (0, 256)):
        assert both(mk(source=vv.MESH_BINS, bins=bins)) == ERR_INVALID and said("bins")
    assert both(good, labels=L0) == ERR_INVALID and said("labels must") and both(mk(source=vv.MESH_BINS), labels=L0) == ERR_INVALID and said("labels must")
    for source in (vv.MESH_LABEL, vv.MESH_NONZERO):
        assert both(mk(source=source, level=0)) == ERR_INVALID and said("labels must")
    for cap in (-1, 2):
        assert both(mk(cap=cap)) == ERR_INVALID and said("cap")
    assert both(good, index=None) == ERR_INVALID and said("index is NULL")
    assert both(mk(max_quads=0), index=None) == ERR_INVALID and said("index is NULL") and both(mk(max_vertices=0), index=None) == ERR_INVALID and said("index is NULL")
    assert both(good, vertices=None) == ERR_INVALID and said("vertices is NULL") and both(good, quads=None) == ERR_INVALID and said("quads is NULL")
    # the order, on the device: each step mends what the step before it was refused for
    steps = ((dict(), dict(), "box"), (dict(lo=(0, 0, 0)), dict(), "source"), (dict(lo=(0, 0, 0), source=0), dict(), "level"),
             (dict(lo=(0, 0, 0), source=1), dict(), "bins"), (dict(lo=(0, 0, 0), source=1, bins=(3, 9)), dict(), "labels must"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9)), dict(labels=None), "cap"), (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None), "index is NULL"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0 + 2), "vertices is NULL"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0 + 2, vertices=V0 + 4), "quads is NULL"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0 + 2, vertices=V0 + 4, quads=V0 + 8), "index capacity"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0 + 2, vertices=V0 + 4, quads=V0 + 8, icap=sites * 4), "vertices capacity"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0 + 2, vertices=V0 + 4, quads=V0 + 8, icap=sites * 4, vcap=128), "quads capacity"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0 + 2, vertices=V0 + 4, quads=V0 + 8, icap=sites * 4, vcap=128, qcap=128), "aligned"),
             (dict(lo=(0, 0, 0), source=1, bins=(3, 9), cap=0), dict(labels=None, index=I0, vertices=V0, quads=V0 + 16, icap=sites * 4, vcap=128, qcap=128, normals=N0, summary=S0), "overlaps"))
    for fix, args, word in steps:
        kw = dict(lo=(1, 0, 0), hi=(0, 0, 0), source=5, level=0, bins=(9, 3), cap=3)
        kw.update(fix)
        a = dict(labels=L0 + 2, index=None, vertices=None, quads=None, icap=(nx - 1) * (ny - 1) * (nz - 1) * 4 - 1, vcap=127, qcap=127, normals=N0 + 8, summary=S0 + 4)
        a.update(args)
        assert call(dp, 1, mk(**kw), **a) == ERR_INVALID and said(word), (word, lib.vv_last_error(hnd))
    # capacities on both paths: one byte short, 16 * max formed in 64 bits
    assert both(good, icap=sites * 4 - 1) == ERR_INVALID and said("index capacity")
    assert both(good, vcap=127) == ERR_INVALID and said("vertices capacity") and both(good, qcap=127) == ERR_INVALID and said("quads capacity")
    assert both(mk(max_vertices=0xFFFFFFFF), vcap=(16 * 0xFFFFFFFF) % (1 << 32)) == ERR_INVALID and said("vertices capacity")
    assert both(mk(max_quads=0xFFFFFFFF), qcap=(16 * 0xFFFFFFFF) % (1 << 32)) == ERR_INVALID and said("quads capacity")
    # alignment (device only)
    for off in (1, 2, 3):
        assert call(dp, 1, mk(source=vv.MESH_NONZERO), labels=L0 + off) == ERR_INVALID and said("aligned")
        assert call(dp, 1, good, index=I0 + off, icap=sites * 4 + GUARD) == ERR_INVALID and said("aligned")
    for off in (1, 4, 8):
        assert call(dp, 1, good, vertices=V0 + off) == ERR_INVALID and said("aligned")
        assert call(dp, 1, good, normals=N0 + off) == ERR_INVALID and said("aligned")
        assert call(dp, 1, good, quads=Q0 + off) == ERR_INVALID and said("aligned")
    for off in (1, 4, 7):
        assert call(dp, 1, good, summary=S0 + off) == ERR_INVALID and said("aligned")
    # overlaps (device only): every output with the labels and with every other output
    nonzero = mk(source=vv.MESH_NONZERO)
    assert call(dp, 1, nonzero, labels=L0, index=L0 + n * 4 - 4) == ERR_INVALID and said("index overlaps")
    assert call(dp, 1, nonzero, labels=L0, vertices=L0 + 16) == ERR_INVALID and said("vertices overlaps")
    assert call(dp, 1, nonzero, labels=L0, quads=L0 + 32) == ERR_INVALID and said("quads overlaps")
    assert call(dp, 1, nonzero, labels=L0, normals=L0 + 64) == ERR_INVALID and said("normals overlaps")
    assert call(dp, 1, nonzero, labels=L0, summary=L0 + 8) == ERR_INVALID and said("summary overlaps")
    assert call(dp, 1, good, vertices=I0 + 16) == ERR_INVALID and said("index overlaps")
    assert call(dp, 1, good, normals=V0 + 112) == ERR_INVALID and said("vertices overlaps")
    assert call(dp, 1, good, quads=N0 + 16) == ERR_INVALID and said("normals overlaps")
    assert call(dp, 1, good, summary=Q0 + 120) == ERR_INVALID and said("quads overlaps")
    assert call(dp, 1, good, summary=I0 + 8) == ERR_INVALID and said("index overlaps")
    assert (host == GARBAGE).all() and bool((raw == GARBAGE).all()), "a refused call writes nothing"
    # exactly the needed capacities are enough, on both paths
    labels = TL._want("aniso", (60, 100), 18)[0]
    want = _model(vol, dict(labels=labels), 1, max_vertices=8, max_quads=8)
    host[L0:L0 + n * 4] = labels.view(np.uint8).ravel()
    raw.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    assert both(nonzero, labels=L0) == 0
    for name, got in (("host", host), ("device", raw.cpu().numpy())):
        _check_volume(got[I0:I0 + sites * 4].view(np.uint32).reshape(want.index.shape), want.index, name + " index, exact capacity")
        _check_records(got[V0:V0 + 128].view(vv.MESH_VERTEX_DTYPE), want.vertices, name + " vertices, exact capacity")
        _check_records(got[N0:N0 + 128].view(vv.MESH_NORMAL_DTYPE), want.normals, name + " normals, exact capacity")
        assert np.array_equal(got[Q0:Q0 + 128].view(np.uint32).reshape(-1, 4), want.quads)
        assert _summary_tuple(vv.MeshSummary.from_bytes(got[S0:S0 + 32])) == want.summary and want.summary[2:] == (8, 8)
        keep = np.ones(total, bool)
        for o, m in ((L0, n * 4), (I0, sites * 4), (V0, 128), (N0, 128), (Q0, 128), (S0, 32)):
            keep[o:o + m] = False
        assert (got[keep] == GARBAGE).all(), name

    # a device call allocates no device memory: the device's free bytes stay what they were
    def calls():
        for source in (0, 1, 2, 3):
            assert call(dp, 1, mk(source=source, bins=(0, 99)), labels=L0 if source >= 2 else None) == 0
        assert call(dp, 1, mk(max_vertices=0, max_quads=0), index=None, vertices=None, normals=None, quads=None) == 0

    VO.free_memory_unchanged(calls)
    # the context is still usable and untouched: volume, layout copies, residency, scratch, frame time, histogram, frames
    before.check()
