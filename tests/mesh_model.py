"""The surface-mesh contract of include/volviz.h (vv_surface_mesh, rules 1-7) in numpy.

A volume is an array [nz, ny, nx] of uint8 or float32, x fastest; a box is ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive, None = the whole
volume.  Nothing here comes from the library: the field comes through hist_model.bins / label_model.foreground, every float is kept in binary32 at
every step (one conversion per integer, one division per crossing, one addition per active edge in the order e = 0..11, one division and one addition
per coordinate), and the outputs are in the canonical order of the header: vertices by site number, quads by (site number, axis).  surface_mesh is
vectorised over the sites with the 12 edges in a Python loop; surface_mesh_loop is the same contract restated cell by cell in plain Python, as naively
as possible, and holds the vectorised form on tiny volumes (test_mesh.py).  Results are compared exactly, floats as bit patterns."""
from types import SimpleNamespace

import numpy as np

import hist_model as HM
import label_model as LM

f32 = np.float32
INDEX, BINS, LABEL, NONZERO = 0, 1, 2, 3
VERTEX_DTYPE = np.dtype({"names": ["x", "y", "z", "site"], "formats": ["<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12], "itemsize": 16})
NORMAL_DTYPE = np.dtype({"names": ["g", "edges"], "formats": [("<i4", 3), "<u4"], "offsets": [0, 12], "itemsize": 16})


def field(vol, source, level=None, bins=None, labels=None, label=None, box=None):
    """Rule 1: (g, level) of the box: g int64 [bz, by, bx] in 0..255."""
    if source == INDEX:
        assert 1 <= level <= 255
        return HM.bins(HM.crop(np.asarray(vol), box)).astype(np.int64), int(level)
    if source == BINS:
        return LM.foreground(vol, bins, box).astype(np.int64), 1
    labels = np.asarray(labels, np.uint32)
    assert labels.shape == HM.crop(np.asarray(vol), box).shape
    return ((labels == np.uint32(label)) if source == LABEL else (labels != 0)).astype(np.int64), 1


def dims(shape, cap):
    """Rule 2: m = (m_x, m_y, m_z) of a box of `shape` = (bz, by, bx)."""
    return tuple(int(b) - 1 + 2 * int(cap) for b in shape[::-1])


def edge(e):
    """Rule 3: (a, p, q) of edge e: its axis and the (dx, dy, dz) of its two ends."""
    a, db, dc = e // 4, e & 1, (e >> 1) & 1
    p = [0, 0, 0]
    p[(a + 1) % 3], p[(a + 2) % 3] = db, dc
    q = list(p)
    q[a] = 1
    return a, tuple(p), tuple(q)


def _result(m, index, vertices, normals, quads, max_vertices, max_quads):
    V, Q = len(vertices), len(quads)
    wv, wq = V if max_vertices is None else min(V, max_vertices), Q if max_quads is None else min(Q, max_quads)
    return SimpleNamespace(dims=m, index=index, vertices=vertices[:wv], normals=normals[:wv], quads=quads[:wq], V=V, Q=Q,
                           summary=(V, Q, wv, wq))


def surface_mesh(g, level, cap, lo=(0, 0, 0), max_vertices=None, max_quads=None):
    """Rules 2-7 for a field g [bz, by, bx]: index uint32 [m_z, m_y, m_x], vertices (VERTEX_DTYPE), normals (NORMAL_DTYPE), quads uint32 [Q, 4], the
    counts V and Q and the summary (vertices, quads, written_vertices, written_quads).  lo: the box's origin in the volume (x, y, z)."""
    g = np.asarray(g, np.int64)
    cap = int(cap)
    m = dims(g.shape, cap)
    mx, my, mz = m
    if min(m) <= 0:
        return _result(m, np.zeros((max(mz, 0), max(my, 0), max(mx, 0)), np.uint32), np.zeros(0, VERTEX_DTYPE), np.zeros(0, NORMAL_DTYPE),
                       np.zeros((0, 4), np.uint32), max_vertices, max_quads)
    G = np.pad(g, 1) if cap else g                                  # the virtual voxels: g = 0
    corner = lambda d: G[d[2]:d[2] + mz, d[1]:d[1] + my, d[0]:d[0] + mx].ravel()
    inside = lambda d: corner(d) >= level
    all_d = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    n_in = sum(inside(d).astype(np.int64) for d in all_d)
    active = (n_in > 0) & (n_in < 8)
    sites = mx * my * mz
    V = int(active.sum())
    index = np.zeros(sites, np.uint32)
    index[active] = np.arange(1, V + 1, dtype=np.uint32)
    # vertices
    S = [np.zeros(sites, f32) for _ in range(3)]
    n = np.zeros(sites, np.int64)
    mask = np.zeros(sites, np.uint32)
    for e in range(12):
        a, p, q = edge(e)
        gp, gq = corner(p), corner(q)
        act = (gp >= level) != (gq >= level)
        num, den = (2 * level - 1 - 2 * gp).astype(f32), np.where(act, 2 * (gq - gp), 1).astype(f32)
        t = num / den
        assert t.dtype == f32 and ((t[act] > 0) & (t[act] < 1)).all()
        for k in range(3):
            term = t if k == a else np.full(sites, f32(p[k]), f32)
            S[k] = np.where(act, S[k] + term, S[k])
            assert S[k].dtype == f32
        n += act
        mask |= act.astype(np.uint32) << np.uint32(e)
    assert np.array_equal(n > 0, active)
    j = np.flatnonzero(active)
    s = (j % mx, (j // mx) % my, j // (mx * my))
    vertices = np.zeros(V, VERTEX_DTYPE)
    for k, name in enumerate("xyz"):
        base = (np.int64(lo[k]) + s[k] - cap).astype(f32)
        vertices[name] = base + S[k][j] / n[j].astype(f32)
    vertices["site"] = j
    normals = np.zeros(V, NORMAL_DTYPE)
    for k in range(3):
        normals["g"][:, k] = sum((corner(d) if d[k] == 0 else -corner(d)) for d in all_d)[j]
    normals["edges"] = mask[j]
    # quads
    sx, sy, sz = np.arange(sites) % mx, (np.arange(sites) // mx) % my, np.arange(sites) // (mx * my)
    pos, stride = (sx, sy, sz), (1, mx, mx * my)
    emit = np.zeros((sites, 3), bool)
    p_in = np.zeros((sites, 3), bool)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        _, p, q = edge(4 * a + 3)
        assert q == (1, 1, 1)
        p_in[:, a] = inside(p)
        emit[:, a] = (p_in[:, a] != inside(q)) & (pos[b] + 1 < m[b]) & (pos[c] + 1 < m[c])
    qj, qa = np.nonzero(emit)                                       # row-major: ascending (j, a)
    quads = np.zeros((len(qj), 4), np.uint32)
    if len(qj):
        sb, sc = np.array(stride)[(qa + 1) % 3], np.array(stride)[(qa + 2) % 3]
        c0, c1, c2, c3 = qj, qj + sb, qj + sb + sc, qj + sc
        assert index[c0].all() and index[c1].all() and index[c2].all() and index[c3].all()
        flip = ~p_in[qj, qa]
        quads[:, 0] = index[c0] - 1
        quads[:, 1] = np.where(flip, index[c3], index[c1]) - 1
        quads[:, 2] = index[c2] - 1
        quads[:, 3] = np.where(flip, index[c1], index[c3]) - 1
    return _result(m, index.reshape(mz, my, mx), vertices, normals, quads, max_vertices, max_quads)


def surface_mesh_loop(g, level, cap, lo=(0, 0, 0)):
    """The same contract, one cell at a time."""
    g = np.asarray(g)
    bz, by, bx = g.shape
    mx, my, mz = bx - 1 + 2 * cap, by - 1 + 2 * cap, bz - 1 + 2 * cap
    m = (mx, my, mz)

    def value(x, y, z):                                             # box voxel (x, y, z), virtual ones included
        return int(g[z, y, x]) if 0 <= x < bx and 0 <= y < by and 0 <= z < bz else 0

    index, vertices, normals = {}, [], []
    for sz in range(mz):
        for sy in range(my):
            for sx in range(mx):
                s = (sx, sy, sz)
                val = {d: value(sx - cap + d[0], sy - cap + d[1], sz - cap + d[2]) for d in [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]}
                S, n, mask = [f32(0), f32(0), f32(0)], 0, 0
                for e in range(12):
                    a, p, q = edge(e)
                    if (val[p] >= level) == (val[q] >= level):
                        continue
                    t = f32(2 * level - 1 - 2 * val[p]) / f32(2 * (val[q] - val[p]))
                    for k in range(3):
                        S[k] = f32(S[k] + (t if k == a else f32(p[k])))
                    n += 1
                    mask |= 1 << e
                if not n:
                    continue
                jj = (sz * my + sy) * mx + sx
                index[jj] = len(vertices)
                vertices.append(tuple(f32(f32(lo[k] + s[k] - cap) + f32(S[k] / f32(n))) for k in range(3)) + (jj,))
                normals.append(([sum(v if d[k] == 0 else -v for d, v in val.items()) for k in range(3)], mask))
    quads = []
    for sz in range(mz):
        for sy in range(my):
            for sx in range(mx):
                s = [sx, sy, sz]
                for a in range(3):
                    b, c = (a + 1) % 3, (a + 2) % 3
                    if not (s[b] + 1 < m[b] and s[c] + 1 < m[c]):
                        continue
                    hi = [sx - cap + 1, sy - cap + 1, sz - cap + 1]
                    low = list(hi)
                    low[a] -= 1
                    p_in, q_in = value(*low) >= level, value(*hi) >= level
                    if p_in == q_in:
                        continue
                    number = lambda t: index[(t[2] * my + t[1]) * mx + t[0]]
                    step = lambda t, k: [t[i] + (1 if i == k else 0) for i in range(3)]
                    c0, c1, c2, c3 = s, step(s, b), step(step(s, b), c), step(s, c)
                    quads.append([number(t) for t in ((c0, c1, c2, c3) if p_in else (c0, c3, c2, c1))])
    idx = np.zeros(max(mx, 0) * max(my, 0) * max(mz, 0), np.uint32)
    for jj, k in index.items():
        idx[jj] = k + 1
    va = np.zeros(len(vertices), VERTEX_DTYPE)
    na = np.zeros(len(vertices), NORMAL_DTYPE)
    for k, (v, nm) in enumerate(zip(vertices, normals)):
        va[k] = v
        na[k]["g"], na[k]["edges"] = nm
    return _result(m, idx.reshape(max(mz, 0), max(my, 0), max(mx, 0)), va, na, np.array(quads, np.uint32).reshape(-1, 4), None, None)


def directed_edges(quads):
    """[4 Q, 2] the directed edges (u, v) of the quads, in record order."""
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    return np.stack([q, np.roll(q, -1, axis=1)], axis=2).reshape(-1, 2)


def closed_and_oriented(quads):
    """Rule 8 (a): every directed edge occurs as often as its reverse; returns the largest use count of an undirected edge."""
    d = directed_edges(quads)
    if not len(d):
        return 0
    big = int(d.max()) + 1
    fwd = np.sort(d[:, 0] * big + d[:, 1])
    rev = np.sort(d[:, 1] * big + d[:, 0])
    assert np.array_equal(fwd, rev), "a directed edge has no partner"
    und = np.minimum(d[:, 0], d[:, 1]) * big + np.maximum(d[:, 0], d[:, 1])
    return int(np.unique(und, return_counts=True)[1].max())


def boundary_faces(inside):
    """Rule 8 (b): the voxel faces between an inside voxel and an outside or non-existent one."""
    pad = np.pad(np.asarray(inside, bool), 1)
    return int(sum((pad != np.roll(pad, 1, axis=a)).sum() for a in range(3)))
