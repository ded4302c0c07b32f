"""developer tool (1 GPU): time of vv_surface_mesh (index, vertices, normals, quads and summary into exactly sized device buffers, cap = 1) on an n^3 u8
volume: the brain phantom at level 255 (no surface: what the walk alone costs), at the levels of its shells, and the noise volume at a high level (a
fragmented surface through about a tenth of the cells) and, where the records fit in --max-gb, at its median (a surface through every cell).

  - the count-only call (two launches), the whole call, and its launches by difference: VV_MESH_PHASES = 1, 2, 3 stops the call behind the count, scan
    and vertices launch (the rest, the quads launch, is the difference to the whole call);
  - vv_derive_volume at factor 1 of the same volume (the streaming yardstick), in the same run;
  - GB/s = the call's compulsory bytes / time: the volume read once in each of the launches 1, 3 and 4 (3 x 1 byte per voxel), `index` written once and read
    once (2 x 4 bytes per site), 32 bytes per vertex (record and normal) and 16 per quad; the corner rows a wave reads again (three of four) and the three
    neighbour index words of a quad are re-reads that the caches may serve and are not counted;
  - the mesh is checked where it is cheap: the summary of the count-only call equals that of the full call, every quad names vertices below V, and on the
    binary input the quad count equals the face count of vv_region_table (the header's rule 8 (b)).

Every figure is the median over the repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library.
    python tools/time_mesh.py [--n 1024] [--iters 2] [--repeats 3] [--max-gb 64] [--out FILE]"""
import argparse, os, statistics, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=2, help="calls per timing")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--max-gb", type=float, default=64.0, help="an input whose records need more than this is only counted")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.iters >= 1 and args.repeats >= 1


def emit(s):
    print(s, flush=True)
    if args.out:                                                # line by line: a run that is cut short keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")


dev = torch.device("cuda", 0)
ctx = vv.Context(0)
n = args.n
vox = n ** 3
stream = vv.stream_handle(torch.cuda.current_stream())


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                    # us per call of fn


def spread(v):
    return f"{statistics.median(v):10.1f} [{min(v):10.1f} .. {max(v):10.1f}]"


def phases(k):
    if k:
        os.environ["VV_MESH_PHASES"] = str(k)
    else:
        os.environ.pop("VV_MESH_PHASES", None)
    ctx.reread_env()


def summary_of(t):
    return vv.MeshSummary.from_bytes(t.cpu().numpy().tobytes())


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 u8, cap 1, {args.iters} calls per timing, {args.repeats} repeats (median [min .. max]); index, vertices, normals, quads and summary into device buffers, enqueue-only")
emit("GB/s = (3 bytes per voxel + 8 per site + 32 per vertex + 16 per quad) / time of the whole call; derive 1x: (1 + 1 bytes per voxel) / time")
tf = vv.transfer_preset(vv.TF_HEAD)
vol = torch.empty(vox, dtype=torch.uint8, device=dev)
out = torch.empty(vox, dtype=torch.uint8, device=dev)
summary = torch.empty(4, dtype=torch.int64, device=dev)
mx, my, mz = n + 1, n + 1, n + 1
sites = mx * my * mz
index = torch.empty(sites, dtype=torch.int32, device=dev)
whole_us = {}

for name, sources in (("brain", (dict(level=255), dict(level=100), dict(level=61), dict(bins=(80, 120)))), ("noise", (dict(level=250), dict(level=128)))):
    if name == "brain":
        ctx.generate_default_brain_device(vol.data_ptr(), n, n, n)
    else:
        ctx.generate_noise_device(vol.data_ptr(), n, n, n, 3)
    torch.cuda.synchronize()
    ctx.load_volume_device(vol.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
    torch.cuda.synchronize()
    derive = lambda: ctx.derive_device(out.data_ptr(), out.numel(), None, 1, vv.REDUCE_MEAN, vv.VOXEL_U8, stream=stream)
    for src in sources:
        what = f"{name} " + ("level %3d" % src["level"] if "level" in src else "bins %d..%d" % src["bins"])
        phases(0)
        count = lambda: ctx.surface_device(0, 0, summary_ptr=summary.data_ptr(), stream=stream, **src)
        assert count() == (mx, my, mz)
        torch.cuda.synchronize()
        sm = summary_of(summary)
        V, Q = sm.vertices, sm.quads
        need = (32 * V + 16 * Q) / 2 ** 30
        t_count = [timed(count, args.iters) for _ in range(args.repeats)]
        if need > args.max_gb:
            emit(f"{what}: vertices {V} quads {Q}: the records need {need:.1f} GiB, above --max-gb; count-only call {spread(t_count)} us")
            continue
        vert = torch.empty(16 * max(V, 1), dtype=torch.uint8, device=dev)
        norm = torch.empty(16 * max(V, 1), dtype=torch.uint8, device=dev)
        quad = torch.empty(16 * max(Q, 1), dtype=torch.uint8, device=dev)
        mesh = lambda: ctx.surface_device(index.data_ptr(), sites * 4, vert.data_ptr() if V else 0, V, quad.data_ptr() if Q else 0, Q,
                                          normals_ptr=norm.data_ptr() if V else 0, summary_ptr=summary.data_ptr(), stream=stream, **src)
        mesh(); derive()
        torch.cuda.synchronize()
        full = summary_of(summary)
        assert (full.vertices, full.quads, full.written_vertices, full.written_quads) == (V, Q, V, Q), (full, sm)
        if Q:
            part = quad[:16 * min(Q, 1 << 24)].cpu().numpy().view(np.uint32)
            assert int(part.max()) < V
        if "bins" in src:                                       # rule 8 (b): the faces of the same set as one region
            labels = torch.empty(vox, dtype=torch.int32, device=dev)
            table = torch.empty(vv.REGION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            ctx.distance_device(labels.data_ptr(), vox * 4, bins=src["bins"], within=0, stream=stream)
            ctx.regions_device(labels.data_ptr(), index.data_ptr(), vox * 4, table.data_ptr(), 1, source=vv.REGION_NONZERO, stream=stream)
            torch.cuda.synchronize()
            faces = int(table.cpu().numpy().view(vv.REGION_DTYPE)[0]["faces"].sum())
            assert faces == Q, (faces, Q)
            del labels, table
        t = {k: [] for k in (1, 2, 3, 0, "derive")}
        for _ in range(args.repeats):                           # alternated
            for k in (1, 2, 3, 0):
                phases(k)
                t[k].append(timed(mesh, args.iters))
            t["derive"].append(timed(derive, args.iters))
        phases(0)
        med = {k: statistics.median(v) for k, v in t.items()}
        nbytes = 3 * vox + 8 * sites + 32 * V + 16 * Q
        whole_us[what] = med[0]
        emit(f"{what}: vertices {V} quads {Q} ({need:.2f} GiB of records)")
        emit(f"    whole call {spread(t[0])} us  {nbytes / med[0] / 1e3:7.1f} GB/s   count {med[1]:9.1f}  scan {med[2] - med[1]:9.1f}  vertices {med[3] - med[2]:9.1f}  "
             f"quads {med[0] - med[3]:9.1f} us   (cumulative: {spread(t[1])} / {spread(t[2])} / {spread(t[3])})")
        emit(f"    count-only call {spread(t_count)} us   derive 1x {spread(t['derive'])} us  {2 * vox / med['derive'] / 1e3:7.1f} GB/s, mesh / derive {med[0] / med['derive']:6.2f}")
        del vert, norm, quad

if len(whole_us) >= 2:
    floor = min(whole_us.values())
    for k, v in whole_us.items():
        emit(f"ratio to the fastest input: {k}: {v / floor:6.2f}")
