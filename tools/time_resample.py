"""developer tool (1 GPU): time of vv_resample_volume writing into a device buffer, against three baselines:
  - vv_derive_volume at factor 1 of a box with the output's extents into the same type: a dense read and a dense write of the same number of
    voxels, the streaming floor of this library for the output's bytes;
  - torch.nn.functional.grid_sample (bilinear, align_corners=False, zeros outside) on a dense float tensor of the same voxels with the same
    affine grid; the grid itself (F.affine_grid, 12 bytes per output voxel) is made outside the timing, the u8 volume's conversion to float too;
    NEAREST is compared with mode="nearest";
  - the streaming read rate tools/ubench/hbm_lines.hip reports on the same machine (run as a child process under its own time limit when its
    binary is built: hipcc -O3 --offload-arch=gfx950 -o tools/ubench/bin/hbm_lines tools/ubench/hbm_lines.hip).

Cases, for an n^3 noise volume as f32 and as u8 with out_type = the volume's type (re-pitched by vv_load_volume_device): the identity at n^3; 30
degrees about z, about x, and a compound rotation; a 2x zoom-in to n^3; n^3 -> (5 n / 8)^3 (1024 -> 640); the NEAREST identity.  Resample call
and baselines run in one process and alternate; every figure is the median over the repeats with their range, device events around --iters
calls, enqueue only.  VV_LIB selects another build of the library; VV_RESAMPLE_BLOCKS caps the grid.
    python tools/time_resample.py [--n 1024] [--iters 10] [--base-iters 2] [--repeats 3] [--voxels f32,u8] [--no-baseline] [--out FILE]"""
import argparse, math, os, re, statistics, subprocess, sys
import torch
import torch.nn.functional as F
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=10, help="resample / derive calls per timing")
ap.add_argument("--base-iters", type=int, default=2, help="torch baseline calls per timing")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--voxels", default="f32,u8")
ap.add_argument("--no-baseline", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.iters >= 1 and args.base_iters >= 1 and args.repeats >= 1


def emit(s):
    print(s, flush=True)
    if args.out:                                                # line by line: a run that is cut short keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")


# the streaming yardstick first, in a process of its own, before this one holds any memory
stream_gbs = None
ubench = os.path.join(HERE, "ubench", "bin", "hbm_lines")
if os.path.exists(ubench):
    txt = subprocess.run(["timeout", "-k", "10", "120", ubench], capture_output=True, text=True, check=True).stdout
    m = re.search(r"sequential streaming\s*:\s*[\d.]+ ms\s+([\d.]+) GB/s", txt)
    stream_gbs = float(m.group(1)) if m else None

dev = torch.device("cuda", 0)
ctx = vv.Context(0)
n = args.n
stream = vv.stream_handle(torch.cuda.current_stream())


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                    # us per call of fn


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):9.1f} .. {max(v):9.1f}]"


def measure(label, voxels, size, ours, derive, base):
    fns = [(ours, args.iters), (derive, args.iters)] + ([(base, args.base_iters)] if base else [])
    for fn, _n in fns:                                          # warm-up: code objects, caches, torch's workspaces
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.repeats):                               # alternated
        for k, (fn, it) in enumerate(fns):
            t[k].append(timed(fn, it))
    med = [statistics.median(v) for v in t]
    line = f"{label:38s}: {spread(t[0])} us {voxels / med[0] / 1e3:6.2f} Gvoxel/s  out + in {2 * voxels * size / med[0] / 1e3:7.1f} GB/s"
    if stream_gbs:
        line += f" = {2 * voxels * size / med[0] / 1e3 / stream_gbs:5.3f} of streaming"
    line += f"   derive 1x {spread(t[1])} us, resample / derive {med[0] / med[1]:5.2f}"
    if base:
        line += f"   grid_sample {spread(t[2])} us, resample / torch {med[0] / med[2]:6.3f}"
    emit(line)


deg = math.pi / 180
m_out = 5 * n // 8
# label, output edge, matrix, filter
CASES = [("identity", n, vv.resample_matrix(), vv.RESAMPLE_TEX8),
         ("30 deg about z", n, vv.resample_matrix((0, 0, 30 * deg)), vv.RESAMPLE_TEX8),
         ("30 deg about x", n, vv.resample_matrix((30 * deg, 0, 0)), vv.RESAMPLE_TEX8),
         ("compound 30 / -20 / 45 deg", n, vv.resample_matrix((30 * deg, -20 * deg, 45 * deg)), vv.RESAMPLE_TEX8),
         ("2x zoom-in", n, vv.resample_matrix(zoom=2.0), vv.RESAMPLE_TEX8),
         (f"identity -> {m_out}^3", m_out, vv.resample_matrix(), vv.RESAMPLE_TEX8),
         ("identity, NEAREST", n, vv.resample_matrix(), vv.RESAMPLE_NEAREST)]

emit(f"library {vv.LIB_PATH}" + (f", VV_RESAMPLE_BLOCKS={os.environ['VV_RESAMPLE_BLOCKS']}" if "VV_RESAMPLE_BLOCKS" in os.environ else ""))
emit(f"volume {n}^3 (noise), {args.iters} calls per timing ({args.base_iters} of the torch baseline), {args.repeats} repeats (median [min .. max])"
     + (f"; hbm_lines sequential streaming {stream_gbs:.1f} GB/s" if stream_gbs else "; no streaming yardstick"))
emit("out + in GB/s = 2 x the output's bytes / time (what a dense copy of that many voxels moves), for every case alike")
tf = vv.transfer_preset(vv.TF_HEAD)
v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev)
ctx.generate_noise_device(v8.data_ptr(), n, n, n, 3)
torch.cuda.synchronize()
for voxel in args.voxels.split(","):
    f32 = voxel == "f32"
    size = 4 if f32 else 1
    if f32:
        dense = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        ctx.promote_device(v8.data_ptr(), dense.data_ptr(), n ** 3)
        ctx.load_volume_device(dense.data_ptr(), vv.VOXEL_F32, n, n, n, tf)
    else:
        dense = v8
        ctx.load_volume_device(v8.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
    torch.cuda.synchronize()
    out = torch.empty(n ** 3 * size, dtype=torch.uint8, device=dev)
    own = vv.VOXEL_F32 if f32 else vv.VOXEL_U8
    pitched = ctx.device_bytes()[0] != n ** 3 * size + (n + 2) * n * size + 4096
    t5 = (dense if f32 else dense.float()).view(1, 1, n, n, n) if not args.no_baseline else None        # (u8: torch samples floats; the conversion is not timed)
    for name, mo, mat, filt in CASES:
        base = grid = None
        if not args.no_baseline:
            A = torch.tensor(mat.reshape(3, 4), dtype=torch.float64)
            theta = torch.cat([A[:, :3], (A[:, :3].sum(dim=1) + 2 * A[:, 3] - 1)[:, None]], dim=1).float()[None].to(dev)   # p' = 2 p - 1 of q' = 2 q - 1
            grid = F.affine_grid(theta, [1, 1, mo, mo, mo], align_corners=False)
            mode = "nearest" if filt == vv.RESAMPLE_NEAREST else "bilinear"
            base = lambda grid=grid, mode=mode: F.grid_sample(t5, grid, mode=mode, padding_mode="zeros", align_corners=False)
        box = None if mo == n else ((0, 0, 0), (mo, mo, mo))
        measure(f"{voxel:3s} {'re-pitched' if pitched else 'dense':10s} {name}", mo ** 3, size,
                lambda: ctx.resample_device(out.data_ptr(), out.numel(), (mo, mo, mo), mat, filt, 0.0, own, stream=stream),
                lambda: ctx.derive_device(out.data_ptr(), out.numel(), box, 1, vv.REDUCE_MEAN, own, stream=stream),
                base)
        del base, grid
        torch.cuda.empty_cache()
    del t5, out
    if f32:
        del dense
    torch.cuda.empty_cache()
