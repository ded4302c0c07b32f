"""developer tool (1 GPU): time of vv_stencil_volume writing into a device buffer, as bytes moved per second (the volume's bytes + the output's
bytes: what a filter that read every voxel once would move), against three baselines:
  - vv_derive_volume at factor 1 of the same volume into the same type: the same compulsory bytes in and out, the streaming floor of this library;
  - the torch call a host would reach for on a dense tensor of the same voxels (a copy made outside the timing; u8 tensors are filtered as float):
    smoothing: torch.nn.functional.conv3d with a (1, 1, K), a (1, K, 1) and a (K, 1, 1) kernel in turn on a replicate-padded tensor;
    gradient magnitude: differences of shifted slices of the replicate-padded tensor, squares, sqrt;
    median: torch has no 3-D median filter (an unfold of 27 shifted copies of a 1024^3 f32 volume is 108 GiB): no baseline;
  - the streaming read rate tools/ubench/hbm_lines.hip reports on the same machine (run as a child process when its binary is built:
    hipcc -O3 --offload-arch=gfx950 -o tools/ubench/bin/hbm_lines tools/ubench/hbm_lines.hip).

Cases, for an n^3 noise volume as f32 and as u8 with out_type = the volume's type: binomial smoothing with R = 1 and R = 4 on all axes, R = 4 on x
alone, the 3x3x3 median, the gradient magnitude.  Stencil call and baselines run in one process and alternate; every figure is the median over the
repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library.
    python tools/time_stencil.py [--n 1024] [--iters 10] [--base-iters 3] [--repeats 3] [--voxels f32,u8] [--no-baseline] [--out FILE]"""
import argparse, os, re, statistics, subprocess, sys
import numpy as np
import torch
import torch.nn.functional as F
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=10, help="stencil / derive calls per timing")
ap.add_argument("--base-iters", type=int, default=3, help="torch baseline calls per timing")
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
    return f"{statistics.median(v):10.1f} [{min(v):10.1f} .. {max(v):10.1f}]"


def measure(label, nbytes, ours, derive, base, base_name):
    fns = [(ours, args.iters), (derive, args.iters)] + ([(base, args.base_iters)] if base else [])
    for fn, _n in fns:                                          # warm-up: code objects, caches, torch's workspaces
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.repeats):                               # alternated
        for k, (fn, it) in enumerate(fns):
            t[k].append(timed(fn, it))
    med = [statistics.median(v) for v in t]
    line = f"{label:34s}: {spread(t[0])} us  {nbytes / med[0] / 1e3:7.1f} GB/s"
    if stream_gbs:
        line += f" = {nbytes / med[0] / 1e3 / stream_gbs:5.3f} of streaming"
    line += f"   derive 1x {spread(t[1])} us {nbytes / med[1] / 1e3:7.1f} GB/s, stencil / derive {med[0] / med[1]:6.2f}"
    if base:
        line += f"   {base_name} {spread(t[2])} us, stencil / torch {med[0] / med[2]:6.3f}"
    elif not args.no_baseline:
        line += f"   {base_name}"
    emit(line)


def torch_smooth(t5, rows, radius):
    """conv3d with the three 1-D kernels in turn, edges replicated."""
    x = t5
    for axis, (row, r) in enumerate(zip(rows, radius)):                        # x, y, z -> the last, middle and first spatial dimension
        if r == 0:
            continue
        k = torch.tensor([float(row[abs(i)]) for i in range(-r, r + 1)], dtype=torch.float32, device=dev)
        shape, pad = [1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]
        shape[4 - axis] = 2 * r + 1
        pad[2 * axis] = pad[2 * axis + 1] = r
        x = F.conv3d(F.pad(x, pad, mode="replicate"), k.view(shape))
    return x


def torch_gradmag(t5):
    p = F.pad(t5, (1, 1, 1, 1, 1, 1), mode="replicate")[0, 0]
    gx = p[1:-1, 1:-1, 2:] - p[1:-1, 1:-1, :-2]
    gy = p[1:-1, 2:, 1:-1] - p[1:-1, :-2, 1:-1]
    gz = p[2:, 1:-1, 1:-1] - p[:-2, 1:-1, 1:-1]
    return torch.sqrt(gx * gx + gy * gy + gz * gz)


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 (noise), {args.iters} calls per timing ({args.base_iters} of the torch baseline), {args.repeats} repeats (median [min .. max])"
     + (f"; hbm_lines sequential streaming {stream_gbs:.1f} GB/s" if stream_gbs else "; no streaming yardstick"))
emit("GB/s = (the volume's bytes + the output's bytes) / time, for the stencil call and for vv_derive_volume at factor 1 alike")
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
    t5 = (dense if f32 else dense.float()).view(1, 1, n, n, n) if not args.no_baseline else None        # (u8: torch filters floats; the conversion is not timed)
    binom = lambda r: [vv.stencil_taps(vv.TAPS_BINOMIAL, v) for v in r]
    # label, kind, radius, torch baseline and its name
    cases = [("binomial R = 1", vv.STENCIL_SEPARABLE, (1, 1, 1), "conv3d x 3"), ("binomial R = 4", vv.STENCIL_SEPARABLE, (4, 4, 4), "conv3d x 3"),
             ("binomial R = 4 on x alone", vv.STENCIL_SEPARABLE, (4, 0, 0), "conv3d x 1"), ("median 3x3x3", vv.STENCIL_MEDIAN, (0, 0, 0), "(torch has no 3-D median filter)"),
             ("gradient magnitude", vv.STENCIL_GRADMAG, (0, 0, 0), "pad, diff, sqrt")]
    for name, kind, radius, base_name in cases:
        rows = binom(radius)
        base = None
        if not args.no_baseline and kind == vv.STENCIL_SEPARABLE:
            base = lambda rows=rows, radius=radius: torch_smooth(t5, rows, radius)
        elif not args.no_baseline and kind == vv.STENCIL_GRADMAG:
            base = lambda: torch_gradmag(t5)
        measure(f"{voxel:3s} {'re-pitched' if pitched else 'dense':10s} {name}", 2 * n ** 3 * size,
                lambda: ctx.stencil_device(out.data_ptr(), out.numel(), kind, None, own, radius, rows, stream=stream),
                lambda: ctx.derive_device(out.data_ptr(), out.numel(), None, 1, vv.REDUCE_MEAN, own, stream=stream),
                base, base_name)
    del t5, out
    if f32:
        del dense
    torch.cuda.empty_cache()
