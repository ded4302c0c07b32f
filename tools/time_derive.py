"""developer tool (1 GPU): time of vv_derive_volume writing into a device buffer, as bytes moved per second (source bytes of the box + output
bytes), against three baselines:
  - vv_volume_histogram of the same box of the same volume: it reads the same source bytes;
  - what a host would reach for if it could see the volume -- torch.nn.functional.avg_pool3d / max_pool3d, (t * 255).clamp(0, 255).to(uint8),
    (t - lo) / (hi - lo), a strided copy of the box -- on a dense device tensor of the same voxels (it cannot: the volume lives in the library's
    layout; the tensor here is a copy made outside the timing; u8 tensors are pooled as float, which torch's pooling needs);
  - the streaming read rate tools/ubench/hbm_lines.hip reports on the same machine (run as a child process when its binary is built:
    hipcc -O3 --offload-arch=gfx950 -o tools/ubench/bin/hbm_lines tools/ubench/hbm_lines.hip).

Cases, for an n^3 noise volume as f32 and as u8: the whole volume reduced 2x and 4x (MEAN) and 2x (MAX), factor 1 into u8 (f32: the index volume),
factor 1 windowed into f32, and a (n/4)^3 box with misaligned corners copied out.  Derive call and baselines run in one process and alternate; every
figure is the median over the repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library.
    python tools/time_derive.py [--n 1024] [--iters 50] [--base-iters 5] [--repeats 3] [--voxels f32,u8] [--no-baseline] [--out FILE]"""
import argparse, os, re, statistics, subprocess, sys
import numpy as np
import torch
import torch.nn.functional as F
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=50, help="derive / histogram calls per timing")
ap.add_argument("--base-iters", type=int, default=5, help="torch baseline calls per timing")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--voxels", default="f32,u8")
ap.add_argument("--no-baseline", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.iters >= 1 and args.base_iters >= 1 and args.repeats >= 1

lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


# the streaming yardstick first, in a process of its own, before this one holds any memory
stream_gbs = None
ubench = os.path.join(HERE, "ubench", "bin", "hbm_lines")
if not args.no_baseline and os.path.exists(ubench):
    txt = subprocess.run(["timeout", "-k", "10", "120", ubench], capture_output=True, text=True, check=True).stdout
    m = re.search(r"sequential streaming\s*:\s*[\d.]+ ms\s+([\d.]+) GB/s", txt)
    stream_gbs = float(m.group(1)) if m else None

dev = torch.device("cuda", 0)
ctx = vv.Context(0)
n = args.n
stream = vv.stream_handle(torch.cuda.current_stream())
hist_out = torch.zeros(2072, dtype=torch.uint8, device=dev)
out = torch.empty(n ** 3 * 4, dtype=torch.uint8, device=dev)               # room for the largest output: n^3 f32
q = n // 4
lo = (q + 3, q + 5, q + 7)                                      # misaligned corners: no row of the box starts or ends on a 16-byte boundary
BOX = (lo, tuple(a + q for a in lo))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                    # us per call of fn


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):9.1f} .. {max(v):9.1f}]"


def measure(label, nbytes, src_bytes, ours, hist, base, base_name):
    fns = [(ours, args.iters), (hist, args.iters)] + ([(base, args.base_iters)] if base else [])
    for _ in range(2):                                          # warm-up: code objects, caches, torch's workspaces
        for fn, _n in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.repeats):                               # alternated
        for k, (fn, it) in enumerate(fns):
            t[k].append(timed(fn, it))
    gbs = nbytes / statistics.median(t[0]) / 1e3
    line = f"{label:50s}: {spread(t[0])} us  {gbs:7.1f} GB/s"
    if stream_gbs:
        line += f" = {gbs / stream_gbs:5.3f} of streaming"
    line += f"   histogram {spread(t[1])} us {src_bytes / statistics.median(t[1]) / 1e3:7.1f} GB/s, derive / histogram {statistics.median(t[0]) / statistics.median(t[1]):6.3f}"
    if base:
        line += f"   {base_name} {spread(t[2])} us, derive / torch {statistics.median(t[0]) / statistics.median(t[2]):6.3f}"
    emit(line)


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 (noise), {args.iters} calls per timing ({args.base_iters} of the torch baseline), {args.repeats} repeats (median [min .. max])"
     + (f"; hbm_lines sequential streaming {stream_gbs:.1f} GB/s" if stream_gbs else "; no streaming yardstick"))
emit("GB/s = (source bytes of the box + output bytes) / time; histogram GB/s = source bytes of the box / time")
tf = vv.transfer_preset(vv.TF_HEAD)
v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev)
ctx.generate_noise_device(v8.data_ptr(), n, n, n, 3)
torch.cuda.synchronize()
for voxel in args.voxels.split(","):
    f32 = voxel == "f32"
    if f32:
        dense = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        ctx.promote_device(v8.data_ptr(), dense.data_ptr(), n ** 3)
        ctx.load_volume_device(dense.data_ptr(), vv.VOXEL_F32, n, n, n, tf)
    else:
        dense = v8
        ctx.load_volume_device(v8.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
    torch.cuda.synchronize()
    size = 4 if f32 else 1
    own = vv.VOXEL_F32 if f32 else vv.VOXEL_U8
    pitched = ctx.device_bytes()[0] != n ** 3 * size + (n + 2) * n * size + 4096
    t5 = dense.view(1, 1, n, n, n)
    win = (0.25, 0.75) if f32 else (64.0, 192.0)
    (x0, y0, z0), (x1, y1, z1) = BOX
    as_float = (lambda t: t) if f32 else (lambda t: t.float())
    # label, box, factor, mode, output type, window, torch baseline and its name
    cases = [
        ("whole 2x MEAN", None, 2, vv.REDUCE_MEAN, own, None, lambda: F.avg_pool3d(as_float(t5), 2), "avg_pool3d"),
        ("whole 4x MEAN", None, 4, vv.REDUCE_MEAN, own, None, lambda: F.avg_pool3d(as_float(t5), 4), "avg_pool3d"),
        ("whole 2x MAX", None, 2, vv.REDUCE_MAX, own, None, lambda: F.max_pool3d(as_float(t5), 2), "max_pool3d"),
        ("whole 1x -> u8", None, 1, vv.REDUCE_MEAN, vv.VOXEL_U8, None,
         (lambda: (dense * 255).clamp(0, 255).to(torch.uint8)) if f32 else (lambda: dense.clone()), "(t*255).clamp.to(u8)" if f32 else "clone"),
        ("whole 1x windowed -> f32", None, 1, vv.REDUCE_MEAN, vv.VOXEL_F32, win, lambda: (as_float(dense) - win[0]) / (win[1] - win[0]), "(t-lo)/(hi-lo)"),
        (f"box {q}^3 at {lo} 1x", BOX, 1, vv.REDUCE_MEAN, own, None, lambda: dense.view(n, n, n)[z0:z1, y0:y1, x0:x1].contiguous(), "slice.contiguous"),
    ]
    for name, box, factor, mode, out_type, window, base, base_name in cases:
        m = ctx.derive_dims(box, factor)
        src_vox = n ** 3 if box is None else q ** 3
        out_bytes = m[0] * m[1] * m[2] * (4 if out_type == vv.VOXEL_F32 else 1)
        assert out_bytes <= out.numel()
        measure(f"{voxel:3s} {'re-pitched' if pitched else 'dense':10s} {name}", src_vox * size + out_bytes, src_vox * size,
                lambda: ctx.derive_device(out.data_ptr(), out_bytes, box, factor, mode, out_type, window, stream=stream),
                lambda: ctx.histogram_device(hist_out.data_ptr(), box, stream=stream),
                None if args.no_baseline else base, base_name)
    del t5
    if f32:
        del dense
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
