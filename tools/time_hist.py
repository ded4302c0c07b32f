"""developer tool (1 GPU): time of a volume histogram (vv_volume_histogram) and of an index-image histogram (vv_histogram_indices) writing into
device buffers, as bytes of voxels read per second, against two baselines:
  - torch.bincount (u8) / torch.histc (f32, 256 bins over [0, 1]) on a dense device tensor of the same voxels: what a host would reach for today if
    it could see the volume (it cannot: the volume lives in the library's layout; the tensor here is a copy made outside the timing, and histc
    neither clamps nor counts NaNs nor finds the range);
  - the streaming read rate tools/ubench/hbm_lines.hip reports on the same machine (run as a child process when its binary is built:
    hipcc -O3 --offload-arch=gfx950 -o tools/ubench/bin/hbm_lines tools/ubench/hbm_lines.hip).

Cases: the whole n^3 volume and a (n/4)^3 sub-box with misaligned corners, for u8 and f32, for the noise volume (uniform bins) and the default brain
(mostly zeros), and a 1920 x 1080 index image.  Histogram and baseline run in one process and alternate; every figure is the median over the
repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library (make variant), --no-baseline
times the library alone.
    python tools/time_hist.py [--n 1024] [--iters 50] [--base-iters 5] [--repeats 3] [--voxels f32,u8] [--no-baseline] [--out FILE]"""
import argparse, os, re, statistics, subprocess, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=50, help="histogram calls per timing")
ap.add_argument("--base-iters", type=int, default=5, help="baseline calls per timing")
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
out = torch.zeros(2072, dtype=torch.uint8, device=dev)
counts = torch.zeros(256, dtype=torch.int64, device=dev)
q = n // 4
lo = (q + 3, q + 5, q + 7)                                      # misaligned corners: no row of the box starts or ends on a 16-byte boundary
BOXES = (("whole", None), (f"box {q}^3 at {lo}", (lo, tuple(a + q for a in lo))))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                    # us per call of fn


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):9.1f} .. {max(v):9.1f}]"


def measure(label, nbytes, ours, base, base_name):
    for _ in range(2):                                          # warm-up: code objects, caches, torch's workspaces
        ours()
        if base:
            base()
    torch.cuda.synchronize()
    to, tb = [], []
    for _ in range(args.repeats):                               # alternated
        to.append(timed(ours, args.iters))
        if base:
            tb.append(timed(base, args.base_iters))
    gbs = nbytes / statistics.median(to) / 1e3
    line = f"{label:52s}: {spread(to)} us  {gbs:7.1f} GB/s"
    if stream_gbs:
        line += f"  = {gbs / stream_gbs:5.3f} of streaming"
    if tb:
        line += f"   {base_name} {spread(tb)} us   histogram / {base_name} {statistics.median(to) / statistics.median(tb):6.3f} [{min(to) / max(tb):6.3f} .. {max(to) / min(tb):6.3f}]"
    emit(line)


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3, {args.iters} calls per timing ({args.base_iters} of the baseline), {args.repeats} repeats (median [min .. max])"
     + (f"; hbm_lines sequential streaming {stream_gbs:.1f} GB/s" if stream_gbs else "; no streaming yardstick"))
tf = vv.transfer_preset(vv.TF_HEAD)
v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev)
for content in ("noise", "brain"):
    if content == "noise":
        ctx.generate_noise_device(v8.data_ptr(), n, n, n, 3)
    else:
        ctx.generate_default_brain_device(v8.data_ptr(), n, n, n)
    torch.cuda.synchronize()
    for voxel in args.voxels.split(","):
        if voxel == "f32":
            dense = torch.empty(n ** 3, dtype=torch.float32, device=dev)
            ctx.promote_device(v8.data_ptr(), dense.data_ptr(), n ** 3)
            ctx.load_volume_device(dense.data_ptr(), vv.VOXEL_F32, n, n, n, tf)
        else:
            dense = v8
            ctx.load_volume_device(v8.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
        torch.cuda.synchronize()
        size = 4 if voxel == "f32" else 1
        pitched = ctx.device_bytes()[0] != n ** 3 * size + (n + 2) * n * size + 4096
        for bname, box in BOXES:
            if box is None:
                sub, nvox = dense, n ** 3
            else:
                (x0, y0, z0), (x1, y1, z1) = box
                sub = dense.view(n, n, n)[z0:z1, y0:y1, x0:x1].contiguous().view(-1)     # the same voxels, dense: made outside the timing
                nvox = sub.numel()
            base, base_name = None, ""
            if not args.no_baseline:
                if voxel == "f32":
                    base, base_name = (lambda sub=sub: torch.histc(sub, bins=256, min=0.0, max=1.0)), "torch.histc"
                else:
                    base, base_name = (lambda sub=sub: torch.bincount(sub, minlength=256)), "torch.bincount"
            measure(f"{voxel:3s} {content:5s} {'re-pitched' if pitched else 'dense':10s} {bname}", nvox * size,
                    lambda box=box: ctx.histogram_device(out.data_ptr(), box, stream=stream), base, base_name)
            del sub
        if voxel == "f32":
            del dense
    if content == "noise":                                      # a 1920 x 1080 index image: bytes of the noise volume
        img = v8[12345:12345 + 1920 * 1080].clone()
        measure("index image 1920 x 1080 (noise)", img.numel(), lambda: ctx.histogram_indices_device(img.data_ptr(), img.numel(), counts.data_ptr(), stream=stream),
                None if args.no_baseline else (lambda: torch.bincount(img, minlength=256)), "torch.bincount")
    else:
        img = v8[n ** 3 // 2:n ** 3 // 2 + 1920 * 1080].clone()
        measure("index image 1920 x 1080 (brain)", img.numel(), lambda: ctx.histogram_indices_device(img.data_ptr(), img.numel(), counts.data_ptr(), stream=stream),
                None if args.no_baseline else (lambda: torch.bincount(img, minlength=256)), "torch.bincount")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
