#!/usr/bin/env python3
"""developer tool (1 GPU): what an isosurface frame costs against the MIP frame of the same view, in the same build.

    python tools/time_iso.py [--out profiles/iso_c3.txt]

Workload: C3 (1024^3 f32 noise volume, its values halved so that some level is out of reach; 1920 x 1080, step 1/512) from bench.py's view a
(the memory-axis camera).  Three calls, alternated
in windows of --frames frames in one process (device events around each window, warm-up first): vv_render_mip (the yardstick),
vv_render_iso at a level no sample reaches -- it executes the rays and samples of the MIP frame, so it should cost what MIP costs -- and
vv_render_iso at the median of the frame's non-zero MIP indices, which should be faster in proportion to the samples it skips.  A closing
MIP window follows; the margin the unreachable-level frame is allowed is the spread of MIP's own windows in the same run.  The executed
samples of all three are counted once each, outside the timed windows.

The driver starts the one child under `timeout -k 10`: a child that fails or hangs ends the run."""
import argparse
import os
import subprocess
import sys

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def child(args):
    sys.path.insert(0, os.path.join(REPO, "volume-viz_amd", "python")); sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import volviz_amd as vv
    n, W, H, steps = args.size, 1920, 1080, 512
    cam = vv.Camera()
    dev = torch.device("cuda", 0); stream = torch.cuda.current_stream().cuda_stream
    ctx = vv.Context(0)
    v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev); ctx.generate_noise_device(v8.data_ptr(), n, n, n, 0x9E3779B9, stream)
    v32 = torch.empty(n ** 3, dtype=torch.float32, device=dev); ctx.promote_device(v8.data_ptr(), v32.data_ptr(), n ** 3, stream)
    v32.mul_(0.5)                   # the noise reaches 1.0 = index 255, the highest level: halved, every level above 127 is out of reach (same bytes, same samples)
    torch.cuda.synchronize()
    del v8
    ramp = np.zeros((256, 4), np.float32); ramp[:, :3] = (np.arange(256, dtype=np.float32) / 255)[:, None]; ramp[:, 3] = 1.0
    ctx.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, n, n, n, ramp.reshape(1024), stream)
    ctx.set_frame_timing(False)
    torch.cuda.synchronize()
    frame = torch.zeros(H * W, dtype=torch.int32, device=dev); index = torch.zeros(H * W, dtype=torch.uint8, device=dev)
    hit = torch.zeros(H * W * 4, dtype=torch.float32, device=dev)
    o = vv.make_options(step=1 / steps)
    ctx.render_mip_device(W, H, cam, 0, index.data_ptr(), options=o, stream=stream); torch.cuda.synchronize()
    M = index.cpu().numpy()
    median, top = int(np.median(M[M > 0])), int(M.max())
    assert top < 255, top
    unreachable = top + 1

    def iso(level, opts=o, three=True):
        return lambda: ctx.render_iso_device(W, H, cam, level, frame.data_ptr(), index.data_ptr() if three else 0, hit.data_ptr() if three else 0,
                                             options=opts, stream=stream)
    calls = {
        "mip": lambda: ctx.render_mip_device(W, H, cam, frame.data_ptr(), index.data_ptr(), options=o, stream=stream),
        "iso-none": iso(unreachable),
        "iso-median": iso(median),
        "iso-median-rgba": iso(median, three=False),
    }

    def window(call, frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            call()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / frames

    for call in calls.values():
        window(call, args.warmup)
    launches = {}
    for k in ("mip", "iso-none"):
        calls[k](); torch.cuda.synchronize(); launches[k] = ctx.last_launch()
    oc = vv.make_options(step=1 / steps, count_samples=True)
    counts = {}
    ctx.render_mip_device(W, H, cam, frame.data_ptr(), 0, options=oc, stream=stream); torch.cuda.synchronize(); counts["mip"] = ctx.last_sample_count()
    for k, level in (("iso-none", unreachable), ("iso-median", median)):
        iso(level, oc)(); torch.cuda.synchronize(); counts[k] = ctx.last_sample_count()
    hits = int((index.cpu().numpy() > 0).sum())
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, call in calls.items():
            times[k].append(window(call, args.frames))
    times["mip"].append(window(calls["mip"], args.frames))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = max(times["mip"]) - min(times["mip"])
    lines = [f"view a: {n}^3 f32 noise x 0.5, {W} x {H}, step 1/{steps}; {args.frames} frames per window after {args.warmup} warm-up frames, {args.rounds} alternations",
             f"  levels: median {median}, unreachable {unreachable} (the frame's largest index is {top}); hits at the median level: {hits} of {(W - 1) * (H - 1)} pixels",
             f"  launch mip      {launches['mip']}", f"  launch iso-none {launches['iso-none']}",
             f"  executed samples: mip {counts['mip']}, iso-none {counts['iso-none']} ({'equal' if counts['mip'] == counts['iso-none'] else 'DIFFERENT'}), "
             f"iso-median {counts['iso-median']} = {100 * counts['iso-median'] / max(counts['mip'], 1):.2f} % of mip"]
    for k, v in times.items():
        lines.append(f"  {k:16s} ms/frame per window: " + " ".join(f"{t:.4f}" for t in v) + f"   median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
    lines.append(f"  mip spread (max - min of its windows): {spread:.4f} ms = {100 * spread / med['mip']:.2f} %")
    d = med["iso-none"] - med["mip"]
    lines.append(f"  iso-none - mip (medians): {d:+.4f} ms = {100 * d / med['mip']:+.2f} %   -> " +
                 ("no slower than MIP within its spread" if d <= spread else "SLOWER than MIP by more than its spread"))
    for k in ("iso-median", "iso-median-rgba"):
        lines.append(f"  {k} / mip (medians): {100 * med[k] / med['mip']:.2f} % of the time for {100 * counts['iso-median'] / max(counts['mip'], 1):.2f} % of the samples")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "a") as f:
        f.write(text)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "iso_c3.txt"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the child may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("tools/time_iso.py: vv_render_iso against vv_render_mip of the same library, windows alternated in one process\n")
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", out, "--frames", str(args.frames),
           "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--size", str(args.size)]
    sys.exit(subprocess.call(cmd, cwd=REPO))


if __name__ == "__main__":
    main()
