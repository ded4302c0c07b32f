#!/usr/bin/env python3
"""developer tool (1 GPU): what a projection frame (vv_render_projection: MAX, MIN, MEAN) costs against the MIP frame of the same view, in the same build.

    python tools/time_proj.py [--out profiles/proj_c3.txt]

Workload: C3 (1024^3 f32 noise volume, 1920 x 1080, step 1/512) from bench.py's memory-axis camera (view a) and its rotated camera.  Yardstick:
vv_render_mip of the same library with its RGBA and index images -- it executes the same rays and samples.  One process per camera alternates windows
of --frames frames (device events around each window, warm-up first): MIP, then each mode with RGBA + index images and with all three images, ... and
a closing MIP window.  The margin a projection frame is allowed is the spread of MIP's own windows in the same run.  Executed samples are counted once
per call, outside the timed windows.  (MAX / MIN without a stat image may drop a ray once it has reached 255 / 0; white noise at this step reaches
neither often.)

The driver starts one child per camera, each under `timeout -k 10`, chained with `&&`: a child that fails or hangs ends the run."""
import argparse
import os
import subprocess
import sys

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CAMERAS = ("front", "rotated")


def child(args):
    sys.path.insert(0, os.path.join(REPO, "volume-viz_amd", "python")); sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import volviz_amd as vv
    n, W, H, steps = args.size, 1920, 1080, 512
    cam = vv.Camera() if args.child == "front" else vv.Camera.orbit(4.0, np.pi / 3, np.pi / 5)
    dev = torch.device("cuda", 0); stream = torch.cuda.current_stream().cuda_stream
    ctx = vv.Context(0)
    v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev); ctx.generate_noise_device(v8.data_ptr(), n, n, n, 0x9E3779B9, stream)
    v32 = torch.empty(n ** 3, dtype=torch.float32, device=dev); ctx.promote_device(v8.data_ptr(), v32.data_ptr(), n ** 3, stream)
    torch.cuda.synchronize()
    del v8
    ramp = np.zeros((256, 4), np.float32); ramp[:, :3] = (np.arange(256, dtype=np.float32) / 255)[:, None]; ramp[:, 3] = 1.0
    ctx.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, n, n, n, ramp.reshape(1024), stream)
    ctx.set_frame_timing(False)
    torch.cuda.synchronize()
    frame = torch.zeros(H * W, dtype=torch.int32, device=dev); index = torch.zeros(H * W, dtype=torch.uint8, device=dev)
    stat = torch.zeros(H * W * 2, dtype=torch.int32, device=dev)
    o = vv.make_options(step=1 / steps)
    modes = (("max", vv.PROJ_MAX), ("min", vv.PROJ_MIN), ("mean", vv.PROJ_MEAN))

    def proj(mode, three, opts=o):
        return lambda: ctx.render_projection_device(W, H, cam, mode, frame.data_ptr(), index.data_ptr(), stat.data_ptr() if three else 0, options=opts, stream=stream)
    calls = {"mip": lambda: ctx.render_mip_device(W, H, cam, frame.data_ptr(), index.data_ptr(), options=o, stream=stream)}
    for name, mode in modes:
        calls[name] = proj(mode, False)
        calls[name + "+stat"] = proj(mode, True)

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
    for k in ("mip", "max"):
        calls[k](); torch.cuda.synchronize(); launches[k] = ctx.last_launch()
    oc = vv.make_options(step=1 / steps, count_samples=True)
    counts = {}
    ctx.render_mip_device(W, H, cam, frame.data_ptr(), index.data_ptr(), options=oc, stream=stream); torch.cuda.synchronize(); counts["mip"] = ctx.last_sample_count()
    for name, mode in modes:
        proj(mode, True, oc)(); torch.cuda.synchronize(); counts[name] = ctx.last_sample_count()
    s = stat.cpu().numpy().view(np.uint32).reshape(H, W, 2)[:-1, :-1]              # (the MEAN frame's records: the last call above)
    counted = int(s[..., 1].astype(np.int64).sum())
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, call in calls.items():
            times[k].append(window(call, args.frames))
    times["mip"].append(window(calls["mip"], args.frames))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = max(times["mip"]) - min(times["mip"])
    same = all(counts[k] == counts["mip"] for k, _ in modes)
    lines = [f"camera {args.child}: {n}^3 f32 noise, {W} x {H}, step 1/{steps}; {args.frames} frames per window after {args.warmup} warm-up frames, {args.rounds} alternations",
             f"  launch mip      {launches['mip']}", f"  launch proj max {launches['max']}",
             f"  executed samples: mip {counts['mip']}, max {counts['max']}, min {counts['min']}, mean {counts['mean']} ({'equal' if same else 'DIFFERENT'}); "
             f"counted (inside the volume): {counted} = {100 * counted / max(counts['mip'], 1):.2f} %"]
    for k, v in times.items():
        lines.append(f"  {k:10s} ms/frame per window: " + " ".join(f"{t:.4f}" for t in v) + f"   median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}  spread {max(v) - min(v):.4f}")
    lines.append(f"  mip spread (max - min of its windows): {spread:.4f} ms = {100 * spread / med['mip']:.2f} %")
    for k in calls:
        if k == "mip":
            continue
        d = med[k] - med["mip"]
        lines.append(f"  {k:10s} - mip (medians): {d:+.4f} ms = {100 * d / med['mip']:+.2f} %   -> " +
                     ("no slower than MIP within its spread" if d <= spread else "SLOWER than MIP by more than its spread"))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "a") as f:
        f.write(text)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "proj_c3.txt"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a camera's child may take")
    ap.add_argument("--child", choices=CAMERAS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("tools/time_proj.py: vv_render_projection against vv_render_mip of the same library, windows alternated in one process\n")
    step = "timeout -k 10 {t} {py} {me} --child {cam} --out {out} --frames {fr} --warmup {wu} --rounds {ro} --size {sz}"
    cmd = " && ".join(step.format(t=args.step_timeout, py=sys.executable, me=os.path.abspath(__file__), cam=c, out=out,
                                  fr=args.frames, wu=args.warmup, ro=args.rounds, sz=args.size) for c in CAMERAS)
    sys.exit(subprocess.call(["bash", "-c", cmd], cwd=REPO))


if __name__ == "__main__":
    main()
