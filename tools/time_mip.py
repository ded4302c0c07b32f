#!/usr/bin/env python3
"""developer tool (1 GPU): what a maximum-intensity projection frame costs against the compositing frame that fetches the same bytes.

    make -C volume-viz_amd variant NAME=parent        in a checkout of the PARENT commit (or any tree to compare against); copy
                                                      lib_v/libvolviz_parent.so to this tree's volume-viz_amd/lib_v/
    python tools/time_mip.py [--baseline-lib volume-viz_amd/lib_v/libvolviz_parent.so] [--out profiles/mip_c3.txt]

Workload: C3 (1024^3 f32 noise volume, 1920 x 1080, step 1/512) from bench.py's memory-axis camera and its rotated camera (bricked copy).
Baseline: vv_render of the baseline library with an all-zero-opacity table -- no ray ever terminates, so the frame executes every sample a MIP
frame executes and gathers the same bytes.  One process per camera holds both libraries and alternates windows of --frames frames (device
events around each window, warm-up first): baseline, MIP (RGBA image), MIP (RGBA + index image), ... and a closing baseline window.  The
margin MIP is allowed is the spread of the baseline's own windows in the same run.

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
    mip = vv.Context(0)
    base = vv.Context(0, lib_path=os.path.abspath(args.baseline_lib))
    v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev); mip.generate_noise_device(v8.data_ptr(), n, n, n, 0x9E3779B9, stream)
    v32 = torch.empty(n ** 3, dtype=torch.float32, device=dev); mip.promote_device(v8.data_ptr(), v32.data_ptr(), n ** 3, stream)
    torch.cuda.synchronize()
    ramp = np.zeros((256, 4), np.float32); ramp[:, :3] = (np.arange(256, dtype=np.float32) / 255)[:, None]; ramp[:, 3] = 1.0
    for c, tf in ((mip, ramp.reshape(1024)), (base, np.zeros(1024, np.float32))):      # baseline: all-zero opacity, every sample executed
        c.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, n, n, n, tf, stream)
        c.set_frame_timing(False)
    torch.cuda.synchronize()
    frame = torch.zeros(H * W, dtype=torch.int32, device=dev); index = torch.zeros(H * W, dtype=torch.uint8, device=dev)
    o = vv.make_options(step=1 / steps)
    calls = {
        "baseline": lambda: base.render_device(W, H, cam, frame.data_ptr(), options=o, stream=stream),
        "mip": lambda: mip.render_mip_device(W, H, cam, frame.data_ptr(), 0, options=o, stream=stream),
        "mip+index": lambda: mip.render_mip_device(W, H, cam, frame.data_ptr(), index.data_ptr(), options=o, stream=stream),
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
    launches = {"baseline": base.last_launch()}
    calls["mip"](); torch.cuda.synchronize(); launches["mip"] = mip.last_launch()
    # the two frames execute the same samples: counted once each, outside the timed windows
    oc = vv.make_options(step=1 / steps, count_samples=True)
    base.render_device(W, H, cam, frame.data_ptr(), options=oc, stream=stream); torch.cuda.synchronize(); n_base = base.last_sample_count()
    mip.render_mip_device(W, H, cam, frame.data_ptr(), 0, options=oc, stream=stream); torch.cuda.synchronize(); n_mip = mip.last_sample_count()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, call in calls.items():
            times[k].append(window(call, args.frames))
    times["baseline"].append(window(calls["baseline"], args.frames))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = max(times["baseline"]) - min(times["baseline"])
    lines = [f"camera {args.child}: {n}^3 f32, {W} x {H}, step 1/{steps}; {args.frames} frames per window after {args.warmup} warm-up frames, {args.rounds} alternations",
             f"  launch baseline {launches['baseline']}", f"  launch mip      {launches['mip']}",
             f"  executed samples: baseline {n_base}, mip {n_mip} ({'equal' if n_base == n_mip else 'DIFFERENT'})"]
    for k, v in times.items():
        lines.append(f"  {k:10s} ms/frame per window: " + " ".join(f"{t:.4f}" for t in v) + f"   median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
    lines.append(f"  baseline spread (max - min of its windows): {spread:.4f} ms = {100 * spread / med['baseline']:.2f} %")
    for k in ("mip", "mip+index"):
        d = med[k] - med["baseline"]
        lines.append(f"  {k:10s} - baseline (medians): {d:+.4f} ms = {100 * d / med['baseline']:+.2f} %   -> " +
                     ("no slower than the baseline within its spread" if d <= spread else "SLOWER than the baseline by more than its spread"))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "a") as f:
        f.write(text)
    mip.close(); base.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=os.path.join(REPO, "volume-viz_amd", "lib_v", "libvolviz_parent.so"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mip_c3.txt"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a camera's child may take")
    ap.add_argument("--child", choices=CAMERAS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not os.path.exists(args.baseline_lib):
        sys.exit(f"{args.baseline_lib} not found: build the baseline as a variant library first (see the head of this file)")
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("tools/time_mip.py: vv_render_mip against vv_render (baseline library, all-zero-opacity table), windows alternated in one process\n")
    step = ("timeout -k 10 {t} {py} {me} --child {cam} --baseline-lib {lib} --out {out} --frames {fr} --warmup {wu} --rounds {ro} --size {sz}")
    cmd = " && ".join(step.format(t=args.step_timeout, py=sys.executable, me=os.path.abspath(__file__), cam=c, lib=os.path.abspath(args.baseline_lib), out=out,
                                  fr=args.frames, wu=args.warmup, ro=args.rounds, sz=args.size) for c in CAMERAS)
    sys.exit(subprocess.call(["bash", "-c", cmd], cwd=REPO))


if __name__ == "__main__":
    main()
