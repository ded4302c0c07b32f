#!/usr/bin/env python3
"""Developer aid: the C3 frame (1024^3 f32 noise volume, 1920 x 1080, step 1/512, ramp table) under a MOVING view: the camera orbits the volume on the
equator, 0.1 degrees of azimuth per frame, to and fro within 5 degrees of view a (the launch policy's choice for the aligned view holds
throughout), so every frame launches the radius pre-pass (no frame's pre-pass arguments equal the last one's).  Event-times FRAMES frames enqueued on one stream after a warm-up and prints one JSON line: ms per frame, and what the context says
about its pre-passes where the library has the read-out.  A/B against another build of the library:
    python tools/run_with_lib.py <lib.so> tools/time_prepass.py          usage (GPU box): python tools/time_prepass.py [frames] [--still]
--still keeps the camera where it is (every frame after the first reuses the radii): the same loop as a reference point."""
import json, os, sys
REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "volume-viz_amd", "python")); sys.path.insert(0, REPO)
import numpy as np
import torch
import volviz_amd as vv
import bench

args = [a for a in sys.argv[1:] if not a.startswith("--")]
FRAMES = int(args[0]) if args else 200
STILL = "--still" in sys.argv
WARM, N, W, H, STEPS = 100, 1024, 1920, 1080, 512
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
ctx = vv.Context(0)
ts = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(ts)
stream = vv.stream_handle(ts)
v8 = torch.empty(N ** 3, dtype=torch.uint8, device=dev)
ctx.generate_noise_device(v8.data_ptr(), N, N, N, 0x9E3779B9, stream)
v32 = torch.empty(N ** 3, dtype=torch.float32, device=dev)
ctx.promote_device(v8.data_ptr(), v32.data_ptr(), N ** 3, stream)
ctx.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, N, N, N, bench.ramp_tf(), stream)
torch.cuda.synchronize()
del v8, v32
torch.cuda.empty_cache()
ctx.set_frame_timing(False)
frame = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
opts = vv.make_options(step=1.0 / STEPS)
# view a looks along +z from (0, 0, -4): theta = 90 degrees, phi = -90 degrees on the orbit of radius 4
cams = [vv.Camera.orbit(4.0, np.pi / 2, -np.pi / 2 + (0.0 if STILL else np.radians(0.1 * (abs(k % 200 - 100) - 50)))) for k in range(WARM + FRAMES)]
for k in range(WARM):
    ctx.render_device(W, H, cams[k], frame.data_ptr(), options=opts, stream=stream)
torch.cuda.synchronize()
try:
    state0 = ctx.prepass_state()
except Exception:                           # (a library from before the read-out)
    state0 = None
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(ts)
for k in range(WARM, WARM + FRAMES):
    ctx.render_device(W, H, cams[k], frame.data_ptr(), options=opts, stream=stream)
e1.record(ts)
torch.cuda.synchronize()
out = {"tool": "time_prepass", "view": "still" if STILL else "0.1 degrees of azimuth per frame", "frames": FRAMES, "ms_per_frame": round(e0.elapsed_time(e1) / FRAMES, 4),
       "launch": ctx.last_launch()}
if state0 is not None:
    s = ctx.prepass_state()
    out["prepasses_launched"] = s[0] - state0[0]; out["frames_reused"] = s[1] - state0[1]; out["fill_blocks"] = s[3]
print(json.dumps(out))
ctx.close()
