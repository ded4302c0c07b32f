"""The fill blocks of march_kernel (volume-viz_amd/csrc/vv_fill.h) walked on the CPU.  No GPU."""
import os
import subprocess

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_fill_grid_walk():
    """bin/fill_grid_check walks the fill-block to pixel mapping through the functions of csrc/vv_fill.h that march_kernel and render_frame use: frames
    2 x 2 ... 70 x 45, every block and wave-tile shape choose_launch reaches, rectangles inside the frame, touching each edge, covering it and empty,
    shards of 2 and 3 ranks and row ranges, with the product's 4096 pixels per block and with 256 and 768 (many blocks per region).  Every owned pixel
    outside the rectangle is written by exactly one fill block, no other pixel is written at all, and there are fill blocks exactly when there is
    something to fill."""
    r = subprocess.run([os.path.join(REPO, "volume-viz_amd", "bin", "fill_grid_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout, r.stdout[-4000:]
