"""Maximum-intensity projection pinned by the compositing oracle (test infrastructure only).

The level-set identity.  Let T_k be the table whose entries k..255 are (1,1,1,1) and whose entries 0..k-1 are zero.  Under
the oracle's render with T_k a pixel's alpha byte is 255 iff some executed sample has index >= k: the first such sample
blends with factor 1 * (1 - 0), so alpha becomes exactly 1, and no later sample can change it; otherwise every sample
blends with factor 0 and the byte is 0.  Hence the per-pixel maximum M over the executed samples equals the number of k
in 1..255 whose frame has alpha 255 at that pixel -- no pixel of the oracle has to be touched to pin a MIP frame.

`sweep` checks the identity's own preconditions on every input it is given (alpha bytes in {0, 255}, hit sets monotone
in k); `assert_not_vacuous` adds the two conditions that keep a comparison against M from passing on an empty image."""
from __future__ import annotations

import contextlib
import os

import numpy as np

import oracle_lib as O
import volviz_amd as vv


def level_table(k: int) -> np.ndarray:
    tf = np.zeros((256, 4), np.float32)
    tf[k:] = 1.0
    return tf.reshape(1024)


def rgba_of(tf: np.ndarray, index: np.ndarray) -> np.ndarray:
    """channel c = sat_u8(clamp(tf[M][c], 0, 1) * 255) in binary32 (pack_rgba's conversion), for an index image of any shape."""
    t = np.ascontiguousarray(tf, np.float32).reshape(256, 4)
    lut = (np.clip(t, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)       # (products <= 255: the cast truncates)
    return lut[index]


def written_mask(vol, W, H, cam, **kw) -> np.ndarray:
    """[H, W] bool: the pixels a frame with these options writes (two oracle frames over different fill bytes)."""
    a, _ = O.render(vol, level_table(256), W, H, cam, fill=0x00, **kw)
    b, _ = O.render(vol, level_table(256), W, H, cam, fill=0xFF, **kw)
    return np.all(a == b, axis=-1)


def sweep(vol, W, H, cam, *, slice=None, rays=None, options_kw=None) -> np.ndarray:
    """M [H, W] uint8 from 255 oracle frames (0 at pixels the frame does not write)."""
    kw = dict(options_kw or {})
    M = np.zeros((H, W), np.int32)
    prev = None
    for k in range(1, 256):
        frame, _ = O.render(vol, level_table(k), W, H, cam, slice=slice, rays=rays, options=vv.make_options(**kw), fill=0)
        a = frame[..., 3]
        assert np.isin(a, (0, 255)).all(), f"level {k}: alpha bytes other than 0 / 255"
        hit = a == 255
        if prev is not None:
            assert not (hit & ~prev).any(), f"level {k}: a pixel hit at level {k} but not at level {k - 1}"
        M += hit
        prev = hit
    return M.astype(np.uint8)


def assert_not_vacuous(M: np.ndarray, what: str = ""):
    share = float((M > 0).mean())
    levels = len(np.unique(M))
    assert share >= 0.25, f"{what}: M > 0 on {share:.3f} of the pixels only"
    assert levels >= 30, f"{what}: {levels} distinct levels only"


def executed_samples(vol, W, H, cam, *, slice=None, rays=None, options_kw=None) -> int:
    """What a frame executes when no ray ever terminates early: the oracle's count under an all-zero-opacity table."""
    _, n = O.render(vol, np.zeros(1024, np.float32), W, H, cam, slice=slice, rays=rays, options=vv.make_options(**dict(options_kw or {})))
    return n


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the GPU comparisons (tests/test_mip_geometry.py)
# ---------------------------------------------------------------------------------------------------------------------
# every VV_* knob the library reads (vv_api.cpp: vv_knobs::read and the pitch knobs of the volume load)
ALL_KNOBS = ("VV_TILE_LOG2W", "VV_XCD_BAND", "VV_UNROLL", "VV_LDS_RESERVE", "VV_LDS_RESERVE_PHONG", "VV_BRICKED", "VV_ZPAIR", "VV_BLOCK_W", "VV_TAIL",
             "VV_ZFAST", "VV_FORCE_BIG", "VV_RECT", "VV_LPT", "VV_LPT_RUN", "VV_PHONG_BRICKS", "VV_PITCH_PAD", "VV_PITCH_FORCE", "VV_PITCH_ROWS")


@contextlib.contextmanager
def knobs(ctx, env):
    """The VV_* knobs of `env` and no others, picked up by `ctx` (the knobs are read at volume load and by vv_reread_env, never per frame); the
    environment the block found is put back at its end and re-read, so that no later test inherits a knob."""
    saved = {k: os.environ.get(k) for k in ALL_KNOBS}
    try:
        for k in ALL_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        ctx.reread_env()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ctx.reread_env()


def expect(M, written, tf, fill):
    """The two images (rgba [H, W, 4], index [H, W]) a MIP frame over `fill` bytes must hold."""
    idx = np.where(written, M, np.uint8(fill)).astype(np.uint8)
    rgba = np.where(written[..., None], rgba_of(tf, M), np.uint8(fill)).astype(np.uint8)
    return rgba, idx


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def assert_frame(ctx, M, written, tf, fill, W, H, cam, what, **kw):
    """One GPU frame over `fill`, both images against the expectation, every pixel; returns (rgba, index)."""
    rgba, idx = ctx.render_mip(W, H, cam, fill=fill, return_index=True, **kw)
    want_rgba, want_idx = expect(M, written, tf, fill)
    assert_same(idx, want_idx, f"{what}: index image")
    assert_same(rgba, want_rgba, f"{what}: rgba")
    return rgba, idx


def share_and_levels(M):
    return float((M > 0).mean()), len(np.unique(M))
