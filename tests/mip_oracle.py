"""Maximum-intensity projection pinned by the compositing oracle (test infrastructure only).

The level-set identity.  Let T_k be the table whose entries k..255 are (1,1,1,1) and whose entries 0..k-1 are zero.  Under
the oracle's render with T_k a pixel's alpha byte is 255 iff some executed sample has index >= k: the first such sample
blends with factor 1 * (1 - 0), so alpha becomes exactly 1, and no later sample can change it; otherwise every sample
blends with factor 0 and the byte is 0.  Hence the per-pixel maximum M over the executed samples equals the number of k
in 1..255 whose frame has alpha 255 at that pixel -- no pixel of the oracle has to be touched to pin a MIP frame.

`sweep` checks the identity's own preconditions on every input it is given (alpha bytes in {0, 255}, hit sets monotone
in k); `assert_not_vacuous` adds the two conditions that keep a comparison against M from passing on an empty image."""
from __future__ import annotations

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
