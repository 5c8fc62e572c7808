"""Reference frames for the batched renderer: rsoccer_amd/Render/raster.py itself, drawn on a padded canvas and cropped.

raster.py clamps the samples of a heading mark onto the window's border; the device renderer drops what falls outside the window
(include/rsx.h).  Drawing on a canvas that is `pad` pixels larger on every side and cropping it is exactly the drop rule: whatever
raster.py clamps lands in the padding.  Nothing else differs: the padded rasteriser is a FieldRaster whose centre moved by `pad`.
"""
import math
from types import SimpleNamespace

import numpy as np

from rsoccer_amd.Render import FieldRaster


class PaddedRaster:
    def __init__(self, view):
        base = FieldRaster(view)
        self.base = base
        self.pad = p = int(math.ceil(view["robot"] * view["scale"])) + 2
        r = FieldRaster.__new__(FieldRaster)
        r.v = dict(view)
        r.w, r.h = base.w + 2 * p, base.h + 2 * p
        r.cx, r.cy = base.cx + p, base.cy + p
        r.window_size = (r.w, r.h)
        r._yy, r._xx = np.mgrid[0:r.h, 0:r.w]
        r._field = np.pad(base._field, ((p, p), (p, p), (0, 0)))
        self.raster = r

    def draw(self, frame):
        p = self.pad
        return self.raster.draw(frame)[p:p + self.base.h, p:p + self.base.w]


def frames_of(state, n_blue, n_yellow, vss):
    """``state``: [rows, B] array in the engine's SoA layout (the env's own float32 values) -> one Frame-shaped namespace per env"""
    state = np.asarray(state)
    rs = 6 if vss else 11
    out = []
    for e in range(state.shape[1]):
        def robot(k):
            return SimpleNamespace(x=float(state[5 + rs * k, e]), y=float(state[6 + rs * k, e]), theta=float(state[7 + rs * k, e]))
        out.append(SimpleNamespace(
            ball=SimpleNamespace(x=float(state[0, e]), y=float(state[1, e])),
            robots_blue={i: robot(i) for i in range(n_blue)},
            robots_yellow={i: robot(n_blue + i) for i in range(n_yellow)}))
    return out


def reference_frames(view, state, n_blue, n_yellow, vss, env_ids=None):
    pr = PaddedRaster(view)
    frames = frames_of(state, n_blue, n_yellow, vss)
    ids = range(len(frames)) if env_ids is None else env_ids
    return np.stack([pr.draw(frames[i]) for i in ids])


def compare_frames(dev, ref, tag):
    """The condition of the renderer's tests.  float32 per-pixel evaluation against raster.py's float64 differs only where a pixel
    centre sits within rounding of a shape's edge: measured on the CPU, at most 1 pixel in a frame and at most 1 per 20 frames.
    So: a frame differs in at most 3 pixels; over the frames of one configuration at most one pixel per 4 frames differs; every
    differing pixel carries a colour the reference shows within its 3 x 3 neighbourhood.  Prints the figures, then asserts."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape and dev.dtype == np.uint8, (tag, dev.shape, ref.shape, dev.dtype)
    n, H, W, _ = ref.shape
    diff = (dev != ref).any(axis=3)
    per_frame = diff.reshape(n, -1).sum(axis=1)
    total = int(per_frame.sum())
    print(f"[render] {tag}: {n} frames of {H} x {W}, differing pixels {total}, worst frame {int(per_frame.max())}")
    assert per_frame.max() <= 3, (tag, "pixels differing in one frame", int(per_frame.max()), int(per_frame.argmax()))
    assert total * 4 <= n, (tag, "differing pixels", total, "frames", n)
    for f, y, x in zip(*np.nonzero(diff)):
        nb = ref[f, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(-1, 3)
        assert (nb == dev[f, y, x]).all(axis=1).any(), (tag, "colour foreign to the neighbourhood", int(f), int(y), int(x), dev[f, y, x].tolist())
    return total
