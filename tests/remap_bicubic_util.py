"""The model of the BICUBIC map calls (include/tsvpp.h): the coordinate of tests/remap_util.py through the cubic sample of tests/warp_bicubic_util.py, and the
footprint formula restated.  No product code.  Its judge is tests/sampler64_cubic.py (tests/test_remap_bicubic_cpu.py)."""
import numpy as np

import remap_util as R
import warp_bicubic_util as B
import warp_util as W


def virtual_frame_from_map(y, uv, w, h, xy, border=None):
    """the dst_w x dst_h NV12 frame the map samples BICUBIC out of the w x h frame (y, uv: planes with any pitch)"""
    fx, fy, cfx, cfy = R.coords(xy, w, h)
    cw, ch = w // 2, h // 2
    planes = [B.sample(y, fx, fy, w, h), B.sample(uv, cfx, cfy, cw, ch, step=2, comp=0), B.sample(uv, cfx, cfy, cw, ch, step=2, comp=1)]
    if border is not None:
        out = [W.outside(fx, w) | W.outside(fy, h), W.outside(cfx, cw) | W.outside(cfy, ch)]
        planes = [np.where(out[min(k, 1)], border[k], v) for k, v in enumerate(planes)]
    UV = np.empty((xy.shape[0] // 2, xy.shape[1]), np.uint8)
    UV[:, 0::2], UV[:, 1::2] = planes[1], planes[2]
    return planes[0].astype(np.uint8), UV


def tile_boxes(xy, w, h, tile):
    """of the tile (j_first, j_last, i_first, i_last), eight numbers each (lo, hi per axis: luma x, y, chroma x, y): the hull of the tap indices the model touches,
    and the header's footprint -- [P(min) - 1, P(max) + 2] clamped into the plane, P the floor clamped into 0 .. limit - 1"""
    j0, j1, i0, i1 = tile
    fx, fy, cfx, cfy = R.coords(xy, w, h)
    luma, chroma = (slice(i0, i1 + 1), slice(j0, j1 + 1)), (slice(i0 >> 1, (i1 >> 1) + 1), slice(j0 >> 1, (j1 >> 1) + 1))
    hull, box = [], []
    for f, limit in ((fx[luma], w), (fy[luma], h), (cfx[chroma], w // 2), (cfy[chroma], h // 2)):
        t = B.tap_indices(B.axis(f, limit)[0], limit)
        hull += [int(t[0].min()), int(t[3].max())]
        p = np.clip(np.floor([f.min(), f.max()]).astype(int), 0, limit - 1)
        box += [max(int(p[0]) - 1, 0), min(int(p[1]) + 2, limit - 1)]
    return tuple(hull), tuple(box)
