"""Writes tests/golden/coord_describe_snapshot.json: the full answer of describe_warp, describe_perspective, describe_remap, describe_mesh and their tensor
forms (kernel, launches, grid, LDS bytes, staged items, store policy, border, ...) for 277 requests, or the status where a request is refused.  The four paths
are one path with a different source coordinate and share their host side (tsvpp_tiles.h, the request skeleton of tsvpp_plan.cpp); the CPU suite compares the
live answers with this file (tests/test_coord_describe_snapshot_cpu.py), so a change to the launch fill, a staging budget, the launch split or the order of the
request rules shows up in review as a diff of this file:
    python tests/golden/make_coord_describe_snapshot.py        # regenerate after an intended change
Host logic only (no GPU)."""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tensor-stream_amd"))

import torch  # noqa: E402
import tensor_stream as ts  # noqa: E402
from tensor_stream import vpp  # noqa: E402
from tensor_stream import _native as N  # noqa: E402

RT = {"NEAREST": 0, "BILINEAR": 1, "BICUBIC": 2, "AREA": 3}
FCC = {"Y800": 0, "RGB24": 1, "BGR24": 2, "NV12": 3}
FLAVOURS = [("RGB24", "PLANAR", False), ("BGR24", "MERGED", False), ("RGB24", "PLANAR", True), ("BGR24", "MERGED", True), ("Y800", "MERGED", False),
            ("Y800", "MERGED", True)]
MERGED = [("BGR24", "MERGED", False), ("BGR24", "MERGED", True)]  # the two flavours with static LDS and a store policy of their own
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# 4 k sizes, 70 x 66 (4 k + 2, as wide as a tile or wider: the shifted last tile column), 30 x 34 (4 k + 2, narrower than a tile: no vector stores)
SIZES = [(112, 112), (640, 640), (70, 66), (30, 34)]
FRAME = (1920, 1080, 2048)
BORDERS = [None, (16, 128, 128)]
LIMITS = {"warp": N.TSVPP_MAX_WARPS, "perspective": N.TSVPP_MAX_PERSP, "remap": N.TSVPP_MAX_REMAPS, "mesh": N.TSVPP_MAX_MESHES}
PATHS = list(LIMITS)
P = ("RGB24", "PLANAR", True)
# (name, centre x, centre y, box width, box height, angle): an axis-aligned 64 x 64 box, where every tile stages; the same box rotated by 30 degrees; 1280 x 720
# pixels, of which at 70 x 66 only the two rows of the last tile row fit the LDS budget (staged and gathering tiles in one launch)
BOXES = {"box64": (400.0, 300.0, 64.0, 64.0, 0.0), "box64rot30": (400.0, 300.0, 64.0, 64.0, math.pi / 6), "box1280x720": (960.0, 540.0, 1280.0, 720.0, 0.0)}


def params(dst, rt, fcc, planes, norm):
    return ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=(0, 0, 0, 0), resize_type=RT[rt], pixel_format=FCC[fcc], planes_pos=0 if planes == "PLANAR" else 1,
                              normalization=norm)


def answer(fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except RuntimeError as e:  # a refused request: its status
        return {"error": str(e).split(":")[0]}


def matrix(box, dst, k=0):
    """the k-th copy of a box, shifted by a few even pixels, as an affine matrix"""
    cx, cy, w, h, a = BOXES[box]
    return vpp.warp_rotated_box(cx + 2 * 37 * k % 200, cy + 2 * 53 * k % 100, w, h, a, dst[0], dst[1])


def homography(box, dst, k=0):
    """... as the homography of the same box with its top edge drawn in by an eighth of its width on both sides: a keystone, no affine map"""
    cx, cy, w, h, a = BOXES[box]
    cx, cy = cx + 2 * 37 * k % 200, cy + 2 * 53 * k % 100
    c, s = math.cos(a), math.sin(a)
    quad = [(cx + x * c - y * s, cy + x * s + y * c) for x, y in ((-0.375 * w, -0.5 * h), (0.375 * w, -0.5 * h), (0.5 * w, 0.5 * h), (-0.5 * w, 0.5 * h))]
    return vpp.perspective_from_quad(quad, dst[0], dst[1])


def ask(path, dst, rt, fl, aligned, n=8, box="box64", grids=((0, 0),), cell=(16, 16), frames=FRAME, remaps=None, items=None, **kw):
    """One request of `path`: n items of one frame.  Matrix paths: n copies of `box` (or `items`); map paths: `grids` = (pitch, lds_bytes) per map or mesh, the
    n outputs take them in turn (or `remaps`)."""
    p = params(dst, rt, *fl)
    if path == "warp":
        return answer(vpp.describe_warp, p, frames, items if items is not None else [matrix(box, dst, k) for k in range(n)], aligned_outputs=aligned, **kw)
    if path == "perspective":
        return answer(vpp.describe_perspective, p, frames, items if items is not None else [homography(box, dst, k) for k in range(n)], aligned_outputs=aligned, **kw)
    rs = remaps if remaps is not None else [(0, k % len(grids)) for k in range(n)]
    if path == "remap":
        return answer(vpp.describe_remap, p, frames, list(grids), remaps=rs, aligned_outputs=aligned, **kw)
    return answer(vpp.describe_mesh, p, frames, list(grids), cell=cell, remaps=rs, aligned_outputs=aligned, **kw)


def name(path, dst, rt, fl, aligned, what, dtype=None):
    return f"{path} {what} ->{dst[0]}x{dst[1]} {rt} {fl[0]} {fl[1]} {'f32' if fl[2] else 'u8'} {'aligned' if aligned else 'unaligned'}" + (f" {dtype}" if dtype else "")


def accepted(snap, path):
    B, D = "BILINEAR", (224, 224)
    matrix_path = path in ("warp", "perspective")
    for fl in FLAVOURS:
        snap[name(path, D, B, fl, True, "8items")] = ask(path, D, B, fl, True)
    for dst in SIZES:
        for fl in MERGED:
            for aligned in (True, False):
                snap[name(path, dst, B, fl, aligned, "8items")] = ask(path, dst, B, fl, aligned)
    # 1 item, and 2 and 3 launches
    for n in (1, 8, LIMITS[path] + 1, 2 * LIMITS[path] + 1):
        snap[name(path, (112, 112), B, FLAVOURS[0], True, f"{n}items")] = ask(path, (112, 112), B, FLAVOURS[0], True, n=n)
    # tensor forms: every dtype, planar and Y800
    for dt in DTYPES:
        for fl in (FLAVOURS[2], FLAVOURS[5]):
            snap[name(path, D, B, fl, True, "8items", dt)] = ask(path, D, B, fl, True, dtype=DTYPES[dt], mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    snap[name(path, (70, 66), B, FLAVOURS[2], False, "33items border", "bf16")] = ask(path, (70, 66), B, FLAVOURS[2], False, n=33, box="box1280x720", border=BORDERS[1], dtype=torch.bfloat16)
    for border in BORDERS:
        bn = "replicate" if border is None else "border"
        if matrix_path:
            for box in BOXES:
                dst = (70, 66) if box == "box1280x720" else D
                snap[name(path, dst, B, P, True, f"3items {box} {bn}")] = ask(path, dst, B, P, True, n=3, box=box, border=border)
            if border is None:  # ... and at 64 x 64, where no tile fits: colour, and tensor with the border
                snap[name(path, (64, 64), B, P, True, "3items box1280x720 replicate")] = ask(path, (64, 64), B, P, True, n=3, box="box1280x720")
                snap[name(path, (64, 64), B, P, False, "3items box1280x720 border", "f16")] = ask(path, (64, 64), B, P, False, n=3, box="box1280x720", border=BORDERS[1],
                                                                                                 dtype=torch.float16)
            continue
        # an LDS hint or none; two maps (meshes) with different hints in one launch: the launch takes the larger; one of them without a hint: the budget
        for what, grids in (("nohint", ((0, 0),)), ("hint", ((0, 20480),)), ("2hints", ((0, 8192), (0, 20480))), ("hint+nohint", ((0, 8192), (0, 0))),
                            ("hint above the budget", ((0, 1 << 20),))):
            snap[name(path, D, B, P, True, f"8items {what} {bn}")] = ask(path, D, B, P, True, grids=grids, border=border)
        snap[name(path, D, B, MERGED[1], False, f"8items hint padded pitch {bn}")] = ask(path, D, B, MERGED[1], False, grids=((8 * 224 + 64, 4096),), border=border)
    if path == "mesh":
        for cell in ((4, 4), (16, 16), (256, 256), (4, 256)):
            snap[name(path, (70, 66), B, P, True, f"8items cell {cell[0]}x{cell[1]}")] = ask(path, (70, 66), B, P, True, cell=cell, grids=((0, 4096),))
        snap[name(path, D, B, P, True, "8items 2 cells")] = ask(path, D, B, P, True, cell=[(8, 32), (64, 4)], grids=((0, 0), (0, 0)))


def refused(snap, path):
    """One refused request per rule of the shared skeleton and of the path, in the skeleton's order; `+`: two faults, to show which status wins"""
    B, D = "BILINEAR", (224, 224)
    matrix_path = path in ("warp", "perspective")
    K = 6 if path == "warp" else 9
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)[:K]

    def put(what, dst=D, rt=B, fl=P, **kw):
        snap[f"refused {path} {what}"] = ask(path, dst, rt, fl, True, **kw)

    def entry(k, v):
        return [ident[:k] + (v,) + ident[k + 1:]]

    if matrix_path:
        put("ERROR frame index", items=[(1,) + ident])
        put("ERROR frame index + UNSUPPORTED odd output", dst=(223, 224), items=[(-1,) + ident])
    else:
        put("ERROR frame index", remaps=[(0, 0), (1, 0)])
        put("ERROR map index", remaps=[(0, 1)])
        put("ERROR frame index + UNSUPPORTED odd output", dst=(223, 224), remaps=[(-1, 0)])
    put("ERROR border -1,0,0", border=(-1, 0, 0))
    put("ERROR border 256", border=(16, 256, 128))
    put("ERROR border 256 + UNSUPPORTED NEAREST", rt="NEAREST", border=(256, 128, 128))
    if matrix_path:
        put("ERROR non-finite entry", items=entry(2, float("nan")))
        put("ERROR infinite last entry", items=entry(K - 1, float("inf")))
        put("ERROR non-finite entry + UNSUPPORTED odd frame", frames=(1919, 1080, 2048), items=entry(0, float("-inf")))
    else:
        put("ERROR pitch below the row", grids=((8 * (15 if path == "mesh" else 224) - 8, 0),))  # (mesh: 15 control points per row at cell 16)
        put("ERROR pitch no multiple of 8", grids=((8 * 224 + 4, 0),))
        put("ERROR negative hint", grids=((0, -1),))
        put("ERROR negative hint in the second grid + UNSUPPORTED AREA", rt="AREA", grids=((0, 0), (0, -16)))
    put("ERROR frame pitch below the width", frames=(1920, 1080, 1000))
    put("UNSUPPORTED odd frame", frames=(1919, 1080, 2048))
    put("UNSUPPORTED odd frame height", frames=(1920, 1079, 2048))
    put("UNSUPPORTED odd output", dst=(224, 223))
    put("UNSUPPORTED NEAREST", rt="NEAREST")
    put("UNSUPPORTED BICUBIC", rt="BICUBIC")
    put("UNSUPPORTED AREA", rt="AREA")
    put("UNSUPPORTED NV12", fl=("NV12", "MERGED", False))
    if matrix_path:
        put("UNSUPPORTED entry above 2^24", items=entry(2, 16777218.0))
        put("UNSUPPORTED entry below -2^24 + UNSUPPORTED NEAREST", rt="NEAREST", items=entry(K - 1 if path == "warp" else 5, -33554432.0))
        snap[f"{path} accepted: an entry of exactly 2^24"] = ask(path, D, B, P, True, items=entry(2, 16777216.0))
    if path == "perspective":
        put("UNSUPPORTED horizon inside the output", items=[(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0 / 112, 0.0, 1.0)])
        put("UNSUPPORTED horizon in the last row", items=[(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, -1.0 / 223.5, 1.0)])
        put("ERROR border 300 + UNSUPPORTED horizon", items=[(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0 / 112, 0.0, 1.0)], border=(0, 0, 300))
        put("UNSUPPORTED negative denominator", items=[ident[:8] + (-1.0,)])
    if path == "mesh":
        put("UNSUPPORTED cell exponent 1", cell=(2, 16))
        put("UNSUPPORTED cell exponent 9", cell=(16, 512))
        put("ERROR negative hint + UNSUPPORTED cell exponent 9", cell=(512, 16), grids=((0, -1),))
        put("ERROR pitch no multiple of 8 + UNSUPPORTED cell exponent 1", cell=(2, 2), grids=((100, 0),))
        put("UNSUPPORTED cell exponent 1: no pitch rule", cell=(2, 2), grids=((8, 0),))
        put("UNSUPPORTED cell exponent 9 + UNSUPPORTED odd output", dst=(223, 224), cell=(512, 512))
    # tensor forms: the plan's status first, then the spec's
    snap[f"refused {path} tensor ERROR std of zero"] = ask(path, D, B, P, True, dtype=torch.float16, std=0.0)
    snap[f"refused {path} tensor UNSUPPORTED without normalization"] = ask(path, D, B, ("RGB24", "PLANAR", False), True, dtype=torch.float16)
    snap[f"refused {path} tensor UNSUPPORTED merged"] = ask(path, D, B, ("RGB24", "MERGED", True), True, dtype=torch.float16)
    snap[f"refused {path} tensor UNSUPPORTED odd output wins over the std of zero"] = ask(path, (223, 224), B, P, True, dtype=torch.float16, std=0.0)


def snapshot():
    snap = {}
    for path in PATHS:
        accepted(snap, path)
        refused(snap, path)
    return snap


if __name__ == "__main__":
    snap = snapshot()
    with open(os.path.join(HERE, "coord_describe_snapshot.json"), "w") as f:
        json.dump(snap, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(snap), "requests")
