"""Writes tests/golden/tile_describe_snapshot.json: the full answer of describe_rois, describe_rois_area, describe_letterbox and their tensor forms (kernel,
launches, grid, LDS bytes, staged items, store policy, ...) for ~300 requests, or the status where a request is refused.  The three paths share one tile
pipeline on the host (tsvpp_tiles.h); the CPU suite compares the live answers with this file (tests/test_tile_describe_snapshot_cpu.py), so a change to the
launch fill, the staging budget, the launch split or a request rule shows up in review as a diff of this file:
    python tests/golden/make_tile_describe_snapshot.py        # regenerate after an intended change
Host logic only (no GPU)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tensor-stream_amd"))

import torch  # noqa: E402
import tensor_stream as ts  # noqa: E402
from tensor_stream import vpp  # noqa: E402

RT = {"NEAREST": 0, "BILINEAR": 1, "BICUBIC": 2, "AREA": 3}
FCC = {"Y800": 0, "RGB24": 1, "BGR24": 2, "NV12": 3}
FLAVOURS = [("RGB24", "PLANAR", False), ("BGR24", "MERGED", False), ("RGB24", "PLANAR", True), ("BGR24", "MERGED", True), ("Y800", "MERGED", False),
            ("Y800", "MERGED", True)]
MERGED = [("BGR24", "MERGED", False), ("BGR24", "MERGED", True)]  # the two flavours with static LDS and a store policy of their own
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# 4 k sizes, 70 x 66 (4 k + 2, as wide as a tile or wider: the shifted last tile column), 30 x 34 (4 k + 2, narrower than a tile: no vector stores)
SIZES = [(224, 224), (112, 112), (640, 640), (70, 66), (30, 34)]
FRAME = (1920, 1080, 2048)


def boxes(n):
    """n boxes of a 1920 x 1080 frame, 64 x 64 up to 1280 x 720, even everywhere: the small ones stage their tiles in LDS, the large ones gather."""
    sizes = [(64, 64), (128, 96), (200, 300), (320, 240), (512, 512), (640, 360), (960, 540), (1280, 720)]
    out = []
    for i in range(n):
        w, h = sizes[i % len(sizes)]
        left, top = (2 * 37 * i) % (1920 - w + 2) & ~1, (2 * 53 * i) % (1080 - h + 2) & ~1
        out.append((left, top, left + w, top + h))
    return out


def lb_frames(n):
    """n frames, portrait and landscape, with pitches of their own"""
    kinds = [(1920, 1080, 2048), (1080, 1920, 1088), (1280, 720, 1280), (720, 1280, 768), (640, 480, 640), (480, 640, 512)]
    return [kinds[i % len(kinds)] for i in range(n)]


def lb_rects(n, dst):
    """given rectangles: even, inside the canvas, not the default ones"""
    w, h = dst
    out = []
    for i in range(n):
        rw, rh = max(2, (w * (3 + i % 4) // 8) & ~1), max(2, (h * (2 + i % 5) // 8) & ~1)
        out.append((((w - rw) // (1 + i % 3)) & ~1, ((h - rh) // (1 + i % 2)) & ~1, rw, rh))
    return out


def params(dst, rt, fcc, planes, norm, crop=(0, 0, 0, 0)):
    return ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=RT[rt], pixel_format=FCC[fcc], planes_pos=0 if planes == "PLANAR" else 1,
                              normalization=norm)


def answer(fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except RuntimeError as e:  # a refused request: its status
        return {"error": str(e).split(":")[0]}


def name(path, dst, rt, fl, aligned, what, dtype=None):
    return f"{path} {what} ->{dst[0]}x{dst[1]} {rt} {fl[0]} {fl[1]} {'f32' if fl[2] else 'u8'} {'aligned' if aligned else 'unaligned'}" + (f" {dtype}" if dtype else "")


def rois(snap, dst, rt, fl, aligned, n, dtype=None, **kw):
    """n = 0: one 1280 x 720 box alone, whose tiles fit no LDS budget at a small output (the gather kernel)"""
    fn = vpp.describe_rois_area if rt == "AREA" else vpp.describe_rois
    bx = boxes(n) if n else [(320, 180, 1600, 900)]
    snap[name("rois", dst, rt, fl, aligned, f"{n}boxes" if n else "1largebox", dtype)] = answer(fn, params(dst, rt, *fl), FRAME, bx, aligned_outputs=aligned,
                                                                                            dtype=DTYPES[dtype] if dtype else None, **kw)


def letterbox(snap, dst, rt, fl, aligned, n, given, dtype=None):
    frames = lb_frames(n) if n > 1 else [FRAME]
    snap[name("letterbox", dst, rt, fl, aligned, f"{n}frames{'+rects' if given else ''}", dtype)] = answer(
        vpp.describe_letterbox, params(dst, rt, *fl), frames, rects=lb_rects(n, dst) if given else None, aligned_outputs=aligned, dtype=DTYPES[dtype] if dtype else None)


def refused(snap):
    P = ("RGB24", "PLANAR", True)
    one = boxes(1)
    # ROIs
    snap["refused rois ERROR box outside its frame"] = answer(vpp.describe_rois, params((224, 224), "BILINEAR", *P), FRAME, [(0, 0, 1922, 64)])
    snap["refused rois ERROR crop in the parameters"] = answer(vpp.describe_rois, params((224, 224), "BILINEAR", *P, crop=(0, 0, 64, 64)), FRAME, one)
    snap["refused rois UNSUPPORTED odd box"] = answer(vpp.describe_rois, params((224, 224), "BILINEAR", *P), FRAME, [(0, 0, 63, 64)])
    snap["refused rois UNSUPPORTED AREA"] = answer(vpp.describe_rois, params((224, 224), "AREA", *P), FRAME, one)
    snap["refused rois UNSUPPORTED NV12"] = answer(vpp.describe_rois, params((224, 224), "BILINEAR", "NV12", "MERGED", False), FRAME, one)
    snap["refused rois ERROR wins over UNSUPPORTED"] = answer(vpp.describe_rois, params((223, 224), "BILINEAR", *P), FRAME, [(0, 0, 1922, 64)])
    # AREA ROIs
    snap["refused rois_area ERROR frame index"] = answer(vpp.describe_rois_area, params((224, 224), "AREA", *P), FRAME, [(1, 0, 0, 64, 64)])
    snap["refused rois_area UNSUPPORTED BILINEAR"] = answer(vpp.describe_rois_area, params((224, 224), "BILINEAR", *P), FRAME, one)
    snap["refused rois_area UNSUPPORTED more than 40 taps"] = answer(vpp.describe_rois_area, params((30, 34), "AREA", *P), FRAME, [(0, 0, 1920, 1080)])
    snap["refused rois_area UNSUPPORTED odd output"] = answer(vpp.describe_rois_area, params((225, 224), "AREA", *P), FRAME, one)
    # letterbox
    snap["refused letterbox ERROR rectangle outside the canvas"] = answer(vpp.describe_letterbox, params((640, 640), "BILINEAR", *P), [FRAME], rects=[(320, 0, 640, 360)])
    snap["refused letterbox ERROR pitch below the width"] = answer(vpp.describe_letterbox, params((640, 640), "BILINEAR", *P), [(1920, 1080, 1000)])
    snap["refused letterbox UNSUPPORTED AREA"] = answer(vpp.describe_letterbox, params((640, 640), "AREA", *P), [FRAME])
    snap["refused letterbox UNSUPPORTED odd rectangle"] = answer(vpp.describe_letterbox, params((640, 640), "BILINEAR", *P), [FRAME], rects=[(1, 0, 320, 180)])
    snap["refused letterbox UNSUPPORTED odd frame"] = answer(vpp.describe_letterbox, params((640, 640), "BILINEAR", *P), [(1919, 1080, 2048)])
    # tensor forms: the plan's status first, then the spec's
    for path, fn, extra in (("rois", vpp.describe_rois, (FRAME, one)), ("rois_area", vpp.describe_rois_area, (FRAME, one)), ("letterbox", vpp.describe_letterbox, ([FRAME],))):
        rt = "AREA" if path == "rois_area" else "BILINEAR"
        snap[f"refused {path} tensor ERROR std of zero"] = answer(fn, params((224, 224), rt, *P), *extra, dtype=torch.float16, std=0.0)
        snap[f"refused {path} tensor UNSUPPORTED without normalization"] = answer(fn, params((224, 224), rt, "RGB24", "PLANAR", False), *extra, dtype=torch.float16)
        snap[f"refused {path} tensor UNSUPPORTED merged"] = answer(fn, params((224, 224), rt, "RGB24", "MERGED", True), *extra, dtype=torch.float16)
        snap[f"refused {path} tensor plan status wins"] = answer(fn, params((223, 224), rt, *P), *extra, dtype=torch.float16, std=0.0)


def snapshot():
    snap = {}
    for rt in RT:
        # every flavour, and every size x alignment with the merged flavours
        for fl in FLAVOURS:
            rois(snap, (224, 224), rt, fl, True, 8)
        for dst in SIZES:
            for fl in MERGED:
                for aligned in (True, False):
                    rois(snap, dst, rt, fl, aligned, 8)
        # 2 and 3 launches (AREA: 33 boxes too)
        for n in (65, 129) + ((33,) if rt == "AREA" else ()):
            rois(snap, (112, 112), rt, FLAVOURS[0], True, n)
        # tensor forms: every dtype, planar and Y800; every size x alignment in fp16
        for dt in DTYPES:
            for fl in (FLAVOURS[2], FLAVOURS[5]):
                rois(snap, (224, 224), rt, fl, True, 8, dt, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
        for dst in SIZES[1:]:
            for aligned in (True, False):
                rois(snap, dst, rt, FLAVOURS[2], aligned, 8, "f16")
        rois(snap, (112, 112), rt, FLAVOURS[2], True, 65, "bf16")
        rois(snap, (70, 66), rt, FLAVOURS[1], True, 0)
        rois(snap, (70, 66), rt, FLAVOURS[2], False, 0, "f32")
        if rt == "AREA":
            continue
        for fl in FLAVOURS:
            letterbox(snap, (640, 640), rt, fl, True, 1, False)
        for dst in SIZES:
            for fl in MERGED:
                for aligned in (True, False):
                    letterbox(snap, dst, rt, fl, aligned, 3, dst != (640, 640))
        letterbox(snap, (640, 640), rt, FLAVOURS[0], True, 33, False)
        letterbox(snap, (224, 224), rt, FLAVOURS[3], False, 33, True)
        for dt in DTYPES:
            for fl in (FLAVOURS[2], FLAVOURS[5]):
                letterbox(snap, (640, 640), rt, fl, True, 1, False, dt)
        for dst in SIZES:
            letterbox(snap, dst, rt, FLAVOURS[2], dst[0] % 4 == 0, 33, True, "f16")
            letterbox(snap, dst, rt, FLAVOURS[2], dst[0] % 4 != 0, 2, False, "bf16")
    refused(snap)
    return snap


if __name__ == "__main__":
    snap = snapshot()
    with open(os.path.join(HERE, "tile_describe_snapshot.json"), "w") as f:
        json.dump(snap, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(snap), "requests")
