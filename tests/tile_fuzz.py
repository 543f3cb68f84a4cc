"""Seeded request generators for the differential fuzz of the tile-pipeline calls (tsvpp_convert_rois, tsvpp_convert_rois_area, tsvpp_convert_letterbox,
tsvpp_convert_warp, tsvpp_convert_perspective and their tensor forms).  tests/test_tile_fuzz_cpu.py checks what the generators reach, tests/test_gpu_tile_fuzz.py
runs every call on the GPU against the reference models.  Contains no product code and touches no device: numpy, the models' own rules and the CPU oracle.

cases(family, chunk) -> the calls of one (family, chunk), always the same list.  A call is a dict of plain Python values:

    family, seed, index      which call this is: np.random.default_rng(seed) drew the whole chunk, `index` is the call's place in it
    frames                   [{w, h, pitch_y, pitch_uv, off_y, off_uv, seed}]: picture size, the two pitches (drawn independently: w + one of PITCH_PADS), the bytes
                             a plane starts past a 16-byte boundary, the seed of its content (planes(), below)
    dst                      (width, height) of the output / the canvas
    flavour                  (fourcc, planes, normalization), one of letterbox_util.FLAVOURS
    tensor                   None, or (dtype, spec): names of tensor_util.DTYPES / tensor_util.SPECS -- the call goes through dtype= / mean= / std=
    rt                       the resize type (rois, letterbox: NEAREST / BILINEAR / BICUBIC; rois_area: AREA; warp, persp: BILINEAR)
    items                    rois, rois_area: (frame, left, top, right, bottom); letterbox: (frame, rect or None) -- one canvas per item, rect = (left, top, width,
                             height); warp: (frame, m0 .. m5); persp: (frame, h0 .. h8), float32 values
    pad / border             letterbox: (Y, U, V); warp, persp: None (replicate) or (Y, U, V)
    placement                "aligned": every output starts on a 16-byte boundary; "unaligned": every output starts one element past one (1, 2 or 4 bytes);
                             "mixed" (the split call): the outputs of the first launch group are aligned, the others are not
    split                    True for the one call per chunk with limit + 1 .. limit + 8 items: two launch groups, a vec and an elem kernel in one call

Whatever the library or a reference model would refuse -- an AREA down-scale box above 40 taps or one the oracle has no weight pattern for, a homography whose
horizon touches the output or that has no closed form, a matrix entry above 2^24 -- is drawn again HERE, and counted: generate() returns the counts beside the
calls, and tests/test_tile_fuzz_cpu.py holds the share of redraws under a tenth.  The GPU test therefore runs every call it is given."""
import math

import numpy as np

import persp_util as P
from letterbox_util import AREA, BICUBIC, BILINEAR, FLAVOURS, NEAREST, PLANAR, Y800
from tensor_util import DTYPES, ESIZE, SPECS, TORCH

FAMILIES = ("rois", "rois_area", "letterbox", "warp", "persp")
CHUNKS = 8
CALLS = 24                     # per (family, chunk)
BASE_SEED = 7402              # the seed of (family, chunk) is BASE_SEED + 8 * FAMILIES.index(family) + chunk
LIMIT = {"rois": 64, "rois_area": 64, "letterbox": 32, "warp": 32, "persp": 32}  # TSVPP_MAX_ROIS, _ROIS_AREA, _LETTERBOX, _WARPS, _PERSP
MAX_TAPS = 40                  # ROI_AREA_MAX_TAPS
MATRIX_BOUND = 2.0 ** 24
PITCH_PADS = (0, 0, 1, 2, 6, 16, 30)
GUARD = 64                     # bytes kept free before and after every output slot
F32 = np.float32


def seed_of(family, chunk):
    return BASE_SEED + 8 * FAMILIES.index(family) + chunk


# ---- draws ------------------------------------------------------------------------------------------------------------------------------------------------

def _even(rng, lo, hi):
    """an even number in [lo, hi]"""
    return 2 * int(rng.integers(lo // 2, hi // 2 + 1))


def _size(rng, max_w, max_h):
    """an even (width, height) in 2 .. max; a quarter of the draws are at most 16 a side"""
    if rng.random() < 0.25:
        max_w, max_h = min(max_w, 16), min(max_h, 16)
    return _even(rng, 2, max_w), _even(rng, 2, max_h)


def _triple(rng):
    return tuple(int(v) for v in rng.integers(0, 256, 3))


def _frame(rng):
    w, h = _size(rng, 320, 180)
    off = [0 if rng.random() < 0.5 else int(rng.integers(1, 16)) for _ in range(2)]
    return {"w": w, "h": h, "pitch_y": w + int(rng.choice(PITCH_PADS)), "pitch_uv": w + int(rng.choice(PITCH_PADS)), "off_y": off[0], "off_uv": off[1],
            "seed": int(rng.integers(0, 2 ** 31))}


def tensor_allowed(flavour):
    """the flavours the tensor entry points take: planar RGB24 / BGR24 or Y800, normalization=True"""
    fcc, planes, norm = flavour
    return bool(norm) and (fcc == Y800 or planes == PLANAR)


def area_taps(box, dst):
    """(down-scale?, taps on x, taps on y) of a box (left, top, right, bottom): the ratios as the library and the oracle form them, in float32"""
    xr, yr = F32(box[2] - box[0]) / F32(dst[0]), F32(box[3] - box[1]) / F32(dst[1])
    return bool(xr > 1 and yr > 1), int(math.ceil(float(xr))), int(math.ceil(float(yr)))


_pattern_ok = {}


def _oracle_has_pattern(scale):
    """does the oracle build the AREA weight pattern of this ratio (it gives up on one that does not repeat within its table)?"""
    key = float(scale)
    if key not in _pattern_ok:
        from oracle import oracle as O
        try:
            O.area_pattern(key)
            _pattern_ok[key] = True
        except RuntimeError:
            _pattern_ok[key] = False
    return _pattern_ok[key]


def _box(rng, fr, bw, bh):
    l, t = int(rng.integers(0, fr["w"] - bw + 1)), int(rng.integers(0, fr["h"] - bh + 1))  # odd origins allowed
    return (l, t, l + bw, t + bh)


def _roi(rng, frames, dst, stats):
    f = int(rng.integers(0, len(frames)))
    fr = frames[f]
    stats["draws"] += 1
    return (f,) + _box(rng, fr, _even(rng, 2, fr["w"]), _even(rng, 2, fr["h"]))


def _roi_area(rng, frames, dst, stats):
    """half of the boxes aim at the down-scale rule (both sides above the output's, up to a little past the tap cap; one in four of them goes for the largest tap
    count the frame allows), half at the up-scale rule (at least one side at most the output's): one call mixes the two"""
    while True:
        f = int(rng.integers(0, len(frames)))
        fr = frames[f]
        stats["draws"] += 1
        sides = []
        if rng.random() < 0.5:
            most = rng.random() < 0.25
            for full, d in ((fr["w"], dst[0]), (fr["h"], dst[1])):
                lo, hi = min(d + 2, full), min(full, 42 * d)
                sides.append(min(full, MAX_TAPS * d) if most else _even(rng, lo, hi))
        else:
            small = int(rng.integers(0, 3))  # which side stays at or below the output's: x, y or both
            for k, (full, d) in enumerate(((fr["w"], dst[0]), (fr["h"], dst[1]))):
                sides.append(_even(rng, 2, min(full, d)) if small in (k, 2) else _even(rng, 2, full))
        box = _box(rng, fr, sides[0], sides[1])
        down, tx, ty = area_taps(box, dst)
        if down and max(tx, ty) > MAX_TAPS:
            stats["over_the_tap_cap"] += 1
            continue
        if down and not (_oracle_has_pattern(F32(sides[0]) / F32(dst[0])) and _oracle_has_pattern(F32(sides[1]) / F32(dst[1]))):
            stats["refused_by_the_oracle"] += 1
            continue
        return (f,) + box


def _letterbox_item(rng, frames, dst, stats, own_rect):
    f = int(rng.integers(0, len(frames)))
    stats["draws"] += 1
    if not own_rect:
        return (f, None)
    # an even rectangle inside the canvas; one side in eight is 2
    w = 2 if rng.random() < 0.125 else _even(rng, 2, dst[0])
    h = 2 if rng.random() < 0.125 else _even(rng, 2, dst[1])
    return (f, (_even(rng, 0, dst[0] - w), _even(rng, 0, dst[1] - h), w, h))


def _matrix(rng, w, h, dw, dh, kind):
    """the distribution of test_warp_cpu.test_every_tap_of_a_tile_lies_inside_the_host_footprint: scales 0.3 .. 5, any angle, shear, and four kinds of
    translation -- centred; partly outside; wholly outside, near; thousands of pixels away"""
    sx, sy = rng.uniform(0.3, 5.0, 2)
    ang, shear = rng.uniform(0, 2 * math.pi), rng.uniform(-0.5, 0.5)
    c, s = math.cos(ang), math.sin(ang)
    a, b, d, e = sx * c, -sy * s + shear * sx * c, sx * s, sy * c + shear * sx * s
    cx = w / 2 + (0, rng.uniform(-w, w), rng.choice([-1, 1]) * (w + 400), rng.choice([-1, 1]) * 5000)[kind]
    cy = h / 2 + (0, rng.uniform(-h, h), rng.choice([-1, 1]) * (h + 400), rng.choice([-1, 1]) * 7000)[kind]
    return tuple(float(F32(v)) for v in (a, b, cx - a * dw / 2 - b * dh / 2, d, e, cy - d * dw / 2 - e * dh / 2))


def _warp(rng, frames, dst, stats, k):
    while True:
        f = int(rng.integers(0, len(frames)))
        stats["draws"] += 1
        m = _matrix(rng, frames[f]["w"], frames[f]["h"], dst[0], dst[1], k % 4)
        if max(abs(v) for v in m) > MATRIX_BOUND:
            stats["entry_above_2^24"] += 1
            continue
        return (f,) + m


def _persp(rng, frames, dst, stats, k):
    """the homography of the frame's corners, each moved by up to 0.3 of the frame size; every fourth quad is shifted half a frame outside, every eighth entry is
    the affine embedding of a drawn warp matrix; float32 values, as coord_paths.f32 rounds them"""
    while True:
        f = int(rng.integers(0, len(frames)))
        w, h = frames[f]["w"], frames[f]["h"]
        stats["draws"] += 1
        if k % 8 == 5:
            hm = P.affine(_matrix(rng, w, h, dst[0], dst[1], (k // 8) % 4))
        else:
            quad = [(x + rng.uniform(-0.3, 0.3) * w, y + rng.uniform(-0.3, 0.3) * h) for x, y in ((0, 0), (w, 0), (w, h), (0, h))]
            if k % 4 == 3:
                dx, dy = [(-0.5 * w, 0), (0.5 * w, 0), (0, -0.5 * h), (0, 0.5 * h)][int(rng.integers(0, 4))]
                quad = [(x + dx, y + dy) for x, y in quad]
            hm = P.from_quad(quad, dst[0], dst[1])
            if hm is None:
                stats["no_closed_form"] += 1
                continue
        hm = tuple(float(F32(v)) for v in hm)
        if not all(math.isfinite(v) for v in hm) or max(abs(v) for v in hm) > MATRIX_BOUND:
            stats["entry_above_2^24"] += 1
            continue
        if not P.in_domain(hm, dst[0], dst[1]):
            stats["out_of_domain"] += 1
            continue
        return (f,) + hm


# ---- calls ------------------------------------------------------------------------------------------------------------------------------------------------

def generate(family, chunk):
    """(calls, stats) of one (family, chunk); stats counts the item draws and, by reason, the ones that had to be drawn again"""
    assert family in FAMILIES and 0 <= chunk < CHUNKS
    seed = seed_of(family, chunk)
    rng = np.random.default_rng(seed)
    stats = {"draws": 0, "over_the_tap_cap": 0, "refused_by_the_oracle": 0, "no_closed_form": 0, "out_of_domain": 0, "entry_above_2^24": 0}
    split_at = int(rng.integers(0, CALLS))
    calls = []
    k = 0  # item counter of the chunk: the "every fourth / eighth" kinds of the warp and perspective draws
    for index in range(CALLS):
        split = index == split_at
        frames = [_frame(rng) for _ in range(int(rng.integers(1, 4)))]
        if split:
            # at most 16 x 16, and a width of 4 k: an output 4 k + 2 columns wide and narrower than a tile has no vector-store kernel (narrow_tail), and this
            # call is here to run one beside an element-wise one
            dst = (4 * int(rng.integers(1, 5)), _even(rng, 2, 16))
            n = LIMIT[family] + int(rng.integers(1, 9))
            placement = "mixed"
        else:
            dst = _size(rng, 160, 100)
            n = int(rng.integers(1, 9))
            placement = "aligned" if rng.random() < 0.5 else "unaligned"
        flavour = FLAVOURS[int(rng.integers(0, len(FLAVOURS)))]
        tensor = None
        if tensor_allowed(flavour) and rng.random() < 0.5:
            tensor = (DTYPES[int(rng.integers(0, len(DTYPES)))], sorted(SPECS)[int(rng.integers(0, len(SPECS)))])
        call = {"family": family, "seed": seed, "index": index, "frames": frames, "dst": dst, "flavour": flavour, "tensor": tensor, "placement": placement,
                "split": split}
        if family == "rois":
            call["rt"] = (NEAREST, BILINEAR, BICUBIC)[int(rng.integers(0, 3))]
            call["items"] = [_roi(rng, frames, dst, stats) for _ in range(n)]
        elif family == "rois_area":
            call["rt"] = AREA
            call["items"] = [_roi_area(rng, frames, dst, stats) for _ in range(n)]
        elif family == "letterbox":
            call["rt"] = (NEAREST, BILINEAR, BICUBIC)[int(rng.integers(0, 3))]
            own_rect = rng.random() < 0.5
            call["items"] = [_letterbox_item(rng, frames, dst, stats, own_rect) for _ in range(n)]
            call["pad"] = _triple(rng)
        else:
            call["rt"] = BILINEAR
            call["border"] = None if rng.random() < 0.5 else _triple(rng)
            draw = _warp if family == "warp" else _persp
            call["items"] = []
            for _ in range(n):
                call["items"].append(draw(rng, frames, dst, stats, k))
                k += 1
        calls.append(call)
    return calls, stats


def cases(family, chunk):
    return generate(family, chunk)[0]


# ---- what the tests make of a call ------------------------------------------------------------------------------------------------------------------------------

def planes(fr):
    """the content of a frame: (flat_y, flat_uv, y, uv) -- two flat uint8 buffers (to be placed on a 16-byte boundary) and the planes (rows x pitch) as views of
    them that start off_y / off_uv bytes in.  fr["content"], where a test has set it: a class of tests/edge_content.py in place of the seeded random bytes"""
    if fr.get("content"):
        import edge_content
        return edge_content.planes(fr["content"], fr)
    rng = np.random.default_rng(fr["seed"])
    out = []
    for rows, pitch, off in ((fr["h"], fr["pitch_y"], fr["off_y"]), (fr["h"] // 2, fr["pitch_uv"], fr["off_uv"])):
        flat = rng.integers(0, 256, off + rows * pitch + 16, dtype=np.uint8)
        out.append((flat, flat[off:off + rows * pitch].reshape(rows, pitch)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def host_frames(call):
    return [planes(fr) for fr in call["frames"]]


def device_frames(host, call):
    """every plane as a slice of a larger flat uint8 tensor: it starts off_y / off_uv bytes past a 16-byte boundary"""
    import torch
    dev = []
    for (flat_y, flat_uv, _, _), fr in zip(host, call["frames"]):
        pair = []
        for flat, rows, pitch, off in ((flat_y, fr["h"], fr["pitch_y"], fr["off_y"]), (flat_uv, fr["h"] // 2, fr["pitch_uv"], fr["off_uv"])):
            t = torch.from_numpy(flat).cuda()
            assert t.data_ptr() % 16 == 0
            pair.append(t[off:off + rows * pitch].view(rows, pitch))
            assert pair[-1].data_ptr() % 16 == off
        dev.append(tuple(pair))
    return dev


def geometry(call):
    """the frames as the describe functions take them"""
    return [(f["w"], f["h"], f["pitch_y"], f["pitch_uv"]) for f in call["frames"]]


def element_bytes(call):
    if call["tensor"] is not None:
        return ESIZE[call["tensor"][0]]
    return 4 if call["flavour"][2] else 1


def output_bytes(call):
    return (1 if call["flavour"][0] == Y800 else 3) * call["dst"][0] * call["dst"][1] * element_bytes(call)


def slot_starts(call):
    """(starts, total): the byte offset of every output in one buffer that begins on a 16-byte boundary, GUARD free bytes before and after every output, placed as
    call["placement"] says; total = the buffer's size"""
    nbytes, esz, limit = output_bytes(call), element_bytes(call), LIMIT[call["family"]]
    starts, pos = [], 0
    for i in range(len(call["items"])):
        aligned = call["placement"] == "aligned" or (call["placement"] == "mixed" and i < limit)
        start = (pos + GUARD + 15) // 16 * 16 + (0 if aligned else esz)
        starts.append(start)
        pos = start + nbytes
    return starts, pos + GUARD


def tensor_kwargs(call):
    """dtype= / mean= / std= of the call ({} without a tensor form)"""
    if call["tensor"] is None:
        return {}
    dtype, spec = call["tensor"]
    return {"dtype": TORCH[dtype], "mean": SPECS[spec][0], "std": SPECS[spec][1]}


def frame_parameters(ts, call):
    fcc, planes_pos, norm = call["flavour"]
    return ts.FrameParameters(width=call["dst"][0], height=call["dst"][1], resize_type=call["rt"], pixel_format=fcc, planes_pos=planes_pos, normalization=norm)


def letterbox_rects(call):
    """rects= of a letterbox call: None (the default rectangle for every canvas) or one per item"""
    rects = [r for _, r in call["items"]]
    return None if rects[0] is None else rects


def describe(call, aligned_outputs=None):
    """what the call would launch (ts.describe_* of its family: host logic only); aligned_outputs: default as drawn -- the first launch group's placement"""
    import tensor_stream as ts
    if aligned_outputs is None:
        aligned_outputs = call["placement"] != "unaligned"
    fp, geo, kw = frame_parameters(ts, call), geometry(call), dict(aligned_outputs=aligned_outputs, **tensor_kwargs(call))
    family = call["family"]
    if family == "rois":
        return ts.describe_rois(fp, geo, call["items"], **kw)
    if family == "rois_area":
        return ts.describe_rois_area(fp, geo, call["items"], **kw)
    if family == "letterbox":
        return ts.describe_letterbox(fp, [geo[f] for f, _ in call["items"]], rects=letterbox_rects(call), **kw)
    if family == "warp":
        return ts.describe_warp(fp, geo, call["items"], border=call["border"], **kw)
    return ts.describe_perspective(fp, geo, call["items"], border=call["border"], **kw)
