"""Seeded request generator for the differential fuzz of tsvpp_convert_letterbox_area.  tests/test_gpu_letterbox_area_fuzz.py runs every case on the GPU against the
oracle and sends the same cases through the describe call on the CPU.  Contains no product code and touches no device.

cases() -> always the same list of CASES dicts of plain Python values:

    seed, index   np.random.default_rng(seed) drew the whole list, `index` is the case's place in it
    canvas        (width, height): even, 2 .. 134 a side -- up to five tile columns, the shifted last column (4 k + 2 wide), canvases narrower than a tile
    frames        1 .. 4 of (width, height, pitch): even, 2 .. 420 a side, the pitch up to 62 bytes above the width
    rects         None (the default rectangles) or one (left, top, width, height) per frame: even, inside the canvas, anywhere
    flavour       (fourcc, planes, normalization) of letterbox_util.FLAVOURS
    tensor        None or (dtype, spec name of tensor_util.SPECS): only where the flavour allows one (planar or Y800, normalization)
    aligned       outputs on a 16-byte boundary, or one element past it
    pad           (Y, U, V)

Every case is legal by construction: a frame is drawn so that its rectangle never needs more than 40 taps on an axis (where the default rectangle would, the case
gets explicit rectangles), so nothing is drawn again and the tests run exactly CASES cases."""
import numpy as np

from letterbox_util import FLAVOURS, MERGED, PLANAR, Y800, default_rect
from tensor_util import DTYPES, SPECS

CASES = 36
SEED = 20261021
MAX_CANVAS, MAX_FRAME, MAX_TAPS = 134, 420, 40


def _even(rng, lo, hi):
    return 2 * int(rng.integers((lo + 1) // 2, hi // 2 + 1))


def taps_ok(frame, rect):
    """no axis needs more than MAX_TAPS taps: stated on the integer ratio, which bounds ceil of the float32 ratio from above"""
    return -(-frame[0] // rect[2]) <= MAX_TAPS and -(-frame[1] // rect[3]) <= MAX_TAPS


def _rect(rng, canvas, frame):
    cw, ch = canvas
    w = _even(rng, max(2, -(-frame[0] // MAX_TAPS)), cw)
    h = _even(rng, max(2, -(-frame[1] // MAX_TAPS)), ch)
    return (_even(rng, 0, cw - w), _even(rng, 0, ch - h), w, h)


def generate():
    rng = np.random.default_rng(SEED)
    out = []
    for index in range(CASES):
        small = rng.random() < 0.25
        canvas = (_even(rng, 2, 30 if small else MAX_CANVAS), _even(rng, 2, 30 if small else MAX_CANVAS))
        frames = []
        for _ in range(int(rng.integers(1, 5))):
            # (a rectangle side of `canvas` serves frames up to 40 times as large)
            w, h = _even(rng, 2, min(MAX_FRAME, MAX_TAPS * canvas[0] - 2)), _even(rng, 2, min(MAX_FRAME, MAX_TAPS * canvas[1] - 2))
            frames.append((w, h, w + _even(rng, 0, 62)))
        rects = None
        if rng.random() < 0.5 or not all(taps_ok(f, default_rect(f[0], f[1], *canvas)) for f in frames):
            rects = [_rect(rng, canvas, f) for f in frames]
        flavour = FLAVOURS[int(rng.integers(0, len(FLAVOURS)))]
        tensor = None
        if flavour[2] and (flavour[1] == PLANAR or flavour[0] == Y800) and rng.random() < 0.5:
            tensor = (DTYPES[int(rng.integers(0, len(DTYPES)))], sorted(SPECS)[int(rng.integers(0, len(SPECS)))])
        out.append({"seed": SEED, "index": index, "canvas": canvas, "frames": frames, "rects": rects, "flavour": flavour, "tensor": tensor,
                    "aligned": bool(rng.random() < 0.6), "pad": tuple(int(v) for v in rng.integers(0, 256, 3))})
    return out


def cases():
    return generate()


def host_frames(case):
    """[(y, uv)] of the case: seeded random planes at the frame's pitch -- or, where a test has set case["content"], that class of tests/edge_content.py"""
    if case.get("content"):
        import edge_content
        return [edge_content.frame(case["content"], w, h, p, p) for w, h, p in case["frames"]]
    from util import synth_nv12
    return [synth_nv12(w, h, seed=case["seed"] + 100 * case["index"] + k, pitch=p) for k, (w, h, p) in enumerate(case["frames"])]


def rects_of(case):
    return case["rects"] if case["rects"] is not None else [default_rect(f[0], f[1], *case["canvas"]) for f in case["frames"]]


def down_frames(case):
    """frames on the down-scale path: both float32 ratios above 1"""
    return sum(1 for f, r in zip(case["frames"], rects_of(case)) if np.float32(f[0]) / np.float32(r[2]) > 1 and np.float32(f[1]) / np.float32(r[3]) > 1)
