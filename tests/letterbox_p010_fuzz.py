"""Seeded request generator for the differential fuzz of tsvpp_convert_letterbox_p010.  tests/test_gpu_letterbox_p010_fuzz.py runs every case on the GPU against
the model of tests/p010_util.py and sends the same cases through the describe call on the CPU.  Contains no product code and touches no device: numpy only.

cases() -> always the same list of CASES dicts of plain Python values:

    seed, index   np.random.default_rng(SEED) drew the whole list, `index` is the case's place in it
    canvas        (width, height): even, 8 .. 200 wide and 8 .. 120 high -- 4 k + 2 widths (the shifted last tile column) and widths below one tile among them
    frames        1 .. 5 of (width, height, layout): even, 2 .. 322 wide and 2 .. 182 high; layout = (luma offset, luma pitch - width, chroma offset, chroma
                  pitch - width) in WORDS, offsets of 0, 1, 2, 3, 5 and pitch increments of 0, 1, 3, 8 (tests/p010_cases.py embeds a frame at a layout)
    rects         None (the default rectangles) or one (left, top, width, height) per frame: even, inside the canvas, anywhere.  A quarter of the cases draw small
                  rectangles for large frames: footprints that exceed the launch's LDS, so the frame gathers
    mode          NEAREST or BILINEAR
    flavour       a name of p010_cases.FLAVOURS (all ten)
    aligned       outputs on a 16-byte boundary, or one element past it
    pad           (Y, U, V), each 0 .. 1023

Every case is legal by construction, so nothing is drawn again, the tests run exactly CASES cases and none is skipped: the model is defined for every one."""
import numpy as np

CASES = 40
SEED = 20261126
FLAVOURS = ("bf16_tensor", "f16_tensor", "f32_merged", "f32_planar", "f32_tensor", "u8_merged", "u8_planar", "y800_f16", "y800_f32", "y800_u8")
OFFSETS, PITCHES = (0, 1, 2, 3, 5), (0, 1, 3, 8)
ESIZE = {"u8": 1, "f32": 4, "f16": 2, "bf16": 2}


def _even(rng, lo, hi):
    return 2 * int(rng.integers((lo + 1) // 2, hi // 2 + 1))


def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def generate():
    rng = np.random.default_rng(SEED)
    out = []
    for index in range(CASES):
        kind = rng.random()
        if kind < 0.2:    # below one tile
            canvas = (_even(rng, 8, 30), _even(rng, 8, 30))
        elif kind < 0.5:  # 4 k + 2 columns
            canvas = (4 * int(rng.integers(2, 50)) + 2, _even(rng, 8, 120))
        else:
            canvas = (_even(rng, 8, 200), _even(rng, 8, 120))
        gather = rng.random() < 0.25
        frames = []
        for _ in range(int(rng.integers(1, 6))):
            w, h = (_even(rng, 200, 322), _even(rng, 120, 182)) if gather else (_even(rng, 2, 322), _even(rng, 2, 182))
            frames.append((w, h, (_pick(rng, OFFSETS), _pick(rng, PITCHES), _pick(rng, OFFSETS), _pick(rng, PITCHES))))
        rects = None
        if gather or rng.random() < 0.5:
            rects = []
            for _ in frames:
                rw, rh = (_even(rng, 2, min(16, canvas[0])), _even(rng, 2, min(12, canvas[1]))) if gather else (_even(rng, 2, canvas[0]), _even(rng, 2, canvas[1]))
                rects.append((_even(rng, 0, canvas[0] - rw), _even(rng, 0, canvas[1] - rh), rw, rh))
        out.append({"seed": SEED, "index": index, "canvas": canvas, "frames": frames, "rects": rects, "mode": int(rng.integers(0, 2)), "flavour": _pick(rng, FLAVOURS),
                    "aligned": bool(rng.random() < 0.5), "pad": tuple(int(v) for v in rng.integers(0, 1024, 3))})
    return out


def cases():
    return generate()


def element_size(flavour):
    return ESIZE[[t for t in flavour.split("_") if t in ESIZE][0]]


def byte_pitches(frame):
    w, _, layout = frame
    return 2 * (w + layout[1]), 2 * (w + layout[3])


def uv4(frame):
    """are the frame's chroma pairs 4-byte aligned: offset and pitch both even words"""
    w, _, layout = frame
    return layout[2] % 2 == 0 and (w + layout[3]) % 2 == 0


def host_frames(case):
    """[(y, uv)] of the case: tight uint16 planes of seeded random words"""
    out = []
    for k, (w, h, _) in enumerate(case["frames"]):
        rng = np.random.default_rng(case["seed"] + 100 * case["index"] + k)
        out.append((rng.integers(0, 65536, (h, w), dtype=np.uint16), rng.integers(0, 65536, (h // 2, w), dtype=np.uint16)))
    return out
