"""Seeded request generator for the differential fuzz of tsvpp_convert_rois_sized and its tensor form, in the conventions of tests/tile_fuzz.py (whose frame
draw, plane content and flavour list it uses).  tests/test_gpu_rois_sized_fuzz.py runs every call on the GPU against the oracle.  Contains no product code and
touches no device.

cases(chunk) -> the calls of one chunk, always the same list.  A call is a dict of plain Python values:

    seed, index      np.random.default_rng(seed) drew the whole chunk, `index` is the call's place in it
    frames           1 .. 3 of tile_fuzz's frames: 2 x 2 .. 320 x 180, the two pitches drawn independently, planes that start anywhere
    flavour, tensor  as tile_fuzz's: (fourcc, planes, normalization); None or (dtype, spec)
    rt               NEAREST / BILINEAR / BICUBIC
    items            1 .. 60 boxes (frame, left, top, right, bottom), odd origins allowed
    sizes            one (width, height) per box: even, 2 .. 160 x 2 .. 100; a quarter of them at most 16 a side
    placement        "aligned" / "unaligned" (one element past a 16-byte boundary) / "mixed": `aligned` holds one drawn bool per output -- the two-class split

Every drawn request is legal by construction -- boxes lie inside their frames with even sides, sizes are even and positive -- so nothing is drawn again and the
GPU test runs exactly CHUNKS * CALLS calls."""
import numpy as np

import tile_fuzz as F
from letterbox_util import BICUBIC, BILINEAR, FLAVOURS, NEAREST
from tensor_util import DTYPES, ESIZE, SPECS

CHUNKS = 3
CALLS = 8
BASE_SEED = 8117  # the seed of a chunk is BASE_SEED + chunk
MAX_BOXES = 60    # above TSVPP_MAX_ROIS_SIZED: some calls take a second launch of a class


def generate(chunk):
    assert 0 <= chunk < CHUNKS
    seed = BASE_SEED + chunk
    rng = np.random.default_rng(seed)
    calls = []
    for index in range(CALLS):
        frames = [F._frame(rng) for _ in range(int(rng.integers(1, 4)))]
        flavour = FLAVOURS[int(rng.integers(0, len(FLAVOURS)))]
        tensor = None
        if F.tensor_allowed(flavour) and rng.random() < 0.5:
            tensor = (DTYPES[int(rng.integers(0, len(DTYPES)))], sorted(SPECS)[int(rng.integers(0, len(SPECS)))])
        n = int(rng.integers(1, MAX_BOXES + 1))
        items, sizes = [], []
        for _ in range(n):
            f = int(rng.integers(0, len(frames)))
            fr = frames[f]
            items.append((f,) + F._box(rng, fr, F._even(rng, 2, fr["w"]), F._even(rng, 2, fr["h"])))
            sizes.append(F._size(rng, 160, 100))
        placement = ("aligned", "unaligned", "mixed")[int(rng.integers(0, 3))]
        aligned = [placement == "aligned" or (placement == "mixed" and rng.random() < 0.5) for _ in range(n)]
        calls.append({"seed": seed, "index": index, "frames": frames, "flavour": flavour, "tensor": tensor, "rt": (NEAREST, BILINEAR, BICUBIC)[int(rng.integers(0, 3))],
                      "items": items, "sizes": sizes, "placement": placement, "aligned": aligned})
    return calls


def cases(chunk):
    return generate(chunk)


def element_bytes(call):
    if call["tensor"] is not None:
        return ESIZE[call["tensor"][0]]
    return 4 if call["flavour"][2] else 1
