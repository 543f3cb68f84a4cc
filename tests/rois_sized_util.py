"""Shared by the tests of tsvpp_convert_rois_sized (include/tsvpp.h): requests, the expected bits and the poisoned output buffer.  No product code.

The contract under test: output i is, bit for bit, what tsvpp_convert_rois returns for box i alone at box i's size -- which is oracle.convert on the box's sliced
planes with dst = that size (tests/test_gpu_rois.py: expect)."""
import ctypes

import numpy as np

OK, UNSUPPORTED, ERROR = 0, -2, -3
NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24, NV12, UYVY, YUV444, HSV = range(7)
PLANAR, MERGED = 0, 1
LIMIT = 48   # TSVPP_MAX_ROIS_SIZED
TILE = 32    # ROI_TILE_W = ROI_TILE_H
GUARD = 64   # bytes kept free before and after every output slot (tests/tile_fuzz.py)
POISON = 0xA5

FLAVOURS = [(fcc, planes, norm) for fcc in (RGB24, BGR24) for planes in (PLANAR, MERGED) for norm in (False, True)] + [(Y800, MERGED, False), (Y800, MERGED, True)]

# ---- the fixed request of tests/test_gpu_rois_sized.py and test_gpu_rois_sized_tensor.py -----------------------------------------------------------------------------
FRAMES = [(320, 180, 328), (192, 108, 200)]  # (width, height, pitch of both planes)
# the sizes of ONE launch, in this order: 2 x 2; a narrow tail; exactly a tile; 4 k + 2 above a tile (shifted last column); 4 k; tiles on both axes and a tail on
# each; multiples of the tile; wide strips; one row pair / one column pair of many tiles
SIZES = [(2, 2), (30, 2), (32, 32), (34, 34), (36, 30), (62, 66), (64, 64), (66, 34), (100, 38), (160, 100), (34, 2), (2, 66)]
BOXES = [
    (1, 190, 106, 192, 108),  # 2 x 2 in the corner of the second frame: exactly its output size
    (0, 101, 40, 201, 90),    # odd left (U and V swap), down-scale
    (0, 0, 0, 320, 180),      # the whole frame
    (1, 10, 11, 26, 27),      # odd top, up-scale
    (0, 100, 50, 136, 80),    # exactly its output size: a plain colour conversion
    (0, 7, 9, 207, 149),      # both odd, down-scale
    (1, 0, 0, 64, 64),        # touches the left and the top edge, exactly its output size
    (0, 254, 100, 320, 180),  # the right and the bottom edge; x as is, y down
    (0, 33, 20, 83, 160),     # up on x, down on y
    (1, 0, 0, 192, 108),      # the whole second frame
    (0, 200, 0, 320, 4),      # the top edge, a strip
    (1, 101, 3, 111, 103),    # odd left, a column pair
]
assert len(SIZES) == len(BOXES) == 12


def tiles(w, h):
    return ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)


def narrow_tail(w):
    """an output 4 k + 2 columns wide and narrower than a tile: no vector stores (narrow_tail, csrc/tsvpp_tiles.h)"""
    return w % 4 != 0 and w < TILE


def channels(fcc):
    return 1 if fcc == Y800 else 3


# ---- C ABI, no GPU ---------------------------------------------------------------------------------------------------------------------------------------------------

def params(native, rt=BILINEAR, fcc=RGB24, planes=MERGED, norm=0, dst=(0, 0), crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, int(norm))


def nv12_records(native, frames):
    """frames (w, h[, pitch_y[, pitch_uv]]) as tsvpp_nv12 records without planes"""
    return (native.NV12 * max(len(frames), 1))(*[native.NV12(None, None, f[2] if len(f) > 2 else 0, f[3] if len(f) > 3 else (f[2] if len(f) > 2 else 0), f[0], f[1])
                                                 for f in frames])


def roi_records(native, rois):
    """rois: (frame, left, top, right, bottom, dst_w, dst_h)"""
    return (native.RoiSized * max(len(rois), 1))(*[native.RoiSized(*r) for r in rois])


def statuses(native, p, frames, rois, spec=None, tensor=False, n_frames=None, n_rois=None, null=(), aligned=1):
    """the status of the describe call and of the convert call with a NULL context for the same request -- (describe, convert, text); `tensor`: the tensor forms"""
    L = native.lib()
    fr, bx = nv12_records(native, frames), roi_records(native, rois)
    outs = (ctypes.c_void_p * max(len(rois), 1))()
    buf = ctypes.create_string_buffer(512)
    nf = len(frames) if n_frames is None else n_frames
    nr = len(rois) if n_rois is None else n_rois
    pp = None if "p" in null else ctypes.byref(p)
    a_fr = None if "frames" in null else fr
    a_bx = None if "rois" in null else bx
    if tensor:
        ps = None if spec is None else ctypes.byref(spec)
        d = L.tsvpp_describe_rois_sized_tensor(pp, ps, nf, a_fr, nr, a_bx, aligned, buf, len(buf))
        c = L.tsvpp_convert_rois_sized_tensor(None, nf, a_fr, nr, a_bx, pp, ps, outs, None)
    else:
        d = L.tsvpp_describe_rois_sized(pp, nf, a_fr, nr, a_bx, aligned, buf, len(buf))
        c = L.tsvpp_convert_rois_sized(None, nf, a_fr, nr, a_bx, pp, outs, None)
    return d, c, buf.value.decode()


def describe(native, p, frames, rois, aligned=1):
    d, _, text = statuses(native, p, frames, rois, aligned=aligned)
    assert d == OK, (d, text)
    out = {}
    for item in text.split(" "):
        k, _, v = item.partition("=")
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


def seeded_request(seed, n=None, max_side=200, frames=((320, 180, 328), (192, 108, 200))):
    """(frames, rois): 1 .. 48 boxes (or n) anywhere in the frames, even output sides 2 .. max_side; one output side in four is at most 34 (narrow tails occur)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, LIMIT + 1)) if n is None else n
    rois = []
    for _ in range(n):
        f = int(rng.integers(0, len(frames)))
        fw, fh = frames[f][0], frames[f][1]
        bw, bh = 2 * int(rng.integers(1, fw // 2 + 1)), 2 * int(rng.integers(1, fh // 2 + 1))
        l, t = int(rng.integers(0, fw - bw + 1)), int(rng.integers(0, fh - bh + 1))
        side = [2 * int(rng.integers(1, (34 if rng.random() < 0.25 else max_side) // 2 + 1)) for _ in range(2)]
        rois.append((f, l, t, l + bw, t + bh, side[0], side[1]))
    return list(frames), rois


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------------

def host_frames(frames=FRAMES, seed=4100):
    """[(y, uv)] of full-range noise, rows x pitch"""
    out = []
    for k, (w, h, pitch) in enumerate(frames):
        rng = np.random.default_rng(seed + k)
        out.append((rng.integers(0, 256, (h, pitch), dtype=np.uint8), rng.integers(0, 256, (h // 2, pitch), dtype=np.uint8)))
    return out


def device_frames(host):
    import torch
    return [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]


_expected = {}


def expect(oracle, host, box, size, rt, fcc, planes, norm, key=None):
    """oracle.convert on the box's sliced planes at the box's own size, as raw bytes; computed once per (key, request) where a key names the frames"""
    k = None if key is None else (key, tuple(box), tuple(size), rt, fcc, planes, bool(norm))
    if k is not None and k in _expected:
        return _expected[k]
    f, l, t, r, b = box
    y, uv = host[f]
    ys, uvs = y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r]  # byte columns: an odd `left` swaps U and V, as the crop stage does
    ref = oracle.convert(ys, uvs, dst=tuple(size), resize_type=rt, fourcc=fcc, planes=planes, normalization=norm)[0]
    ref = np.ascontiguousarray(ref).view(np.uint8).ravel()
    if k is not None:
        _expected[k] = ref
    return ref


_TILE_PATTERN = ((np.arange(4096, dtype=np.int64) * 131 + 17) % 251).astype(np.uint8)  # the guard pattern of tests/test_gpu_tile_fuzz.py


def slot_starts(nbytes, aligned, esz):
    """(starts, total): the byte offset of every output in one buffer that begins on a 16-byte boundary, GUARD free bytes before and after every output; output i
    starts on a 16-byte boundary if aligned[i], else one element (`esz` bytes) past one"""
    starts, pos = [], 0
    for nb, al in zip(nbytes, aligned):
        start = (pos + GUARD + 15) // 16 * 16 + (0 if al else esz)
        starts.append(start)
        pos = start + nb
    return starts, pos + GUARD


def run(v, dev, boxes, sizes, fp, fcc, esz, aligned=True, frames=FRAMES, dtype=None, what="", **kw):
    """one convert_rois_sized into the slots of a poisoned buffer -> the bytes of every output; every byte outside the slots must be unchanged.  aligned: a bool for
    all outputs or one per output; esz: bytes of an element; dtype: the torch element of the slots (default by esz)"""
    import torch
    n = len(boxes)
    aligned = [aligned] * n if isinstance(aligned, bool) else list(aligned)
    nbytes = [channels(fcc) * w * h * esz for w, h in sizes]
    starts, total = slot_starts(nbytes, aligned, esz)
    pat = np.tile(_TILE_PATTERN, (total + 4095) // 4096)[:total]
    host = pat.copy()
    for s, nb in zip(starts, nbytes):
        host[s:s + nb] = POISON
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    if dtype is not None:  # the tensor form: the call is told the element, and the slots were sized for it
        assert torch.empty((), dtype=dtype).element_size() == esz
        kw["dtype"] = dtype
    else:
        assert "mean" not in kw and "std" not in kw
        dtype = {1: torch.uint8, 4: torch.float32}[esz]
    out = [buf[s:s + nb].view(dtype) for s, nb in zip(starts, nbytes)]
    ret = v.convert_rois_sized([d[0] for d in dev], [d[1] for d in dev], boxes, fp, sizes, out=out, width=[f[0] for f in frames], height=[f[1] for f in frames], **kw)
    assert ret is out
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    outs = [got[s:s + nb].copy() for s, nb in zip(starts, nbytes)]
    for s, nb in zip(starts, nbytes):
        got[s:s + nb] = pat[s:s + nb]
    bad = np.flatnonzero(got != pat)
    if bad.size:
        k = max(int(np.searchsorted(np.array(starts), bad[0], side="right")) - 1, 0)
        raise AssertionError(f"{what}: {bad.size} guard bytes damaged, the first at {int(bad[0]) - starts[k]} relative to output {k} ({sizes[k]}, {nbytes[k]} bytes)")
    return outs


def compare(outs, refs, boxes, sizes, what=""):
    for i, (g, ref) in enumerate(zip(outs, refs)):
        assert g.size == ref.size, f"{what}: output {i} has {g.size} bytes, expected {ref.size}"
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what}: output {i} (box {boxes[i]} -> {sizes[i]}): {bad.size} of {g.size} bytes differ, first at {bad[:4]}"


def frame_parameters(ts, rt, fcc, planes, norm, dst=(0, 0)):
    return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
