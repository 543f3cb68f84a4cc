"""No GPU: the host side of tsvpp_convert_letterbox_area / tsvpp_describe_letterbox_area / tsvpp_letterbox_area_rows (include/tsvpp.h).

The jump start: tsvpp_letterbox_area_rows -- the generator begun at the last multiple of the pattern's period in front of `first` -- returns, bit for bit, the
rows tsvpp_roi_area_rows returns from index 0, and reports the start the restatement below derives.  The restatement is numpy float32 arithmetic written here:
the closing test of build_area_rows, `(float)k * scale` has no fraction above FLT_EPSILON, evaluated for k = 1 .. first independently.
Then: every validation status in its stated order (the letterbox call's cases, reused from tests/test_letterbox_cpu.py; then the AREA limits; then the spec's),
describe and convert agreeing; the describe line's keys, chain= against the restatement; the existing letterbox entry points still refusing AREA."""
import ctypes
import random

import numpy as np
import pytest

from letterbox_util import default_rect
from test_letterbox_cpu import ERROR_CASES, UNSUPPORTED_CASES

OK, UNSUPPORTED, ERROR = 0, -2, -3
NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24 = 0, 1, 2
F1080 = (1920, 1080, 2048)
TILE = 32
EPS = np.float32(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------------
def scale_of(src, dst):
    return np.float32(src) / np.float32(dst)


def period(scale, limit):
    """the first k in 1 .. limit whose product with the scale, in float32, has no fraction above FLT_EPSILON; 0: none"""
    if limit < 1:
        return 0
    k = np.arange(1, limit + 1, dtype=np.int64)
    pos = k.astype(np.float32) * np.float32(scale)
    assert pos.dtype == np.float32
    frac = pos - np.trunc(pos)
    hit = np.flatnonzero(~(frac > EPS))
    return int(k[hit[0]]) if hit.size else 0


def start_of(scale, first):
    p = period(scale, first)
    return (first // p) * p if p else 0


def rows(native, fn, scale, first, n):
    t, s = ctypes.c_int(-1), ctypes.c_int(-1)
    out = np.full(n * 40, np.nan, np.float32)
    extra = (ctypes.byref(s),) if fn == "tsvpp_letterbox_area_rows" else ()
    got = getattr(native.lib(), fn)(ctypes.c_float(scale), first, n, out.ctypes.data, out.size, ctypes.byref(t), *extra)
    assert got == n, (fn, scale, first, n, got)
    return out[:n * t.value].view(np.uint32).copy(), t.value, s.value


NAMED = [(1920, 640, 1), (240, 100, 5), (200, 76, 19), (1920, 608, 57), (1366, 640, 320), (214, 70, 105), (186, 46, None)]


def firsts(p, dst):
    base = [0, 1, 31, 32, 33, dst - 1]
    if p:
        base += [p - 1, p, p + 1, 2 * p + 3]
    return sorted({f for f in base if 0 <= f < dst})


def check_rows(native, src, dst):
    scale = scale_of(src, dst)
    for first in firsts(period(scale, dst), dst):
        n = min(TILE, dst - first)
        a, ta, start = rows(native, "tsvpp_letterbox_area_rows", scale, first, n)
        b, tb, _ = rows(native, "tsvpp_roi_area_rows", scale, first, n)
        assert ta == tb == int(np.ceil(scale)) and np.array_equal(a, b), (src, dst, first)
        assert start == start_of(scale, first), (src, dst, first, start)


@pytest.mark.parametrize("src,dst,p", NAMED)
def test_rows_from_the_jump_start_are_the_generators_rows(native, src, dst, p):
    scale = scale_of(src, dst)
    if p is None:  # nothing closes within 184
        assert period(scale, 184) == 0
        for first in (1, 33, dst - 1):
            assert rows(native, "tsvpp_letterbox_area_rows", scale, first, 1)[2] == 0
    else:
        assert period(scale, 4096) == p
        if p >= dst:  # no close inside the output: every chain starts at 0
            assert rows(native, "tsvpp_letterbox_area_rows", scale, dst - 1, 1)[2] == 0
    check_rows(native, src, dst)


def test_rows_of_seeded_pairs(native):
    r = random.Random(20261021)
    seen = set()
    for _ in range(200):
        dst = 2 * r.randrange(1, 321)
        src = 2 * r.randrange(dst // 2 + 1, min(2048, 20 * dst) + 1)  # even, ratio in (1, 40]
        check_rows(native, src, dst)
        seen.add(period(scale_of(src, dst), dst) > 1)
    assert seen == {False, True}


def test_rows_argument_checks(native):
    L = native.lib()
    out = np.zeros(64, np.float32)
    t, s = ctypes.c_int(), ctypes.c_int()
    call = lambda scale, first, n, buf=out.ctypes.data, cap=64: L.tsvpp_letterbox_area_rows(ctypes.c_float(scale), first, n, buf, cap, ctypes.byref(t), ctypes.byref(s))
    assert call(3.0, 0, 4, buf=None) == ERROR and call(3.0, -1, 4) == ERROR and call(3.0, 0, 0) == ERROR and call(3.0, 0, 22) == ERROR
    assert call(1.0, 0, 4) == UNSUPPORTED and call(40.5, 0, 1) == UNSUPPORTED and call(3.0, 65536, 1) == UNSUPPORTED
    assert L.tsvpp_letterbox_area_rows(ctypes.c_float(3.0), 7, 2, out.ctypes.data, 64, None, None) == 2  # taps / start are optional


# ---- statuses -------------------------------------------------------------------------------------------------------------------------------------------------
def P(native, dst=(640, 640), rt=AREA, fcc=RGB24, planes=1, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def both(native, p, frames, rects=None, pad=(114, 128, 128), n=None, null=(), spec=None):
    """the status of tsvpp_describe_letterbox_area and of tsvpp_convert_letterbox_area with a NULL context for the same request: (describe, convert, text)"""
    L = native.lib()
    fr = (native.NV12 * max(len(frames), 1))(*[native.NV12(None, None, f[2] if len(f) > 2 else 0, f[2] if len(f) > 2 else 0, f[0], f[1]) for f in frames])
    rc = None if rects is None else (native.Rect * max(len(rects), 1))(*[native.Rect(*r) for r in rects])
    outs = (ctypes.c_void_p * max(len(frames), 1))()
    buf = ctypes.create_string_buffer(512)
    cnt = len(frames) if n is None else n
    pp = None if "p" in null else ctypes.byref(p)
    a_fr = None if "frames" in null else fr
    sp = None if spec is None else ctypes.byref(spec)
    d = L.tsvpp_describe_letterbox_area(pp, sp, cnt, a_fr, rc, 1, buf, len(buf))
    c = L.tsvpp_convert_letterbox_area(None, cnt, a_fr, pp, sp, rc, pad[0], pad[1], pad[2], outs, None)
    return d, c, buf.value.decode()


def _status(native, case, **more):
    case = dict(case)
    frames = case.pop("frames", [F1080])
    kw = {k: case.pop(k) for k in ("rects", "pad", "n", "null") if k in case}
    case.setdefault("rt", AREA)
    return both(native, P(native, **case), frames, **kw, **more)


def test_symbols_and_facades(native):
    L = native.lib()
    for sym in ("tsvpp_convert_letterbox_area", "tsvpp_describe_letterbox_area", "tsvpp_letterbox_area_rows"):
        assert sym in native.SYMBOLS and hasattr(L, sym)
    assert len(L.tsvpp_convert_letterbox_area.argtypes) == 11 and len(L.tsvpp_describe_letterbox_area.argtypes) == 8 and len(L.tsvpp_letterbox_area_rows.argtypes) == 7
    import tensor_stream as ts
    from tensor_stream import vpp
    assert ts.describe_letterbox_area is vpp.describe_letterbox_area and hasattr(ts.VideoProcessor, "convert_letterbox_area")


@pytest.mark.parametrize("case", ERROR_CASES, ids=[c[0] for c in ERROR_CASES])
def test_the_letterbox_calls_errors(native, case):
    d, c, text = _status(native, case[1])
    assert (d, c, text[:5]) == ((OK, ERROR, "mode=") if len(case) > 2 else (ERROR, ERROR, ""))  # (the describe call takes no pad)


@pytest.mark.parametrize("case", [c for c in UNSUPPORTED_CASES if c[0] != "AREA"], ids=[c[0] for c in UNSUPPORTED_CASES if c[0] != "AREA"])
def test_the_letterbox_calls_refusals(native, case):
    assert _status(native, case[1])[:2] == (UNSUPPORTED, UNSUPPORTED)


def make_spec(native, dtype=1, mean=(0.5, 0.5, 0.5), scale=(2.0, 2.0, 2.0)):
    return native.TensorSpec(dtype, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*scale))


def test_the_calls_own_refusals_in_order(native):
    for rt in (NEAREST, BILINEAR, BICUBIC, 7):
        assert _status(native, dict(rt=rt))[:2] == (UNSUPPORTED, UNSUPPORTED)
    # the limits: 40 taps pass, 41 do not (1920 -> 48 columns is ratio 40, -> 46 is 41.7; 1080 -> 26 rows is 41.5); on either axis; only where the frame is down-scaled
    assert _status(native, dict(rects=[(0, 0, 48, 360)]))[:2] == (OK, ERROR)  # (convert: the request is fine, the context is null)
    assert _status(native, dict(rects=[(0, 0, 46, 360)]))[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert _status(native, dict(rects=[(0, 0, 640, 26)]))[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert _status(native, dict(frames=[F1080, F1080], rects=[(0, 0, 640, 360), (0, 0, 46, 360)]))[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert _status(native, dict(frames=[(4096, 16, 4096)], dst=(64, 64), rects=[(0, 0, 64, 64)]))[:2] == (OK, ERROR)  # 64 x on x, up-scaled on y: the 2 x 2 rule
    # a rectangle side above 65536 (Y800 uint8 so that the canvas stays below 4 GiB)
    assert _status(native, dict(frames=[(64, 64, 64)], dst=(65540, 2), fcc=Y800, rects=[(0, 0, 65538, 2)]))[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert _status(native, dict(frames=[(64, 64, 64)], dst=(65540, 2), fcc=Y800, rects=[(0, 0, 65536, 2)]))[:2] == (OK, ERROR)
    # the letterbox call's rules come first, the limits second, the spec's last
    assert _status(native, dict(rects=[(0, 0, 46, 0)]))[:2] == (ERROR, ERROR)
    assert _status(native, dict(rects=[(0, 0, 46, 361)]))[:2] == (UNSUPPORTED, UNSUPPORTED)
    bad_spec = make_spec(native, scale=(0.0, 2.0, 2.0))
    assert _status(native, dict(rects=[(0, 0, 46, 360)], norm=1, planes=0), spec=bad_spec)[:2] == (UNSUPPORTED, UNSUPPORTED)  # limit before rule 2
    assert _status(native, dict(norm=1, planes=0), spec=bad_spec)[:2] == (ERROR, ERROR)                                          # rule 2
    assert _status(native, dict(norm=1, planes=0), spec=make_spec(native, mean=(float("nan"), 0, 0)))[:2] == (ERROR, ERROR)
    good = make_spec(native)
    assert _status(native, dict(norm=1, planes=0), spec=good)[:2] == (OK, ERROR)
    assert _status(native, dict(norm=1, planes=0, fcc=Y800), spec=good)[:2] == (OK, ERROR)
    assert _status(native, dict(norm=1, planes=0), spec=make_spec(native, dtype=5))[:2] == (UNSUPPORTED, UNSUPPORTED)             # rule 3
    assert _status(native, dict(norm=0, planes=0), spec=good)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert _status(native, dict(norm=1, planes=1), spec=good)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert _status(native, dict(rt=BILINEAR, norm=1, planes=0), spec=good)[:2] == (UNSUPPORTED, UNSUPPORTED)


def test_the_existing_entry_points_still_refuse_area(native):
    L = native.lib()
    fr = (native.NV12 * 1)(native.NV12(None, None, 2048, 2048, 1920, 1080))
    buf = ctypes.create_string_buffer(512)
    outs = (ctypes.c_void_p * 1)()
    p = P(native, rt=AREA, norm=1, planes=0)
    sp = make_spec(native)
    assert L.tsvpp_describe_letterbox(ctypes.byref(p), 1, fr, None, 1, buf, len(buf)) == UNSUPPORTED
    assert L.tsvpp_convert_letterbox(None, 1, fr, ctypes.byref(p), None, 114, 128, 128, outs, None) == UNSUPPORTED
    assert L.tsvpp_describe_letterbox_tensor(ctypes.byref(p), ctypes.byref(sp), 1, fr, None, 1, buf, len(buf)) == UNSUPPORTED
    assert L.tsvpp_convert_letterbox_tensor(None, 1, fr, ctypes.byref(p), ctypes.byref(sp), None, 114, 128, 128, outs, None) == UNSUPPORTED
    import tensor_stream as ts
    with pytest.raises(RuntimeError, match="-2"):
        ts.describe_letterbox(ts.FrameParameters(width=640, height=640, resize_type=AREA, pixel_format=RGB24, planes_pos=1, normalization=False), [F1080])


# ---- the describe line ----------------------------------------------------------------------------------------------------------------------------------------
def chain_of(frames, canvas, rects=None, vec=True):
    """the most steps a chain of any tile runs in front of its first row: per down-scale frame, per tile column and row that touches the rectangle, the luma chain
    (first - start) and the chroma chain of [first >> 1, ..]; tile columns as the kernel lays them out (the shifted last column of 4 k + 2 wide canvases)"""
    cw, ch = canvas
    longest = 0
    for k, (w, h, *_) in enumerate(frames):
        left, top, rw, rh = rects[k] if rects else default_rect(w, h, cw, ch)
        sx, sy = scale_of(w, rw), scale_of(h, rh)
        if not (sx > 1 and sy > 1):
            continue
        cols = list(range(0, cw, TILE))
        if vec and cw % 4 and cw >= TILE:
            cols[-1] = cw - TILE
        for scale, firsts_, origin, size, extent in ((sx, cols, left, rw, cw), (sy, list(range(0, ch, TILE)), top, rh, ch)):
            for f in firsts_:
                lo, hi = max(f, origin) - origin, min(min(f + TILE, extent) - 1, origin + size - 1) - origin
                if lo > hi:
                    continue
                p = period(scale, lo)
                for first in (lo, lo >> 1):
                    longest = max(longest, first - ((first // p) * p if p else 0))
    return longest


def describe(frames, canvas, rects=None, **kw):
    import tensor_stream as ts
    fp = ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=AREA, pixel_format=kw.pop("fcc", BGR24), planes_pos=kw.pop("planes", 0),
                            normalization=kw.pop("norm", True))
    return ts.describe_letterbox_area(fp, frames, rects=rects, **kw)


def test_describe_keys_and_chain():
    d = describe([F1080], (640, 640))
    assert d["mode"] == "area" and d["out"] == "f32_planar" and d["dst"] == "640x640" and d["frames"] == 1 and d["launches"] == 1 and d["limit"] == 32
    assert d["kernel"] == "vpp_letterbox_area<O_F32_PLANAR,vec,staged>" and d["shape"] == "8x16" and d["grid"] == 400 and d["tiles"] == "20x20"
    assert d["inner"] == "640x360+0+140" and d["down"] == 1 and d["taps"] == "3x3" and d["chain"] == 0
    # lds= includes the weight rows: 49 rows per axis at a stride of 3 floats, 2 x 50 records of 12 bytes, rounded to 16 -- and the staged footprint behind them
    rows_bytes = (4 * (49 * (3 + 3) + 2 * 3 * 50) + 15) & ~15
    assert d["lds"] > rows_bytes and d["staged"] == 1
    # 608 x 608 (P = 57) and 1366 x 768 into 640 x 640 (P = 320 on x): the value the restatement derives
    for frames, canvas in (([F1080], (608, 608)), ([(1366, 768, 1408)], (640, 640)), ([F1080, (1366, 768, 1408), (3840, 2160, 3840)], (640, 640))):
        got = describe(frames, canvas)["chain"]
        assert got == chain_of(frames, canvas) and (got > 0), (frames, canvas, got)
    assert describe([F1080], (608, 608))["chain"] == 56 and period(scale_of(1920, 608), 608) == 57
    assert describe([(3840, 2160, 3840)], (640, 640))["chain"] == 0 and describe([(1280, 720, 1280)], (640, 360))["chain"] == 0
    # an up-scaled frame alone: no rows, no chain
    u = describe([(320, 180, 320)], (640, 640))
    assert u["down"] == 0 and u["taps"] == "0x0" and u["chain"] == 0
    # chain= is of the FIRST launch: 33 frames, the long chain in the last
    many = describe([F1080] * 32 + [(1366, 768, 1408)], (640, 640))
    assert many["launches"] == 2 and many["chain"] == 0 and many["down"] == 33
    # caller's rectangles and the shifted tile column
    r = [(0, 12, 100, 76)]
    assert describe([(240, 180, 256)], (100, 100), rects=r)["chain"] == chain_of([(240, 180)], (100, 100), rects=r)
    assert describe([(214, 182, 224)], (70, 66))["tail"] == 2
    assert describe([(214, 182, 224)], (70, 66), rects=[(0, 0, 70, 66)])["chain"] == chain_of([(214, 182)], (70, 66), rects=[(0, 0, 70, 66)])
    assert describe([(214, 182, 224)], (70, 66), rects=[(0, 0, 70, 66)], aligned_outputs=False)["chain"] == chain_of([(214, 182)], (70, 66), rects=[(0, 0, 70, 66)], vec=False)


def test_describe_with_a_spec_names_the_tensor_kernel():
    torch = pytest.importorskip("torch")
    d = describe([F1080], (640, 640), dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    assert d["out"] == "f16_planar" and d["kernel"] == "vpp_letterbox_area_tensor<PLANAR,EL_HALF,vec,staged>" and d["mode"] == "area" and d["chain"] == 0
    y = describe([F1080], (640, 640), fcc=Y800, planes=1, dtype=torch.float32)
    assert y["out"] == "f32n_y800" and y["kernel"] == "vpp_letterbox_area_tensor<Y800,EL_F32,vec,staged>"
