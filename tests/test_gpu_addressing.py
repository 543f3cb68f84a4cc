"""GPU: the 32-bit addressing of the kernels at its limits (profiles/addressing_limits.txt is the audit this file tests).

Inside one plane and inside one output the kernels address with unsigned 32-bit byte offsets.  Everything else in the suite stays below 2^27 bytes: here the
offsets cross the sign bit and come within a row of what the host accepts.

  sources   planes whose span, as seen from the address the kernel is handed, lies just past 2^31 (class A) and within one row under TSVPP_SOURCE_SPAN_LIMIT
            (class B), luma and chroma each with a pitch of its own, at pitches that are multiples of 16 (the LDS-DMA staging) and 6 mod 16: the cheapest request
            of tests/dispatch_grid.py per kernel name through tsvpp_convert (one frame, and a batch of 3 whose frames interleave in memory), and the tile calls
            (ROI, AREA-ROI, letterbox, warp, perspective, remap, mesh; replicate and constant border; staged and gathering contexts; one tensor form);
  outputs   of more than 2^31 bytes and of just under 2^32: one per store routine of the audit (S1 .. S9 and S11; each case asserts the kernel it launched), in the
            flavours the suite's time allows.  Section 5 of the audit names the routine (S10) and the flavours that are left out, with the oracle's measured time.

All of it lives in ONE device allocation (tests/arena_util.py) in which every address within 2^32 bytes of a kernel's base is owned by the test and holds a fill
byte: a sign-extended, truncated or late-scaled offset reads or writes the fill and fails a comparison -- it cannot fault.  Expected bits are the oracle's on the
tight frame (the result does not depend on the pitch); raw bits, every element, no tolerance.  Nothing at or above the limit is launched: that is
tests/test_plan_cpu.py's side."""
import ctypes
import time
import zlib

import numpy as np
import pytest
import torch

import arena_util as AU
import dispatch_grid as G
import letterbox_util as L
import mesh_util as M
import persp_util as P
import remap_util as R
import tensor_util as T
import warp_util as W
from util import knob_run, synth_nv12

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24, NV12, UYVY, YUV444, HSV = range(7)
PLANAR, MERGED = 0, 1
N_BATCH = 3
CHUNKS = 4
BORDER = (3, 250, 7)
# kernels the selection names only for launches of 32 frames and more (the 32-row tile of the AREA column kernel; its 8-row instance runs here): the batches of
# this file are 1 and 3 frames whose planes interleave inside one pitch
MANY_FRAMES_ONLY = {"vpp_area_cols_kernel<2,32,OUT>"}


@pytest.fixture(scope="module")
def arena():
    a = AU.Arena(torch.device("cuda", 0))
    yield a
    del a
    torch.cuda.empty_cache()


def _params(dst, rt, fcc, planes, norm, crop=(0, 0, 0, 0)):
    import tensor_stream as ts
    return ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


def _first_diff(got, want):
    """(first differing byte, number of differing bytes) of two device byte tensors, in pieces of 256 MiB"""
    first, count = None, 0
    for lo in range(0, got.numel(), 1 << 28):
        bad = got[lo: lo + (1 << 28)] != want[lo: lo + (1 << 28)]
        c = int(bad.sum())
        if c and first is None:
            first = lo + int(torch.nonzero(bad)[0])
        count += c
    return first, count


def _same_bits(got, want, what):
    if not torch.equal(got, want):
        first, count = _first_diff(got, want)
        fill = int((got == AU.FILL).sum())
        raise AssertionError(f"{what}: {count} of {got.numel()} bytes differ from the expected bits, the first at byte {first} (got {int(got[first])}, expected "
                             f"{int(want[first])}; {fill} bytes of the output equal the arena's fill byte)")


# ---- sources: tsvpp_convert, one request per kernel name ------------------------------------------------------------------------------------------------------------

def _seen(req):
    """(left, top, width, height) of the region Convert's kernels see: the crop box where the crop stage applies (tsvpp_plan.cpp: make_plan), else the frame"""
    (w, h, _, _), crop = req[0], req[1]
    cw, ch = crop[2] - crop[0], crop[3] - crop[1]
    return (crop[0], crop[1], cw, ch) if (0 < cw < w and 0 < ch < h) else (0, 0, w, h)


def _describe_kernel(req, py, puv, n):
    import tensor_stream as ts
    (w, h, _, _), crop, dst, rt, fcc, planes, norm, _, aligned = req
    return ts.describe(_params(dst, rt, fcc, planes, norm, crop), w, h, pitch=py, pitch_uv=puv, n_frames=n, aligned_outputs=bool(aligned))["kernel"]


_cases = {}


def convert_cases():
    """[(kernel name, request, [(residue_y, residue_uv)])]: per kernel name describe knows on the grid, the cheapest request (fewest oracle bytes) with a source of
    at least 16 rows that still selects the kernel as one frame and as a batch of 3 at an everyday pitch of some residue mod 16 -- a multiple of 16, 6 mod 16,
    the request's own: the residues "the signature allows".  Host logic, deterministic; under A/B knobs the grid and the names are the knobs'."""
    if "convert" in _cases:
        return _cases["convert"]
    by_kernel = {}
    for sig in sorted(G.signatures()):
        req = G.representative(sig)
        if _seen(req)[3] >= 16:
            by_kernel.setdefault(G.kernel_name(sig), []).append((G.oracle_bytes(req), req[7], repr(req), req))
    out, lost = [], []
    for kernel in sorted(by_kernel):
        for _, _, _, req in sorted(by_kernel[kernel]):
            w, py0, puv0 = req[0][0], req[0][2], req[0][3]
            residues = []
            for ry, ruv in dict.fromkeys(((0, 0), (6, 6), (py0 % 16, puv0 % 16))):
                py, puv = (w + 15) // 16 * 16 + ry, (w + 15) // 16 * 16 + ruv
                if all(_describe_kernel(req, py, puv, n) == kernel for n in (1, N_BATCH)):
                    residues.append((ry, ruv))
            if residues:
                out.append((kernel, req, residues))
                break
        else:
            lost.append(kernel)
    _cases["convert"], _cases["lost"] = out, lost
    return out


def _place_frames(arena, host, region, pitches):
    """the rows of `region` = (left, top, width, height) of every frame of `host` [(y, uv) tight device planes] written into the arena at `pitches` (luma, chroma),
    the frames interleaved; returns the planes [(luma, chroma)] -- to be erased by the caller"""
    left, top, rw, rh = region
    w = host[0][0].shape[1]
    placed = _planes(len(host), w, region, pitches)
    for (yp, uvp), (y, uv) in zip(placed, host):
        arena.write(yp, y[top: top + rh])
        arena.write(uvp, uv[top // 2: top // 2 + rh // 2])
    return placed


def _planes(n, w, region, pitches):
    """n frames' planes, placed (host logic).  Every luma plane comes before every chroma plane: the chroma pitch is a little more than twice the luma pitch,
    so chroma row s drifts to the right of luma row 2 s as s grows -- from a column of its own further right it never meets it."""
    left, top, rw, rh = region
    py, puv = pitches
    lumas = [AU.Plane(rh, rw, py, lead=top * py + left, first=top, total_bytes=w) for _ in range(n)]
    chromas = [AU.Plane(rh // 2, rw, puv, lead=(top // 2) * puv + left, first=top // 2, total_bytes=w) for _ in range(n)]
    AU.place(lumas + chromas)
    return list(zip(lumas, chromas))


def _class_pitches(region, residues, cls):
    return AU.pitch_pair(region[3], region[2], residues, cls)


def _run_convert(vpp, oracle, arena, kernel, req, residues):
    import tensor_stream as ts
    dev = arena.buf.device
    (w, h, _, _), crop, dst, rt, fcc, planes, norm, _, aligned = req
    region = _seen(req)
    fp = _params(dst, rt, fcc, planes, norm, crop)
    f32 = bool(norm) or fcc == HSV
    nbytes = G.out_bytes(req)
    seed = zlib.crc32(kernel.encode())
    host = [synth_nv12(w, h, seed=seed + k) for k in range(N_BATCH)]
    want = []
    for y, uv in host:
        ref, _, _ = oracle.convert(y, uv, crop=crop, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=16)
        assert ref.view(np.uint8).size == nbytes
        want.append(torch.from_numpy(ref.view(np.uint8).ravel()).to(dev))
    tight = [(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev)) for y, uv in host]
    off = 0 if aligned else (4 if f32 else 1)
    stride = (nbytes + 15) // 16 * 16 + 16
    raw = torch.empty(N_BATCH * stride + 16, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    slots = [raw[k * stride + off: k * stride + off + nbytes] for k in range(N_BATCH)]
    ran = 0
    for res in residues:
        for cls in "AB":
            py, puv = _class_pitches(region, res, cls)
            what = f"{kernel}, request {req}, class {cls}, pitches {py} / {puv} (residues {res}), spans {AU.span(region[3], region[2], py)} / {AU.span(region[3] // 2, region[2], puv)}"
            for n in (1, N_BATCH):  # the big pitch selects what the everyday pitch of its residue selects: the kernel this request stands for
                named = _describe_kernel(req, py, puv, n)
                assert named == kernel, f"describe names {named} for {n} frame(s): {what}"
            placed = _place_frames(arena, tight, region, (py, puv))
            try:
                raw.fill_(0x5A)
                vpp.Convert(arena.handle(placed[0][0]), arena.handle(placed[0][1]), fp, out=slots[0], width=w, height=h)
                torch.cuda.synchronize()
                assert ts.vpp.debug_last_launch()["kernel"] == kernel, f"launched {ts.vpp.debug_last_launch()['kernel']}: {what}"
                _same_bits(slots[0], want[0], f"one frame: {what}")
                raw.fill_(0x5A)
                vpp.convert_batch([arena.handle(p[0]) for p in placed], [arena.handle(p[1]) for p in placed], fp, out=slots, width=w, height=h)
                torch.cuda.synchronize()
                assert ts.vpp.debug_last_launch()["kernel"] == kernel, f"batch: launched {ts.vpp.debug_last_launch()['kernel']}: {what}"
                for k in range(N_BATCH):
                    _same_bits(slots[k], want[k], f"frame {k} of a batch of {N_BATCH}: {what}")
            finally:
                for p in placed:
                    arena.erase(p[0])
                    arena.erase(p[1])
            ran += 1
    return ran


def test_every_kernel_name_of_the_grid_has_a_request_here():
    cases = convert_cases()
    assert cases
    if knob_run():  # (the grid and its kernel names follow the knobs: TSVPP_FORCE_GATHER=1 leaves two)
        return
    assert set(_cases["lost"]) <= MANY_FRAMES_ONLY, f"no request of the grid selects {_cases['lost']} as one frame and as a batch of {N_BATCH}"
    assert len(cases) >= 20 and len({k.split('<')[0] for k, _, _ in cases}) >= 10, [k for k, _, _ in cases]
    both = sum(1 for _, _, res in cases if (0, 0) in res and (6, 6) in res)
    assert both >= 10, f"only {both} kernels run at both pitch residues"


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_convert_reads_planes_whose_span_crosses_2_31_and_comes_within_a_row_of_the_limit(vpp, oracle, arena, chunk):
    mine = convert_cases()[chunk::CHUNKS]
    if knob_run() and not mine:  # (a knob setting may leave fewer kernel names than chunks; test_every_kernel_name... above fails if it leaves none at all)
        return
    assert mine, "the grid lost its kernel names"
    t0, ran = time.perf_counter(), 0
    for kernel, req, residues in mine:
        ran += _run_convert(vpp, oracle, arena, kernel, req, residues)
    assert arena.untouched(0, AU.MARGIN), "a conversion wrote into the margin in front of its sources"
    print(f"chunk {chunk}: {len(mine)} kernels, {ran} placements (x one frame and a batch of {N_BATCH}) in {time.perf_counter() - t0:.1f} s")


# ---- sources: the tile calls ------------------------------------------------------------------------------------------------------------------------------------------
FLAV = [(BGR24, PLANAR, True), (RGB24, MERGED, False)]
TW, TH = 322, 182          # the frames of the calls that sample the whole frame: no multiple of a tile, 91 chroma rows
RW, RH = 640, 360          # the frames of the ROI calls ...
BOX = (64, 40, 64 + 320, 40 + 200)  # ... and the box of each: its span crosses, the frame's is larger still


@pytest.fixture(scope="module")
def tile_frames():
    dev = torch.device("cuda", 0)
    whole = [synth_nv12(TW, TH, seed=7100 + k) for k in range(N_BATCH)]
    roi = [synth_nv12(RW, RH, seed=7200 + k) for k in range(N_BATCH)]
    up = lambda fr: [(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev)) for y, uv in fr]
    return dict(whole=whole, roi=roi, whole_dev=up(whole), roi_dev=up(roi))


_want = {}


def _cached(key, make):
    if key not in _want:
        _want[key] = make()
    return _want[key]


def _tile_calls(oracle, fr):
    """{name: (frames key, region, call(vpp, ys, uvs, fp, border, size kw) -> outputs, expected(k, flavour, border) -> bytes, dst, resize type, takes a border)}"""
    whole, roi = fr["whole"], fr["roi"]
    dst = (112, 80)
    m_rot = [tuple(_rotated(TW, TH, 20.0 + 25 * k, dst)) for k in range(N_BATCH)]
    quad = [(30.0, 12.0), (TW - 20.0, 25.0), (TW - 40.0, TH - 10.0), (12.0, TH - 30.0)]
    h_quad = P.from_quad(quad, *dst)
    xy = R.barrel(dst[0], dst[1], TW, TH)
    cell = (16, 8)
    mesh = M.barrel(dst[0], dst[1], cell, TW, TH)
    dense = M.expand(mesh, dst[0], dst[1], cell)

    def conv(frames, k, fl, **kw):
        ref, _, _ = oracle.convert(frames[k][0], frames[k][1], fourcc=fl[0], planes=fl[1], normalization=fl[2], nthreads=16, **kw)
        return ref.view(np.uint8).ravel()

    return {
        "rois": ("roi", BOX, lambda v, ys, uvs, fp, b, kw: v.convert_rois(ys, uvs, [(k,) + BOX for k in range(N_BATCH)], fp, **kw),
                 lambda k, fl, b: conv(roi, k, fl, crop=BOX, dst=dst, resize_type=BICUBIC), dst, BICUBIC, False),
        "rois_area": ("roi", BOX, lambda v, ys, uvs, fp, b, kw: v.convert_rois_area(ys, uvs, [(k,) + BOX for k in range(N_BATCH)], fp, **kw),
                      lambda k, fl, b: conv(roi, k, fl, crop=BOX, dst=(64, 48), resize_type=AREA), (64, 48), AREA, False),
        "letterbox": ("whole", None, lambda v, ys, uvs, fp, b, kw: v.convert_letterbox(ys, uvs, fp, pad=(114, 128, 128), **kw)[0],
                      lambda k, fl, b: L.expected_canvas(oracle, whole[k][0], whole[k][1], TW, TH, L.default_rect(TW, TH, 128, 128), (128, 128), BILINEAR, fl[0], fl[1], fl[2],
                                                         (114, 128, 128)), (128, 128), BILINEAR, False),
        "warp": ("whole", None, lambda v, ys, uvs, fp, b, kw: v.convert_warp(ys, uvs, [(k,) + m_rot[k] for k in range(N_BATCH)], fp, border=b, **kw),
                 lambda k, fl, b: W.expected(oracle, whole[k][0], whole[k][1], TW, TH, m_rot[k], dst, fl[0], fl[1], fl[2], b), dst, BILINEAR, True),
        "perspective": ("whole", None, lambda v, ys, uvs, fp, b, kw: v.convert_perspective(ys, uvs, [(k,) + tuple(h_quad) for k in range(N_BATCH)], fp, border=b, **kw),
                        lambda k, fl, b: P.expected(oracle, whole[k][0], whole[k][1], TW, TH, h_quad, dst, fl[0], fl[1], fl[2], b), dst, BILINEAR, True),
        "remap": ("whole", None, lambda v, ys, uvs, fp, b, kw: v.convert_remap(ys, uvs, torch.from_numpy(xy).cuda(), fp, border=b, **kw),
                  lambda k, fl, b: R.expected(oracle, whole[k][0], whole[k][1], TW, TH, xy, fl[0], fl[1], fl[2], b), dst, BILINEAR, True),
        "mesh": ("whole", None, lambda v, ys, uvs, fp, b, kw: v.convert_mesh(ys, uvs, torch.from_numpy(mesh).cuda(), fp, cell=cell, border=b, **kw),
                 lambda k, fl, b: R.expected(oracle, whole[k][0], whole[k][1], TW, TH, dense, fl[0], fl[1], fl[2], b), dst, BILINEAR, True),
    }


def _rotated(w, h, degrees, dst):
    import tensor_stream as ts
    return ts.vpp.warp_rotated_box(w / 2.0 + 3.0, h / 2.0 - 2.0, 0.8 * w, 0.8 * h, np.deg2rad(degrees), dst[0], dst[1])


TILE_CALLS = ("rois", "rois_area", "letterbox", "warp", "perspective", "remap", "mesh")


@pytest.mark.parametrize("name", TILE_CALLS)
def test_tile_calls_read_planes_whose_span_crosses_2_31_and_comes_within_a_row_of_the_limit(oracle, arena, tile_frames, monkeypatch, name):
    """each call on three frames interleaved in the arena, classes A and B, pitches 0 and 6 mod 16, two flavours, replicate and a constant border where the call has
    one, in a context with the default LDS budget (tiles stage their footprint) and in one with TSVPP_LDS_KB=0 (every tile gathers from global memory)"""
    import tensor_stream as ts
    key, box, call, expected, dst, rt, bordered = _tile_calls(oracle, tile_frames)[name]
    host, tight = tile_frames[key], tile_frames[key + "_dev"]
    h, w = host[0][0].shape
    region = (box[0], box[1], box[2] - box[0], box[3] - box[1]) if box else (0, 0, w, h)
    for kb in (None, "0"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            for res in ((0, 0), (6, 6)):
                for cls in "AB":
                    pitches = _class_pitches(region, res, cls)
                    placed = _place_frames(arena, tight, region, pitches)
                    if box:  # the frame's own span is larger still -- beyond the limit in class B, where only a box can be read
                        assert AU.span(h, w, pitches[0]) > AU.span(region[3], region[2], pitches[0]) > (1 << 31)
                    try:
                        for fl in FLAV:
                            for border in ((None, BORDER) if bordered else (None,)):
                                fp = _params(dst, rt, *fl)
                                got = call(v, [arena.handle(p[0]) for p in placed], [arena.handle(p[1]) for p in placed], fp, border, dict(width=w, height=h))
                                torch.cuda.synchronize()
                                for k in range(N_BATCH):
                                    want = _cached((name, k, fl, border), lambda: torch.from_numpy(np.ascontiguousarray(expected(k, fl, border))).cuda())
                                    _same_bits(got[k].contiguous().view(-1).view(torch.uint8), want,
                                               f"{name} output {k}, LDS_KB={kb}, class {cls}, pitches {pitches}, flavour {fl}, border {border}")
                    finally:
                        for p in placed:
                            arena.erase(p[0])
                            arena.erase(p[1])
        finally:
            v.Close()


def test_a_tensor_form_reads_such_planes_too(vpp, oracle, arena, tile_frames):
    """tsvpp_convert_warp_tensor, fp16 with the ImageNet statistics: the sampler is the one above, the store is not what this is about"""
    host, tight = tile_frames["whole"], tile_frames["whole_dev"]
    dst = (112, 80)
    m = [tuple(_rotated(TW, TH, 20.0 + 25 * k, dst)) for k in range(N_BATCH)]
    mean, std = T.SPECS["imagenet"]
    for cls in "AB":
        pitches = _class_pitches((0, 0, TW, TH), (0, 6), cls)
        placed = _place_frames(arena, tight, (0, 0, TW, TH), pitches)
        try:
            got = vpp.convert_warp([arena.handle(p[0]) for p in placed], [arena.handle(p[1]) for p in placed], [(k,) + m[k] for k in range(N_BATCH)],
                                   _params(dst, BILINEAR, RGB24, PLANAR, True), border=BORDER, width=TW, height=TH, dtype=torch.float16, mean=mean, std=std)
            torch.cuda.synchronize()
            for k in range(N_BATCH):
                virtual = W.virtual_frame(host[k][0], host[k][1], TW, TH, m[k], dst[0], dst[1], BORDER)
                want = T.expected(R.expected_planar_f32(oracle, virtual, RGB24), 3, T.SPECS["imagenet"], T.F16)
                assert np.array_equal(T.bits(got[k]), want), f"warp tensor output {k}, class {cls}, pitches {pitches}"
        finally:
            for p in placed:
                arena.erase(p[0])
                arena.erase(p[1])


# ---- outputs between 2^31 and 2^32 bytes ------------------------------------------------------------------------------------------------------------------------------
SMALL = (640, 480)
PAST31 = (16384, 10924)    # x 3 fp32: 2 147 745 792 bytes, just past 2^31
UNDER32 = (16384, 21844)   # x 3 fp32: 4 294 705 152 bytes, just under 2^32
Y800_PAST31 = (32768, 16386)   # x 1 fp32
U8_PAST31 = (32768, 21846)     # x 3 uint8: 2 147 549 184 bytes
NV12_PAST31 = (16384, 21846)   # x 1.5 fp32: 2 147 549 184 bytes
UYVY_PAST31 = (16384, 16386)   # x 2 fp32: 2 147 745 792 bytes


def _tiled(block_y, block_uv, w, h):
    """a w x h frame that repeats a seeded block (a gigabyte of noise costs more to make than to convert)"""
    bh, bw = block_y.shape
    y = np.tile(block_y, ((h + bh - 1) // bh, (w + bw - 1) // bw))[:h, :w]
    uv = np.tile(block_uv, ((h // 2 + bh // 2 - 1) // (bh // 2), (w + bw - 1) // bw))[:h // 2, :w]
    return np.ascontiguousarray(y), np.ascontiguousarray(uv)


def _holds(selection, record, what):
    """the launch (or, for the tile calls, which keep no launch record, the describe answer for the same request) is the routine the case stands for: every key of
    `record`.  Only in a run without A/B knobs -- under one the selection is the knob's, and the bits are what counts."""
    ran = " ".join(f"{k}={selection[k]}" for k in ("kernel", "nt", "pass2") if k in selection)
    if not knob_run():
        for k, v in record.items():
            assert selection.get(k) == v, f"{what}: selected {ran}; the case stands for {k}={v}"
    return ran


def _launched(record, what):
    import tensor_stream as ts
    return _holds(ts.vpp.debug_last_launch(), record, what)


def _big(arena, name, launches, expected, nbytes, off=0):
    """calls whose single output is arena[MARGIN + off, + nbytes), one after the other: after each, both margins still the fill byte and the output the expected
    bits (computed once, whatever the number of launches).  launches: [(label, launch(out), selected(what) -> text)] -- `selected` checks which routine ran"""
    assert (1 << 31) < nbytes < (1 << 32), nbytes
    lo = AU.MARGIN + off
    hi = lo + nbytes
    end = (hi + 7) // 8 * 8
    AU.check_margins(lo, nbytes)
    assert end + 16 <= AU.ARENA_BYTES
    out = arena.buf[lo: hi]
    want_dev = None
    try:
        for label, launch, selected in launches:
            what = name + (" / " + label if label else "")
            t0 = time.perf_counter()
            launch(out)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ran = selected(what)
            before = arena.untouched(0, AU.MARGIN) and bool((arena.buf[AU.MARGIN: lo] == AU.FILL).all())
            after = bool((arena.buf[hi: end] == AU.FILL).all()) and arena.untouched(end, AU.ARENA_BYTES)
            assert before, f"{what}: the 2^32 bytes in front of the output were written, first at {arena.first_touched(0, lo) - lo} bytes from its start"
            assert after, f"{what}: the bytes behind the output were written, first {arena.first_touched(hi, AU.ARENA_BYTES) - hi} bytes behind its end"
            t2 = time.perf_counter()
            if want_dev is None:
                want = expected()
                assert want.dtype == np.uint8 and want.size == nbytes, (want.dtype, want.size, nbytes)
                t3 = time.perf_counter()
                want_dev = torch.from_numpy(want).to(out.device)
                del want
            else:
                t3 = t2
            _same_bits(out, want_dev, what)
            print(f"{what}: {nbytes} bytes{' at +' + str(off) if off else ''}, {ran}, call {t1 - t0:.2f} s, expected bits {t3 - t2:.2f} s, "
                  f"upload and compare {time.perf_counter() - t3:.2f} s")
            out.fill_(AU.FILL)
    finally:  # the arena as the next test expects it, whatever this one did to it
        del want_dev
        arena.buf[AU.MARGIN: end + 16].fill_(AU.FILL)
        if not arena.untouched(0, AU.MARGIN):
            arena.buf[:AU.MARGIN].fill_(AU.FILL)
        if not arena.untouched(end + 16, AU.ARENA_BYTES):
            arena.buf[end + 16:].fill_(AU.FILL)


def _convert_case(vpps, oracle, arena, name, src, dst, rt, fcc, planes, norm, record, off=0, exact_index=False, dev_src=None):
    """`vpps`: one processor, or [(label, processor, record)] that run the same request one after the other (contexts with knobs of their own) against the same
    expected bits.  `record`: what tsvpp_debug_last_launch must answer (_holds).  `dev_src`: the source's planes on the device, where the caller has them."""
    y, uv = src
    h, w = y.shape
    fp = _params(dst, rt, fcc, planes, norm)
    if not isinstance(vpps, list):
        vpps = [("", vpps, record)]
    nbytes = int(vpps[0][1]._lib.tsvpp_out_bytes(ctypes.byref(fp.parameters), w, h))
    ty, tuv = dev_src if dev_src else (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())

    def expected():
        oracle.set_exact_index(exact_index)  # (sources of more than 2^24 samples: the kernels index with integers, tests/test_gpu_edges.py::test_8k_frame)
        try:
            ref, _, _ = oracle.convert(y, uv, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=16)
        finally:
            oracle.set_exact_index(False)
        return ref.view(np.uint8).ravel()

    _big(arena, name, [(label, lambda out, v=v: v.Convert(ty, tuv, fp, out=out), lambda what, r=r: _launched(r, what)) for label, v, r in vpps], expected, nbytes, off)


@pytest.fixture(scope="module")
def small():
    return synth_nv12(SMALL[0], SMALL[1], seed=9000)


POINT, TWO_TAP, ELEMENTWISE = "vpp_point_kernel<PK_NEAREST,OUT>", "vpp_bilinear_kernel<bilinear,OUT>", "vpp_fused_gather_kernel<MODE,OUT,false>"
# (id, dst, resize type, fourcc, planes, normalization, offset of the output from 16-byte alignment, the launch record the case stands for).  The store routines
# S1 .. S11 are those of profiles/addressing_limits.txt, section 4.
UPSCALES = [
    ("bilinear-f32-planar-under-2^32", UNDER32, BILINEAR, BGR24, PLANAR, True, 0, dict(kernel=TWO_TAP, nt=1)),   # S2: plane-major non-temporal stores
    ("nearest-f32-planar-under-2^32", UNDER32, NEAREST, RGB24, PLANAR, True, 0, dict(kernel=POINT, nt=1)),       # S1: plane bases + 32-bit offsets (and nt=0, below)
    ("nearest-f32-merged-under-2^32", UNDER32, NEAREST, BGR24, MERGED, True, 0, dict(kernel=POINT, nt=1)),       # S3: the in-wave exchange of the merged fp32 rows
    ("bilinear-f32-planar-elementwise", PAST31, BILINEAR, RGB24, PLANAR, True, 4, dict(kernel=ELEMENTWISE)),     # S4: an output 4 bytes off 16-byte alignment
    ("nearest-hsv", PAST31, NEAREST, HSV, MERGED, True, 0, dict(kernel=POINT, nt=1)),                            # S3
    ("nearest-nv12-f32", NV12_PAST31, NEAREST, NV12, PLANAR, True, 0, dict(kernel=POINT, nt=1)),                 # S6
    ("nearest-uyvy-f32", UYVY_PAST31, NEAREST, UYVY, PLANAR, True, 0, dict(kernel=POINT, pass2="fmt_uyvy")),     # S9: two passes, the format kernel's flat index
    ("nearest-y800-f32", Y800_PAST31, NEAREST, Y800, PLANAR, True, 0, dict(kernel=POINT, nt=1)),                 # S6
    ("nearest-u8-planar", U8_PAST31, NEAREST, RGB24, PLANAR, False, 0, dict(kernel=POINT, nt=1)),                # S5
    ("nearest-u8-merged", U8_PAST31, NEAREST, BGR24, MERGED, False, 0, dict(kernel=POINT, nt=1)),                # S5
]


@pytest.mark.parametrize("case", UPSCALES, ids=[c[0] for c in UPSCALES])
def test_an_up_scale_stores_an_output_past_2_31_bytes(vpp, oracle, arena, small, monkeypatch, case):
    import tensor_stream as ts
    name, dst, rt, fcc, planes, norm, off, record = case
    if name != "nearest-f32-planar-under-2^32":
        _convert_case(vpp, oracle, arena, name, small, dst, rt, fcc, planes, norm, record, off)
        return
    # At 16384 columns the selection gives every vector fp32 launch non-temporal stores (vpp_select.hip: sel_store_policy), whose `nt` forms are inline assembly.
    # The PLAIN vector form of st4o -- base + (uint32_t) offset in C++ -- runs above 2^31 only here: the same request in a context of its own with TSVPP_NT=0,
    # against the same expected bits.
    monkeypatch.setenv("TSVPP_NT", "0")
    plain = ts.VideoProcessor(device=0, max_consumers=1)  # (the knobs are read when a processor is made)
    monkeypatch.undo()
    try:
        _convert_case([("", vpp, record), ("TSVPP_NT=0", plain, dict(kernel=POINT, nt=0))], oracle, arena, name, small, dst, rt, fcc, planes, norm, None, off)
    finally:
        plain.Close()


def test_the_colour_only_conversion_stores_an_output_past_2_31_bytes(vpp, oracle, arena, small):
    """no resize: the source is the output's size (S1 from vpp_color_kernel: its `sc1` stores with a scalar base and a 32-bit offset)"""
    _convert_case(vpp, oracle, arena, "colour-only-f32-planar", _tiled(small[0], small[1], *PAST31), (0, 0), NEAREST, RGB24, PLANAR, True,
                  dict(kernel="vpp_color_kernel<OUT>", nt=2))


def test_an_exact_2_to_1_down_scale_stores_an_output_past_2_31_bytes(vpp, oracle, arena, small):
    src = _tiled(small[0], small[1], 2 * PAST31[0], 2 * PAST31[1])
    _convert_case(vpp, oracle, arena, "bilinear-2:1-f32-planar", src, PAST31, BILINEAR, BGR24, PLANAR, True, dict(kernel=TWO_TAP, nt=1), exact_index=True)


def test_an_exact_1_to_2_up_scale_stores_a_merged_uint8_output_past_2_31_bytes(vpp, oracle, arena, small):
    """S7, r32_store_tile (vpp_r32_store.h), the output side the streaming kernels share: vpp_rep2_kernel is NEAREST at exactly 1 : 2.  Its merged uint8 rows
    leave as exchanged 16-byte non-temporal stores (bc_st16 -> st16_nt, inline assembly) at byte offsets 3 * pixel up to 2.1 GB -- the one flavour of S7 whose
    offsets pass 2^31 at a legal size besides fp32 merged: the planar ones count per plane.  32768 x 21848 is the least exact double of an even source height
    past 2^31 bytes (the 21846 rows of the other uint8 cases are twice an odd 10923)."""
    w, h = PAST31
    assert 3 * 2 * w * 2 * h > (1 << 31) > 3 * 2 * w * 2 * (h - 2)
    _convert_case(vpp, oracle, arena, "nearest-1:2-u8-merged", _tiled(small[0], small[1], w, h), (2 * w, 2 * h), NEAREST, BGR24, MERGED, False,
                  dict(kernel="vpp_rep2_kernel<OUT>", nt=1), exact_index=True)


def test_the_single_pass_uyvy_fp32_of_the_streaming_kernel_stores_an_output_past_2_31_bytes(vpp, oracle, arena, small):
    """S8, the stores vpp_bilinear_r32.hip keeps to itself: BILINEAR at exactly 3 : 2 makes UYVY fp32 in one pass, a run's rows exchanged through LDS and stored at
    (2 * pixel + 4 g) * 4 bytes.  16384 x 16388 (8 bytes per pixel, 2 148 007 936) is the least height past 2^31 bytes that is a multiple of 4, which the
    streaming kernels need; its uint8 flavours pass 2^31 only from sources of 2.4 GB (profiles/addressing_limits.txt)."""
    dst = (16384, 16388)
    src = _tiled(small[0], small[1], dst[0] * 3 // 2, dst[1] * 3 // 2)
    _convert_case(vpp, oracle, arena, "bilinear-3:2-uyvy-f32", src, dst, BILINEAR, UYVY, PLANAR, True,
                  dict(kernel="vpp_bilinear_r32_kernel<OUT,bilinear,3:2>", nt=1), exact_index=True)


def test_remap_reads_a_map_past_2_31_bytes_and_stores_an_output_just_under_2_32(vpp, oracle, arena, small):
    """the identity map, built on the device, of the largest legal fp32 output: 2.86 GB of map rows addressed by row * pitch, 4.29 GB stored.  include/tsvpp.h: the
    identity map with dst equal to the frame is tsvpp_convert without a resize (tests/test_gpu_remap.py pins it), so the oracle supplies the expected bits."""
    import tensor_stream as ts
    w, h = UNDER32
    y, uv = _tiled(small[0], small[1], w, h)
    ty, tuv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    xy = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
    xy[..., 0] = torch.arange(w, dtype=torch.float32, device="cuda")[None, :]
    xy[..., 1] = torch.arange(h, dtype=torch.float32, device="cuda")[:, None]
    assert xy.numel() * 4 > (1 << 31)
    fp = _params((w, h), BILINEAR, RGB24, PLANAR, True)

    def expected():
        ref, _, _ = oracle.convert(y, uv, fourcc=RGB24, planes=PLANAR, normalization=True, nthreads=16)
        return ref.view(np.uint8).ravel()

    said = lambda what: _holds(ts.describe_remap(fp, UNDER32, (0, 0)), dict(kernel="vpp_remap<O_F32_PLANAR,vec,staged,replicate>", nt=1), what)
    _big(arena, "remap-identity-f32-planar-under-2^32", [("", lambda out: vpp.convert_remap(ty, tuv, xy, fp, out=[out]), said)], expected, 3 * w * h * 4)


def test_letterbox_stores_a_canvas_past_2_31_bytes(vpp, oracle, arena, small):
    """the inner rectangle against the oracle, the pad as the constant the colour back end makes of it (tests/letterbox_util.py)"""
    import tensor_stream as ts
    w, h = PAST31
    y, uv = small
    ty, tuv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    fp = _params((w, h), BILINEAR, BGR24, PLANAR, True)
    rect = L.default_rect(SMALL[0], SMALL[1], w, h)
    assert rect[2] < w or rect[3] < h
    said = lambda what: _holds(ts.describe_letterbox(fp, SMALL), dict(kernel="vpp_letterbox<M_BILINEAR,O_F32_PLANAR,vec,staged>", nt=1), what)
    _big(arena, "letterbox-f32-planar", [("", lambda out: vpp.convert_letterbox([ty], [tuv], fp, pad=(114, 128, 128), out=[out]), said)],
         lambda: L.expected_canvas(oracle, y, uv, SMALL[0], SMALL[1], rect, (w, h), BILINEAR, BGR24, PLANAR, True, (114, 128, 128)), 3 * w * h * 4)


def test_a_tensor_form_stores_an_fp32_output_past_2_31_bytes(vpp, oracle, arena, small):
    """tsvpp_convert_rois_tensor, fp32 with the ImageNet statistics: tensor_store_tile's plane bases and 32-bit offsets"""
    import tensor_stream as ts
    w, h = PAST31
    y, uv = small
    ty, tuv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    fp = _params((w, h), NEAREST, RGB24, PLANAR, True)
    mean, std = T.SPECS["imagenet"]

    def expected():
        q, _, _ = oracle.convert(y, uv, dst=(w, h), resize_type=NEAREST, fourcc=RGB24, planes=PLANAR, normalization=True, nthreads=16)
        return T.expected(q, 3, T.SPECS["imagenet"], T.F32)

    box = [(0, 0, SMALL[0], SMALL[1])]
    said = lambda what: _holds(ts.describe_rois(fp, SMALL, box, dtype=torch.float32, mean=mean, std=std),
                               dict(kernel="vpp_rois_tensor<M_NEAREST,PLANAR,EL_F32,vec,staged>", nt=1), what)
    _big(arena, "rois-tensor-f32", [("", lambda out: vpp.convert_rois(ty, tuv, box, fp, out=[out], dtype=torch.float32, mean=mean, std=std), said)], expected, 3 * w * h * 4)
