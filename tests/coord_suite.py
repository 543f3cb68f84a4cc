"""What the GPU tests of the coordinate paths (warp, perspective, remap, mesh) share: the frames and output sizes, the cache of the model's virtual frames, the
one comparison against the model, and the bodies of the cases every path has.  A path's file names its DESCRIPTOR (Path below) and calls these bodies from
tests of a line or two; what only that path has stays in its file.  A helper module, not a conftest: a file binds `frames = cs.frames_fixture(seed)` itself.

The descriptors are tests/coord_paths.py's.  Their fields:
  name            "warp": VideoProcessor.convert_warp, tensor_stream.describe_warp, tsvpp_convert_warp
  model           the name its virtual frames are cached under (mesh samples through remap's model: "remap")
  LIMIT           outputs per launch
  call(v, ys, uvs, items, fp, **kw)          the convert call for `items`, the path's own form of a request (rows of coefficients; tables and (frame, table))
  describe(fp, geo, items, **kw)             the describe call for the same
  output(items, i, dst)                      output i -> (frame, model argument, cache tag, words for a message)
  virtual_frame(y, uv, w, h, arg, dst, border), expected(oracle, arg, dst, fcc, planes, norm, border, virtual)   the model (tests/*_util.py)
  pick(picks, geo, dst)                      the items of [(frame, name in the frame's item set)]
  staging(), split_items(geo), guard_items(dst), gterm_items(dst), capture_items(step, geo), capture_dst, resident(items), overwrite(items, now)
                                             the requests of the shared cases (see each body); None where a path writes a case out itself
  valid(w, h), on_frame(items, k), broken(items), refusals(call, items), records(N, items)   the status-code and refusal cases (see those bodies)"""
import ctypes
import dataclasses
import types

import numpy as np
import pytest
import torch

import tensor_util as T
from guard_util import GUARD, arena  # noqa: F401  (GUARD: part of this module's vocabulary)
from letterbox_util import BGR24, BILINEAR, MERGED, PLANAR, RGB24, Y800, bits
from util import frame_k, knob_run, synth_nv12

# (width, height, pitch): landscape, portrait, a frame several tiles' footprints large, one smaller than a tile
GEO = [(128, 72, 192), (72, 128, 96), (322, 182, 384), (32, 18, 48)]
# 70 x 66: 4 k + 2 columns (the shifted tile column); 30 x 34: narrower than a tile (element-wise stores)
DSTS = [(64, 64), (70, 66), (30, 34), (112, 112)]
BORDERS = [None, (114, 128, 128), (3, 250, 7)]
FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]  # what the tensor calls store

@dataclasses.dataclass(frozen=True)
class Path:
    """a descriptor: every field above is required, so a path that lacks one fails when tests/coord_paths.py is imported, not in the middle of a GPU run"""
    name: str
    model: str
    LIMIT: int
    call: object
    describe: object
    output: object
    virtual_frame: object
    expected: object
    pick: object
    staging: object
    split_items: object
    guard_items: object
    gterm_items: object
    capture_items: object
    capture_dst: tuple
    resident: object
    overwrite: object
    valid: object
    on_frame: object
    broken: object
    refusals: object
    records: object


Tables = types.SimpleNamespace  # the request of remap and mesh: tables [(name, host array)], remaps [(frame, table)], dev (the device tables, or None: upload)


def params(ts, dst, fcc, planes, norm, rt=BILINEAR):
    return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


def tensor_params(dst, fcc, planes, norm=True):
    """params() as the tensor forms take them: normalised unless a refusal is being asked for"""
    import tensor_stream as ts
    return params(ts, dst, fcc, planes, norm)


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_frames(geo, seed):
    host = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    return host, [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]


def frames_fixture(seed):
    """the module-scoped fixture `frames`: the frames of GEO from `seed`, [(y, uv)] on the host, the same on the device"""
    @pytest.fixture(scope="module")
    def frames():
        return device_frames(GEO, seed)
    return frames


_virtual = {}


def virtual(path, host, k, geo, arg, tag, dst, border, key=None):
    """the virtual frame of (frame k, the item `tag` names, dst, border), computed once per session; key: the cache key of frame k's content, where it is not GEO's"""
    kk = (path.model, key if key is not None else k, geo[k][:2], tag, dst, border)
    if kk not in _virtual:
        _virtual[kk] = path.virtual_frame(host[k][0], host[k][1], geo[k][0], geo[k][1], arg, dst, border)
    return _virtual[kk]


def check(path, v, oracle, host, dev, geo, items, dst, fcc, planes, norm, border=None, out=None, only=None, what="", key=None):
    """one convert call of `path` for `items`; the outputs (all, or the indices `only`) are the model's, byte for byte; returns the output tensor.
    key: frame index -> cache key of that frame's content"""
    import tensor_stream as ts
    got = path.call(v, [d[0] for d in dev], [d[1] for d in dev], items, params(ts, dst, fcc, planes, norm), border=border, out=out,
                    width=[g[0] for g in geo], height=[g[1] for g in geo])
    torch.cuda.synchronize()
    for i in (range(len(got)) if only is None else only):
        k, arg, tag, words = path.output(items, i, dst)
        ref = path.expected(oracle, arg, dst, fcc, planes, norm, border, virtual(path, host, k, geo, arg, tag, dst, border, None if key is None else key(k)))
        g = bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (f"{what} output {i}: frame {k} {geo[k]} {words} -> {dst} fcc={fcc} planes={planes} norm={norm} border={border}: {bad.size} bytes differ, "
                               f"first at {bad[:4]}")
    return got


def check_tensor(path, v, oracle, host, dev, items, dst, fcc, planes, dtype, spec, border, what=""):
    """the tensor form of the call on the frames of GEO: every element is tests/tensor_util.py's image of the fp32 value the plain call stores"""
    channels = 1 if fcc == Y800 else 3
    got = path.call(v, [d[0] for d in dev], [d[1] for d in dev], items, tensor_params(dst, fcc, planes), border=border, width=[g[0] for g in GEO], height=[g[1] for g in GEO],
                    dtype=T.TORCH[dtype], mean=T.SPECS[spec][0], std=T.SPECS[spec][1])
    torch.cuda.synchronize()
    assert got.dtype == T.TORCH[dtype]
    for i in range(len(got)):
        k, arg, tag, words = path.output(items, i, dst)
        q = path.expected(oracle, arg, dst, fcc, planes, True, border, virtual(path, host, k, GEO, arg, tag, dst, border)).view(np.float32)
        ref = T.expected(q, channels, T.SPECS[spec], dtype)
        g = T.bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} output {i}: frame {k} {words} -> {dst} fcc={fcc} {dtype} {spec} border={border}: {bad.size} bytes differ, first at {bad[:4]}"
    return got


def staged_gather_and_mixed_launches(path, oracle, frames, monkeypatch):
    """path.staging() -> (dst, [(TSVPP_LDS_KB or None, items, expect)]): a context per run (the variable is read when one is created), expect(d) judges the
    describe line, and every run gives the same bits, the model's"""
    import tensor_stream as ts
    host, dev = frames
    dst, runs = path.staging()
    fp = params(ts, dst, BGR24, PLANAR, True)
    results = []
    for n, (kb, items, expect) in enumerate(runs):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        else:
            monkeypatch.delenv("TSVPP_LDS_KB", raising=False)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            if not knob_run(("TSVPP_LDS_KB",)):
                expect(path.describe(fp, GEO, items))
            got = check(path, v, oracle, host, dev, GEO, items, dst, BGR24, PLANAR, True, what=f"run {n} LDS_KB={kb}")
            results.append(bits(got))
            check(path, v, oracle, host, dev, GEO, items, dst, RGB24, MERGED, False, border=(114, 128, 128), what=f"run {n} LDS_KB={kb}")
        finally:
            v.Close()
    for r in results[1:]:
        assert np.array_equal(results[0], r), "staged, gathering, mixed and hinted launches differ"


def splitting_over_launches(path, vpp, oracle, frames, n):
    """one call, a frame of its own per output -- different sizes and pitches, distinct content (every byte + 37 k) --: the first and the last output of every
    launch are right.  path.split_items(geo) -> (dst, items): output k samples frame k"""
    host, dev = frames
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    dst, items = path.split_items(geo)
    only = sorted({0, n - 1} | {k for k in (path.LIMIT - 1, path.LIMIT, 2 * path.LIMIT - 1, 2 * path.LIMIT) if k < n})
    check(path, vpp, oracle, h, d, geo, items, dst, BGR24, PLANAR, True, only=only, what=f"n={n}", key=lambda k: ("split", k))
    check(path, vpp, oracle, h, d, geo, items, dst, RGB24, MERGED, False, border=(114, 128, 128), only=only, what=f"n={n}", key=lambda k: ("split", k))


GUARD_DSTS = [(64, 64), (70, 66), (30, 34)]
GUARD_FLAVOURS = [(BGR24, PLANAR, True, 0), (BGR24, PLANAR, True, 4), (RGB24, MERGED, True, 4), (RGB24, MERGED, False, 0),
                  (RGB24, MERGED, False, 1), (BGR24, PLANAR, False, 1), (Y800, MERGED, False, 1), (RGB24, MERGED, True, 0)]  # fcc, planes, norm, off


def unaligned_outputs_and_guard_bytes(path, vpp, oracle, frames, fcc, planes, norm, off, dst):
    """outputs 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were.
    path.guard_items(dst): two outputs per frame of GEO"""
    import tensor_stream as ts
    host, dev = frames
    items = path.guard_items(dst)
    n = 2 * len(GEO)
    nbytes = (1 if fcc == Y800 else 3) * dst[0] * dst[1] * (4 if norm else 1)
    _, slots, verify = arena([nbytes] * n, off, what="output", where=f"dst {dst}")
    out = [s.view(torch.float32) if norm else s for s in slots]
    check(path, vpp, oracle, host, dev, GEO, items, dst, fcc, planes, norm, border=(114, 128, 128), out=out, what=f"offset {off}")
    verify()
    if not knob_run():
        d = path.describe(params(ts, dst, fcc, planes, norm), GEO, items, border=(114, 128, 128), aligned_outputs=(off == 0))
        assert d["kernel"].split(",")[1] == ("vec" if off == 0 and dst[0] >= 32 else "elem")
        assert d["tail"] == (2 if (off == 0 and dst[0] == 70) else 0)


CT_RESIZE, CT_INNER = 1 | 2 | 8 | 16 | 64, 256  # the oracle's contraction bits, as tests/test_gpu_parity.py sets them


def colour_g_term_variants(path, oracle, frames, g_term, ct_bits):
    """TSVPP_OPT_COLOR_G_TERM against the oracle's matching contraction variant, border included, then the default again; everything restored afterwards.
    path.gterm_items(dst): two outputs per frame of GEO"""
    import tensor_stream as ts
    from tensor_stream import vpp as V
    host, dev = frames
    dst = (64, 64)
    items = path.gterm_items(dst)
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        try:
            check(path, v, oracle, host, dev, GEO, items, dst, RGB24, PLANAR, False, border=(77, 201, 33))
            check(path, v, oracle, host, dev, GEO, items, dst, BGR24, MERGED, True, border=(77, 201, 33))
        finally:
            oracle.set_contract(-1)
        v.set_option(V.OPT_COLOR_G_TERM, 0)
        check(path, v, oracle, host, dev, GEO, items, dst, RGB24, PLANAR, False, border=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def graph_capture_replays(path, vpp, oracle, seed):
    """the records travel in the kernarg segment (and hold the tables' ADDRESSES, where the path has tables): the call allocates, copies and synchronises nothing,
    is legal during capture (one kernel node), and the graph replays the captured request on whatever the frames -- and the tables -- hold at replay time, onto
    re-poisoned outputs.  path.capture_items(step, geo): the request at capture (step 0) and what replay `step` finds in its place; path.resident(items) puts the
    tables on the device, path.overwrite(items, now) replaces their content"""
    import tensor_stream as ts
    geo = [GEO[0], GEO[1], GEO[2]]
    dst = path.capture_dst
    border = (114, 128, 128)
    a, dev = device_frames(geo, seed)
    items = path.resident(path.capture_items(0, geo))
    fp = params(ts, dst, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, dst[0], dst[1], 2 * len(geo))
    kw = dict(width=[g[0] for g in geo], height=[g[1] for g in geo], out=out, border=border)
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        path.call(vpp, ys, uvs, items, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        path.call(vpp, ys, uvs, items, fp, **kw)
    for step in (1, 2):
        b = [synth_nv12(w, h, seed=seed + 10 * step + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
        for k in range(len(geo)):
            dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
            dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
        now = path.capture_items(step, geo)
        path.overwrite(items, now)
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for i in range(len(out)):
            k, arg, _, _ = path.output(now, i, dst)
            ref = path.expected(oracle, arg, dst, RGB24, MERGED, False, border, path.virtual_frame(b[k][0], b[k][1], geo[k][0], geo[k][1], arg, dst, border))
            assert np.array_equal(bits(out[i]), ref), (seed + 10 * step, i)


def status_codes_with_a_live_context(path, vpp, frames):
    """the validation of the path's CPU test file answers before any launch: what every path refuses, then path.refusals(call, items) for its own; at
    the C entry point a null plane, a null output, a null output list and a null context are TSVPP_ERROR.  path.valid(w, h) -> the items of one output at
    64 x 64; path.on_frame(items, k): the same from frame k; path.records(N, items) -> (the entry point's arguments between the frames and the parameters, the
    path's own checks there, a function of raw(ctx, outs) -> status, the context and the outputs)"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    y, uv = dev[0]
    w, h, pitch = GEO[0]
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    items = path.valid(w, h)
    one = dict(width=w, height=h)

    def call(items=items, fp=fp, **kw):
        return path.call(vpp, y, uv, items, fp, **{**one, **kw})
    with pytest.raises(RuntimeError, match="-3"):
        call(path.on_frame(items, 1))
    with pytest.raises(RuntimeError, match="-3"):
        call(border=(256, 128, 128))
    path.refusals(call, items)
    for rt in (0, 2, 3):  # NEAREST, BICUBIC, AREA: follow-ups
        with pytest.raises(RuntimeError, match="-2"):
            call(fp=params(ts, (64, 64), RGB24, MERGED, False, rt=rt))
    with pytest.raises(RuntimeError, match="-2"):
        call(width=w - 1)
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), uv.data_ptr(), pitch, pitch, w, h))
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    records, own = path.records(N, items)
    entry = getattr(N.lib(), "tsvpp_convert_" + path.name)
    p = ctypes.byref(fp.parameters)

    def raw(ctx, outs):
        return entry(ctx, 1, fr, *records, p, -1, -1, -1, outs, None)
    own(raw, vpp._ctx, outs)
    fr[0].uv = None
    assert raw(vpp._ctx, outs) == -3
    fr[0].uv = uv.data_ptr()
    outs[0] = None
    assert raw(vpp._ctx, outs) == -3
    assert raw(vpp._ctx, None) == -3
    outs[0] = out.data_ptr()
    assert raw(None, outs) == -3
    assert raw(vpp._ctx, outs) == 0
    torch.cuda.synchronize()


def identity_fp32_is_the_plain_call(path, vpp, frames, items, dst):
    """mean 0, std 1, float32: (q - 0) * 1 is q -- the tensor call stores the bits of the plain call"""
    host, dev = frames
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO], border=(3, 250, 7))
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    for fcc, planes in FORMATS:
        a = path.call(vpp, ys, uvs, items, tensor_params(dst, fcc, planes), **kw)
        b = path.call(vpp, ys, uvs, items, tensor_params(dst, fcc, planes), dtype=torch.float32, mean=0.0, std=1.0, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(T.bits(a), T.bits(b)), (dst, fcc, planes)


def tensor_refusals(path, vpp, frames, items=None):
    """the tensor form takes planar, normalised requests only and a std that is not zero; the status of path.broken(items), a request wrong in itself, comes first.
    items: one output of frame 0 at 64 x 64 (default: path.valid's)"""
    host, dev = frames
    y, uv = dev[0]
    items = path.valid(GEO[0][0], GEO[0][1]) if items is None else items
    kw = dict(width=GEO[0][0], height=GEO[0][1], dtype=torch.float16)
    with pytest.raises(RuntimeError, match="-2"):
        path.call(vpp, y, uv, items, tensor_params((64, 64), RGB24, MERGED), **kw)
    with pytest.raises(RuntimeError, match="-2"):
        path.call(vpp, y, uv, items, tensor_params((64, 64), RGB24, PLANAR, norm=False), **kw)
    with pytest.raises(RuntimeError, match="-3"):
        path.call(vpp, y, uv, items, tensor_params((64, 64), RGB24, PLANAR), std=0.0, **kw)
    with pytest.raises(RuntimeError, match="-3"):  # rule 1 first: the request's own status
        path.call(vpp, y, uv, path.broken(items), tensor_params((64, 64), RGB24, MERGED), **kw)
    out = path.call(vpp, y, uv, items, tensor_params((64, 64), Y800, MERGED), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 64, 64)
