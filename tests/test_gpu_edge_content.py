"""GPU: every kernel on content that sits on the truncation boundaries -- the classes of tests/edge_content.py (flat frames of four levels, a checkerboard, a
vertical and a horizontal edge, a ramp) in place of the random frames every other bit-exact test draws.  On random content a weight one ulp off or a sum taken in
another order flips one output byte in ~1e5; on a flat 255 frame the reference itself returns 254 for 7 .. 47 % of the samples (tests/test_edge_content_cpu.py),
so the same error flips bytes by the dozen.  Raw-bit equality throughout, against the models the fuzz tests use; no case is skipped, nothing has a tolerance.

    tile and coordinate calls   the nine fuzz families x the eight classes: the calls of chunk 0 (rois_sized: its chunk 0; remap, mesh, letterbox_area, whose
                                generators have no chunks: their first 24 calls) through the fuzz tests' own run / compare / expected -- guards, poisoned slots and
                                tensor forms included -- with every frame replaced by the class
    named AREA cases            edge_content.LETTERBOX_AREA_CASES through convert_letterbox_area, edge_content.ROIS_AREA_CASES through convert_rois_area, at the
                                flat classes and the ramp: uint8 merged, fp32 planar and Y800, one fp16 tensor case each with the ImageNet constants, and once with
                                TSVPP_LDS_KB=0, where every tile gathers from global memory
    Convert                     for every kernel name the grid of tests/dispatch_grid.py reaches, the representative of the name's cheapest signature as a batch of
                                two frames: the class and its complement 255 - x"""
import numpy as np
import pytest
import torch

import dispatch_grid as G
import edge_content as E
import letterbox_area_fuzz as ZA
import rois_sized_fuzz as ZS
import tensor_util as T
import test_gpu_dispatch_cover as C
import test_gpu_letterbox_area as LA
import test_gpu_letterbox_area_fuzz as LF
import test_gpu_mesh_fuzz as MF
import test_gpu_remap_fuzz as RF
import test_gpu_rois_area as RA
import test_gpu_rois_sized_fuzz as SF
import test_gpu_tile_fuzz as TF
import tile_fuzz as F
from letterbox_util import AREA, BGR24, MERGED, PLANAR, Y800, expected_canvas
from util import knob_run

pytestmark = pytest.mark.gpu

FAMILIES = F.FAMILIES + ("rois_sized", "letterbox_area", "remap", "mesh")
FIRST = 24  # calls of a generator that has no chunks: a chunk of tile_fuzz's
# the named cases' flavours: uint8 merged and fp32 planar -- and Y800, the one flavour in which a flat 255 frame shows its boundary: the colour back end maps
# Y = 254 and Y = 255 at U = V = 128 to the same clamped 255 in every RGB channel
NAMED_FLAVOURS = LA.TWO + [(Y800, MERGED, False)]


def run_family(v, oracle, family, name):
    """chunk 0 of the family with every frame replaced by the class `name`; returns the number of calls run"""
    if family in F.FAMILIES:
        calls = [E.with_content(c, name) for c in F.cases(family, 0)]
        for call in calls:
            host = F.host_frames(call)
            TF.compare(call, TF.run(v, call, F.device_frames(host, call)), TF.expected(oracle, call, host))
    elif family == "rois_sized":
        calls = [E.with_content(c, name) for c in ZS.cases(0)]
        for call in calls:
            SF.run_call(v, oracle, call)
    elif family == "letterbox_area":
        calls = [E.with_content(c, name) for c in ZA.cases()[:FIRST]]
        for case in calls:
            LF.run_case(v, oracle, case)
    else:
        mod = {"remap": RF, "mesh": MF}[family]
        calls = [E.with_content(c, name) for c in mod.CALLS_DRAWN[:FIRST]]
        for index, call in enumerate(calls):
            mod.run_call(v, oracle, call, index)
    return len(calls)


@pytest.mark.parametrize("name", E.CLASSES)
@pytest.mark.parametrize("family", FAMILIES)
def test_tile_and_coordinate_calls(vpp, oracle, family, name):
    assert run_family(vpp, oracle, family, name) == (ZS.CALLS if family == "rois_sized" else FIRST)


# ---- the named AREA cases -----------------------------------------------------------------------------------------------------------------------------------

def letterbox_area_case(v, oracle, case, name, key):
    (w, h, pitch), canvas, rect = E.LETTERBOX_AREA_CASES[case]
    y, uv = E.frame(name, w, h, pitch, pitch)
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())]
    for fcc, planes, norm in NAMED_FLAVOURS:
        LA.check(v, oracle, [(y, uv)], dev, [(w, h, pitch)], canvas, fcc, planes, norm, rects=[rect], key=(key, case, name), what=f"{name} case {case}")
    return (y, uv), dev


@pytest.fixture(scope="module")
def rois_area_frames():
    """class -> ((y, uv) on the host, the same on the device) of the ROIS_AREA_FRAME frame"""
    w, h, pitch = E.ROIS_AREA_FRAME
    out = {}
    for name in E.NAMED_CLASSES:
        y, uv = E.frame(name, w, h, pitch, pitch)
        out[name] = ((y, uv), (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()))
    return out


def rois_area_case(v, oracle, frames, case, name):
    box, dst = E.ROIS_AREA_CASES[case]
    host, dev = frames[name]
    for fcc, planes, norm in NAMED_FLAVOURS:
        RA.check_rois(v, oracle, [host], [dev], [box], dst, fcc, planes, norm, widths=E.ROIS_AREA_FRAME[0], what=f"{name} case {case}")


@pytest.mark.parametrize("name", E.NAMED_CLASSES)
@pytest.mark.parametrize("case", range(len(E.LETTERBOX_AREA_CASES)))
def test_named_letterbox_area_cases(vpp, oracle, case, name):
    letterbox_area_case(vpp, oracle, case, name, "edge")


@pytest.mark.parametrize("name", E.NAMED_CLASSES)
@pytest.mark.parametrize("case", range(len(E.ROIS_AREA_CASES)))
def test_named_rois_area_cases(vpp, oracle, rois_area_frames, case, name):
    rois_area_case(vpp, oracle, rois_area_frames, case, name)


def test_named_area_cases_as_fp16_tensors(vpp, oracle, rois_area_frames):
    """322 x 182 -> 70 x 66 through both calls, flat (200, 90, 240) -- G and B stay inside 0 .. 255, so the boundary shows in them: fp16 elements of
    (q - mean[c]) * scale[c] with the ImageNet constants, q the fp32 planar result"""
    import tensor_stream as ts
    name, dtype, spec = "flat_200_90_240", T.F16, T.IMAGENET
    kw = dict(dtype=T.TORCH[dtype], mean=spec[0], std=spec[1])
    (w, h, pitch), canvas, rect = E.LETTERBOX_AREA_CASES[5]
    assert (w, h, rect[2:]) == (322, 182, (70, 66))
    y, uv = E.frame(name, w, h, pitch, pitch)
    got, _ = vpp.convert_letterbox_area([torch.from_numpy(y).cuda()], [torch.from_numpy(uv).cuda()], LA.params(ts, canvas, BGR24, PLANAR, True), rects=[rect],
                                        width=w, height=h, **kw)
    torch.cuda.synchronize()
    q = expected_canvas(oracle, y, uv, w, h, rect, canvas, AREA, BGR24, PLANAR, True, LA.GRAY).view(np.float32)
    assert got[0].dtype == torch.float16 and np.array_equal(T.bits(got[0]), T.expected(q, 3, spec, dtype))
    box, dst = E.ROIS_AREA_CASES[4]
    assert (box[2] - box[0], box[3] - box[1], dst) == (322, 182, (70, 66))
    (hy, huv), (dy, duv) = rois_area_frames[name]
    got = vpp.convert_rois_area([dy], [duv], [box], RA.params(ts, dst, BGR24, PLANAR, True), width=E.ROIS_AREA_FRAME[0], **kw)
    torch.cuda.synchronize()
    q = RA.expect(oracle, hy, huv, box, dst, BGR24, PLANAR, True).view(np.float32)
    assert got[0].dtype == torch.float16 and np.array_equal(T.bits(got[0]), T.expected(q, 3, spec, dtype))


def test_named_area_cases_without_an_lds_budget(oracle, rois_area_frames, monkeypatch):
    """TSVPP_LDS_KB=0 (read when a context is created): every tile gathers from global memory, the weight rows still live in LDS -- the gathering sampler sees the
    same content: every named case at flat 255 and the ramp"""
    import tensor_stream as ts
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        if not knob_run(("TSVPP_LDS_KB",)):
            (w, h, pitch), canvas, rect = E.LETTERBOX_AREA_CASES[5]
            d = ts.describe_letterbox_area(LA.params(ts, canvas, BGR24, PLANAR, True), [(w, h, pitch)], rects=[rect])
            assert d["staged"] == 0 and d["kernel"].endswith("gather>")
        for name in ("flat_255_128_128", "ramp"):
            for case in range(len(E.LETTERBOX_AREA_CASES)):
                letterbox_area_case(v, oracle, case, name, "edge")
            for case in range(len(E.ROIS_AREA_CASES)):
                rois_area_case(v, oracle, rois_area_frames, case, name)
    finally:
        v.Close()


# ---- Convert: every kernel name of the dispatch grid ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kernels():
    """family -> [(kernel name, request)]: per kernel name the grid reaches, the representative of its cheapest signature by dispatch_grid.oracle_bytes.  The
    request runs as a batch of two frames where describe still names the kernel for two, with the representative's own frame count where it does not"""
    cheapest = {}
    for sig in sorted(G.signatures()):
        req = G.representative(sig)
        cost = (G.oracle_bytes(req), sig)
        name = G.kernel_name(sig)
        if name not in cheapest or cost < cheapest[name][0]:
            cheapest[name] = (cost, req)
    desc = G._Describer()
    by_family = {}
    for name, (_, req) in sorted(cheapest.items()):
        two = desc(req[:7] + (2, req[8]))
        if two is not None and two["kernel"] == name:
            req = req[:7] + (2, req[8])
        assert desc(req)["kernel"] == name
        by_family.setdefault(name.split("<")[0], []).append((name, req))
    return by_family


def _poison_outside_the_crop(y, uv, crop, p):
    """what test_gpu_dispatch_cover._fill_inputs does to a cropped frame: everything outside the legal footprint holds p, the pitch padding included"""
    l, t, r, b = crop
    y[:t] = p
    y[b:] = p
    y[:, :l] = p
    y[:, r:] = p
    c0, c1 = t // 2, t // 2 + (b - t) // 2
    uv[:c0] = p
    uv[c1:] = p
    uv[:, :l] = p
    uv[:, r:] = p


def run_convert(v, oracle, kernel, req, name):
    import tensor_stream as ts
    dev = torch.device("cuda", 0)
    (w, h, py, puv), crop, dst, rt, fcc, planes, norm, n, aligned = req
    what = f"{name}: kernel {kernel} request {req}"
    y0, uv0 = E.frame(name, w, h, py, puv)
    host = [(y0, uv0), (E.complement(y0), E.complement(uv0))]  # frame 0: the class, frame 1: its complement
    if crop != (0, 0, 0, 0):
        for k, (y, uv) in enumerate(host):
            _poison_outside_the_crop(y, uv, crop, 0 if k == 0 else 255)
    on_dev = [(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev)) for y, uv in host]
    assert all(t.data_ptr() % 256 == 0 for pair in on_dev for t in pair)  # (what describe assumes for in4=)
    ys, uvs = [on_dev[k % 2][0] for k in range(n)], [on_dev[k % 2][1] for k in range(n)]
    fp = ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
    f32 = bool(norm) or fcc == 6
    nbytes = G.out_bytes(req)
    buf, slots, pat, starts = C._outputs(nbytes, n, 0 if aligned else (4 if f32 else 1), 17, 0xA5, dev)
    v.convert_batch(ys, uvs, fp, out=[s.view(torch.float32) if f32 else s for s in slots], width=w, height=h)
    torch.cuda.synchronize()
    if not knob_run():  # (replayed under A/B knobs the selections are the knobs')
        live = ts.vpp.debug_last_launch()
        assert live["kernel"] == kernel, f"the launch went to {live['kernel']}: {what}"
    g = C._guards_intact(buf, pat, starts, nbytes)
    assert g is None, f"{g}: {what}"
    for k in sorted({0, 1, n - 1}):
        y, uv = host[k % 2]
        ref = oracle.convert(y, uv, crop=crop, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=16, width=w)[0].view(np.uint8).ravel()
        got = slots[k].cpu().numpy()
        assert got.size == ref.size, f"frame {k}: {got.size} bytes, oracle {ref.size}: {what}"
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, f"frame {k} of {n}: {bad.size} of {got.size} bytes differ from the oracle, first at {bad[:4]}: {what}"


@pytest.mark.parametrize("name", E.CLASSES)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_convert_kernels(vpp, oracle, kernels, family, name):
    mine = kernels.get(family, [])
    if not mine:
        assert knob_run(), f"the grid reaches no {family} launch"  # (a knob may route a whole family elsewhere)
        return
    for kernel, req in mine:
        run_convert(vpp, oracle, kernel, req, name)
    torch.cuda.empty_cache()


def test_the_convert_leg_reaches_every_kernel_name_of_the_grid(kernels):
    """(host only, but it belongs with the leg above) one request per kernel name, every family of dispatch_grid.FAMILIES among them"""
    names = {n for fam in kernels.values() for n, _ in fam}
    assert names == {G.kernel_name(s) for s in G.signatures()}
    if not knob_run():
        assert set(kernels) == set(G.FAMILIES) and len(names) >= 67
