"""No GPU: the content classes of tests/edge_content.py do what they are there for, shown from the reference alone -- the oracle lands on the truncation boundary
for a large share of the samples, so tests/test_gpu_edge_content.py probes the kernels' weights and roundings and not only their addressing -- and the hooks that
put the classes into the fuzz generators leave the generators' own draws as they were.

Measured with the oracle (profiles/edge_content.txt holds the same figures):
    (a) chunk 0, every frame flat_255_128_128, share of Y800 luma samples that are not 255:
        rois BILINEAR 8.88 % of 113452, letterbox BILINEAR 8.97 % of 66684 (inside the rectangles), rois_area 6.59 % of 471520
    (b) share of 254 in the luma of a flat 255 frame, per named AREA case: 17.7 % .. 47.4 % (the list is printed by the test)
    (c) chunk 0, every frame `checker`, BICUBIC calls of rois and letterbox: 4.24 % of the 111576 luma samples are 0 and 5.01 % are 255 -- the floors are half of each"""
import hashlib

import numpy as np
import pytest

import edge_content as E
import letterbox_area_fuzz as ZA
import rois_sized_fuzz as ZS
import tile_fuzz as F
from letterbox_util import AREA, BICUBIC, BILINEAR, MERGED, Y800, default_rect

FLAT = "flat_255_128_128"


def luma_of_chunk0(oracle, family, content, rts):
    """the oracle's Y800 luma of every output of the family's chunk-0 calls whose resize type is in `rts`, every frame holding `content`: one flat uint8 array
    (letterbox: the rectangles only -- the pad is not sampled)"""
    out = []
    for call in F.cases(family, 0):
        if call["rt"] not in rts:
            continue
        call = E.with_content(call, content)
        host = F.host_frames(call)
        for item in call["items"]:
            fr = call["frames"][item[0]]
            _, _, y, uv = host[item[0]]
            if family == "letterbox":
                rect = item[1] if item[1] is not None else default_rect(fr["w"], fr["h"], *call["dst"])
                ys, uvs, dst = y[:fr["h"], :fr["w"]], uv[:fr["h"] // 2, :fr["w"]], rect[2:]
            else:
                l, t, r, b = item[1:]
                ys, uvs, dst = y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r], call["dst"]
            out.append(oracle.convert(ys, uvs, dst=dst, resize_type=call["rt"], fourcc=Y800, planes=MERGED, normalization=False)[0].view(np.uint8).ravel())
    return np.concatenate(out)


@pytest.mark.parametrize("family,rts", [("rois", (BILINEAR,)), ("letterbox", (BILINEAR,)), ("rois_area", (AREA,))])
def test_a_flat_255_frame_puts_the_reference_on_the_boundary(oracle, family, rts):
    """(a) at least 2 % of the samples are 254 (measured: 8.88 %, 8.97 %, 6.59 %): a flat frame is not the trivial case"""
    luma = luma_of_chunk0(oracle, family, FLAT, rts)
    share = float(np.mean(luma != 255))
    print(f"(a) {family}: {100 * share:.2f} % of {luma.size} luma samples differ from 255")
    assert set(np.unique(luma).tolist()) <= {254, 255}
    assert share >= 0.02


def test_every_named_area_case_probes(oracle):
    """(b) the share of c - 1 at c = 255 is at least 5 % for every named case: a case that measures 0 is no probe and has no place in the list"""
    for sw, sh, dw, dh in E.named_area_geometries():
        y, uv = E.frame(FLAT, sw, sh, sw, sw)
        luma = oracle.convert(y, uv, dst=(dw, dh), resize_type=AREA, fourcc=Y800, planes=MERGED, normalization=False)[0].view(np.uint8).ravel()
        share = float(np.mean(luma == 254))
        print(f"(b) {sw} x {sh} -> {dw} x {dh}: {100 * share:.1f} % of {luma.size} samples are 254")
        assert set(np.unique(luma).tolist()) <= {254, 255}
        assert share >= 0.05, (sw, sh, dw, dh, share)


# (c) measured shares of the luma samples that are 0 / 255; the test holds half of each
CHECKER_ZERO, CHECKER_FULL = 0.0424, 0.0501


def test_checker_clamps_bicubic_in_both_directions(oracle):
    luma = np.concatenate([luma_of_chunk0(oracle, family, "checker", (BICUBIC,)) for family in ("rois", "letterbox")])
    zero, full = float(np.mean(luma == 0)), float(np.mean(luma == 255))
    print(f"(c) checker through BICUBIC: {100 * zero:.2f} % of {luma.size} luma samples are 0, {100 * full:.2f} % are 255")
    assert zero >= CHECKER_ZERO / 2 and full >= CHECKER_FULL / 2


def _digest(buffers):
    d = hashlib.sha256()
    for b in buffers:
        d.update(np.ascontiguousarray(b).tobytes())
    return d.hexdigest()[:16]


# (d) sha256 (first 16 digits) over the flat luma and chroma buffers of every frame of the generators' own draws, taken before the hooks went in
DEFAULT_DRAWS = {"rois": "0f8452fe5b919e3f", "rois_area": "3d642d2c82658f84", "letterbox": "2ccb0b438aa0c205", "warp": "f9402bde92b2b2bb", "persp": "878e816f12e270c1",
                 "rois_sized": "c2a1eb017f7f8aee", "remap": "ff504bb687b704c3", "mesh": "3c6be08e0b2a3dc7", "letterbox_area": "419ab05dc298f1cd"}


def _default_draws(family):
    if family in F.FAMILIES:
        return _digest(b for c in F.cases(family, 0) for fr in F.host_frames(c) for b in fr[:2])
    if family == "rois_sized":
        return _digest(b for c in ZS.cases(0) for fr in F.host_frames(c) for b in fr[:2])
    if family == "letterbox_area":
        return _digest(b for c in ZA.cases() for fr in ZA.host_frames(c) for b in fr)
    pytest.importorskip("torch")  # (the two modules hold GPU tests beside their generators)
    import test_gpu_mesh_fuzz
    import test_gpu_remap_fuzz
    mod = {"remap": test_gpu_remap_fuzz, "mesh": test_gpu_mesh_fuzz}[family]
    return _digest(b for c in mod.CALLS_DRAWN for fr in c["frames"] for b in mod.planes(fr)[:2])


@pytest.mark.parametrize("family", sorted(DEFAULT_DRAWS))
def test_the_hooks_leave_the_default_draws_unchanged(family):
    """(d) chunk 0 of the tile families and of rois_sized, every call of remap, mesh and letterbox_area"""
    assert _default_draws(family) == DEFAULT_DRAWS[family]


@pytest.mark.parametrize("name", E.CLASSES)
def test_classes_and_their_padding(name):
    """(e) at odd pitches and offsets: the picture is the stated one, and every byte outside it -- pitch padding, lead-in, the 16 trailing bytes -- holds the stated
    value, which no pixel next to it has"""
    lv = E.flat_levels(name)
    for w, h, pitch_y, pitch_uv, off_y, off_uv in ((2, 2, 2, 2, 0, 0), (6, 4, 7, 9, 1, 15), (34, 18, 37, 64, 13, 2), (320, 180, 321, 350, 7, 5)):
        fr = dict(w=w, h=h, pitch_y=pitch_y, pitch_uv=pitch_uv, off_y=off_y, off_uv=off_uv)
        flat_y, flat_uv, y, uv = E.planes(name, fr)
        assert flat_y.size == off_y + h * pitch_y + 16 and flat_uv.size == off_uv + (h // 2) * pitch_uv + 16
        assert np.shares_memory(flat_y, y) and np.shares_memory(flat_uv, uv) and y.shape == (h, pitch_y) and uv.shape == (h // 2, pitch_uv)
        y2, uv2 = E.frame(name, w, h, pitch_y, pitch_uv)
        assert np.array_equal(y, y2) and np.array_equal(uv, uv2) and np.array_equal(E.make(name, h, w, pitch_y, False), y)
        r, x = np.mgrid[0:h, 0:w]
        cr, cx = np.mgrid[0:h // 2, 0:w // 2]
        if lv:
            want_y, want_u, want_v = np.full((h, w), lv[0]), np.full((h // 2, w // 2), lv[1]), np.full((h // 2, w // 2), lv[2])
        elif name == "checker":
            want_y, want_u = 255 * ((r + x) & 1), 255 * ((cr + cx) & 1)
            want_v = 255 - want_u
        elif name == "edge_v":
            want_y, want_u = 255 * (x >= ((w // 2) | 1)), 255 * (cx >= ((w // 4) | 1))
            want_v = want_u
        elif name == "edge_h":
            want_y, want_u = 255 * (r >= ((h // 2) | 1)), 255 * (cr >= ((h // 4) | 1))
            want_v = want_u
        else:
            want_y, want_u = (x + 3 * r) & 255, (2 * cx + cr) & 255
            want_v = 255 - want_u
        assert np.array_equal(y[:, :w], want_y) and np.array_equal(uv[:, 0:w:2], want_u) and np.array_equal(uv[:, 1:w:2], want_v)
        # everything else
        mask_y, mask_uv = np.ones(flat_y.size, bool), np.ones(flat_uv.size, bool)
        for k in range(h):
            mask_y[off_y + k * pitch_y:off_y + k * pitch_y + w] = False
        for k in range(h // 2):
            mask_uv[off_uv + k * pitch_uv:off_uv + k * pitch_uv + w] = False
        assert mask_y.sum() == flat_y.size - w * h and mask_uv.sum() == flat_uv.size - w * (h // 2)
        if lv:
            assert (flat_y[mask_y] == 255 - lv[0]).all()
            k = np.flatnonzero(mask_uv) - off_uv  # the byte's index in the plane: even bytes are U's, odd ones V's
            assert np.array_equal(flat_uv[mask_uv], np.where(k & 1, 255 - lv[2], 255 - lv[1]))
            assert 255 - lv[0] != lv[0] and 255 - lv[1] != lv[1] and 255 - lv[2] != lv[2]
        else:
            assert (flat_y[mask_y] == 0x5A).all() and (flat_uv[mask_uv] == 0x5A).all()
    c = E.complement(y)
    assert c.dtype == np.uint8 and np.array_equal(c.astype(int) + y, np.full(y.shape, 255))


def test_with_content_marks_every_frame_and_the_call():
    call = F.cases("rois", 0)[0]
    marked = E.with_content(call, "ramp")
    assert "content" not in call and all("content" not in fr for fr in call["frames"])
    assert marked["content"] == "ramp" and all(fr["content"] == "ramp" for fr in marked["frames"]) and marked["items"] == call["items"]
    case = E.with_content(ZA.cases()[0], "checker")
    assert case["content"] == "checker" and case["frames"] == ZA.cases()[0]["frames"]
    y, uv = ZA.host_frames(case)[0]
    w, h, p = case["frames"][0]
    assert np.array_equal(y, E.make("checker", h, w, p, False)) and np.array_equal(uv, E.make("checker", h // 2, w, p, True))
