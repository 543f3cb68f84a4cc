"""No GPU: the host side of tsvpp_convert_rois_sized and its siblings (include/tsvpp.h) -- struct layout, every status rule and their precedence (through the
describe call, and through the convert call with a null context: the request is checked before the context is touched), tsvpp_rois_sized_bytes, the describe
line, the launch split, and the workgroup lookup: tsvpp_rois_sized_tile runs the kernel's own __host__ __device__ function (sized_tile, csrc/vpp_rois_sized.h),
and test_every_workgroup_has_exactly_one_tile walks every workgroup of seeded requests through it.  That test is where mutations of the lookup were tried (`<`
for `<=` in the count, tile0 of the NEXT box, column-major tiles, the shifted last column taken for element-wise launches): each one fails it.  Then the two
pure-Python helpers on hand-computed values."""
import ctypes
import os
import subprocess

import pytest

import rois_sized_util as U
from rois_sized_util import AREA, BGR24, BICUBIC, BILINEAR, ERROR, HSV, LIMIT, MERGED, NEAREST, NV12, OK, PLANAR, RGB24, UNSUPPORTED, UYVY, Y800, YUV444
from util import knob_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F1080 = (1920, 1080, 2048)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def spec_of(native, dtype=0, mean=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    return native.TensorSpec(dtype, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*scale))


def test_symbols_and_struct_layout(native):
    L = native.lib()
    for s in ("tsvpp_rois_sized_bytes", "tsvpp_convert_rois_sized", "tsvpp_describe_rois_sized", "tsvpp_convert_rois_sized_tensor", "tsvpp_describe_rois_sized_tensor",
              "tsvpp_rois_sized_tile"):
        assert s in native.SYMBOLS and getattr(L, s)
    assert ctypes.sizeof(native.RoiSized) == 28
    assert [f[0] for f in native.RoiSized._fields_] == ["frame", "left", "top", "right", "bottom", "dst_width", "dst_height"]
    assert native.TSVPP_MAX_ROIS_SIZED == LIMIT == 48
    assert "#define TSVPP_MAX_ROIS_SIZED 48" in open(os.path.join(ROOT, "include", "tsvpp.h")).read()


def test_the_header_compiles_as_c_and_the_struct_is_28_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tsvpp.h"\n_Static_assert(sizeof(tsvpp_roi_sized) == 28, "tsvpp_roi_sized");\nint main(void) { return TSVPP_MAX_ROIS_SIZED == 48 ? 0 : 1; }\n')
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(src)])
    subprocess.check_call([str(tmp_path / "t")])


GOOD = (0, 100, 50, 700, 550, 96, 32)

ERROR_CASES = {
    "null params": dict(null=("p",)),
    "null frames": dict(null=("frames",)),
    "null rois": dict(null=("rois",)),
    "n_rois zero": dict(n_rois=0),
    "n_rois negative": dict(n_rois=-1),
    "n_frames zero": dict(n_frames=0),
    "frame without size": dict(frames=[(0, 1080, 2048)]),
    "pitch below the width": dict(frames=[(1920, 1080, 1900)]),
    "frame index out of range": dict(rois=[(1, 0, 0, 64, 64, 32, 32)]),
    "negative frame index": dict(rois=[(-1, 0, 0, 64, 64, 32, 32)]),
    "empty box": dict(rois=[(0, 10, 10, 10, 74, 32, 32)]),
    "inverted box": dict(rois=[(0, 100, 10, 50, 74, 32, 32)]),
    "box outside its frame": dict(rois=[(0, 0, 0, 1922, 64, 32, 32)]),
    "negative origin": dict(rois=[(0, -2, 0, 62, 64, 32, 32)]),
    "dst_width of a box zero": dict(rois=[(0, 0, 0, 64, 64, 0, 32)]),
    "dst_height of a box negative": dict(rois=[(0, 0, 0, 64, 64, 32, -2)]),
    "p->dst_width set": dict(dst=(96, 0)),
    "p->dst_height set": dict(dst=(0, 32)),
    "p->dst_* set to the boxes' own size": dict(dst=(96, 32)),
    "crop set": dict(crop=(0, 0, 64, 64)),
}

UNSUPPORTED_CASES = {
    "odd box width": dict(rois=[(0, 0, 0, 63, 64, 32, 32)]),
    "odd box height": dict(rois=[(0, 0, 0, 64, 63, 32, 32)]),
    "odd dst_width of a box": dict(rois=[(0, 0, 0, 64, 64, 33, 32)]),
    "odd dst_height of a box": dict(rois=[(0, 0, 0, 64, 64, 32, 31)]),
    "odd frame width": dict(frames=[(1919, 1080, 2048)]),
    "odd frame height": dict(frames=[(1920, 1079, 2048)]),
    "AREA": dict(rt=AREA),
    "unknown resize type": dict(rt=7),
    "NV12 output": dict(fcc=NV12),
    "UYVY output": dict(fcc=UYVY),
    "YUV444 output": dict(fcc=YUV444),
    "HSV output": dict(fcc=HSV),
    "unknown planes": dict(planes=2),
    # (65538 - 1) * 65536 + 65536 = 2^32 + 2^17 bytes as seen from the box's origin
    "source span at the limit": dict(frames=[(65536, 65538, 65536)], rois=[(0, 0, 0, 65536, 65538, 32, 32)]),
    # 32768 x 32768 fp32 Y800 = 4 GiB exactly
    "output of 4 GiB": dict(fcc=Y800, norm=1, rois=[(0, 0, 0, 64, 64, 32768, 32768)]),
}


def request(native, frames=(F1080,), rois=(GOOD,), rt=BILINEAR, fcc=RGB24, planes=MERGED, norm=0, dst=(0, 0), crop=(0, 0, 0, 0), **kw):
    return U.statuses(native, U.params(native, rt, fcc, planes, norm, dst, crop), list(frames), list(rois), **kw)


def test_the_good_request_is_ok(native):
    d, c, text = request(native)
    assert d == OK and text.startswith("mode=bilinear out=u8_merged dst=var rois=1 frames=1 launches=1 kernel=vpp_rois_sized<")
    assert c == ERROR  # the request passed; a null context is the convert call's own error
    # just below the limits of the two UNSUPPORTED cases that have one
    assert request(native, frames=[(65536, 65536, 65536)], rois=[(0, 0, 0, 65536, 65534, 32, 32)])[0] == OK
    assert request(native, fcc=Y800, norm=1, rois=[(0, 0, 0, 64, 64, 32768, 32766)])[0] == OK


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_error_statuses(native, name):
    d, c, text = request(native, **ERROR_CASES[name])
    assert (d, c, text) == (ERROR, ERROR, ""), name


@pytest.mark.parametrize("name", sorted(UNSUPPORTED_CASES))
def test_unsupported_statuses(native, name):
    d, c, text = request(native, **UNSUPPORTED_CASES[name])
    assert (d, c, text) == (UNSUPPORTED, UNSUPPORTED, ""), name


def test_an_error_in_a_later_box_wins_over_an_unsupported_earlier_one(native):
    odd = (0, 0, 0, 63, 64, 32, 32)          # UNSUPPORTED alone
    outside = (0, 0, 0, 1922, 64, 32, 32)    # ERROR alone
    assert request(native, rois=[odd, GOOD, GOOD, GOOD])[0] == UNSUPPORTED
    assert request(native, rois=[odd, GOOD, GOOD, outside])[:2] == (ERROR, ERROR)
    assert request(native, rois=[odd, GOOD, GOOD, (0, 0, 0, 64, 64, 0, 32)])[:2] == (ERROR, ERROR)  # a box's dst <= 0 is an ERROR condition too
    assert request(native, rt=AREA, rois=[GOOD, GOOD, GOOD, outside])[:2] == (ERROR, ERROR)
    assert request(native, rt=AREA, dst=(96, 32))[:2] == (ERROR, ERROR)                            # non-zero p->dst_* before AREA


def test_area_is_unsupported_from_all_four_entry_points_and_describe_rois_answers_as_before(native):
    spec = spec_of(native)
    for norm, planes in ((0, MERGED), (1, PLANAR)):
        assert request(native, rt=AREA, norm=norm, planes=planes)[:2] == (UNSUPPORTED, UNSUPPORTED)
        assert request(native, rt=AREA, norm=norm, planes=planes, tensor=True, spec=spec)[:2] == (UNSUPPORTED, UNSUPPORTED)
    # the existing calls keep their answers: tsvpp_describe_rois refuses AREA, tsvpp_describe_rois_area takes it
    L = native.lib()
    fr, bx = U.nv12_records(native, [F1080]), (native.Roi * 1)(native.Roi(*GOOD[:5]))
    buf = ctypes.create_string_buffer(512)
    p = U.params(native, AREA, dst=(96, 32))
    assert L.tsvpp_describe_rois(ctypes.byref(p), 1, fr, 1, bx, 1, buf, len(buf)) == UNSUPPORTED
    assert L.tsvpp_describe_rois_area(ctypes.byref(p), 1, fr, 1, bx, 1, buf, len(buf)) == OK and buf.value.decode().startswith("mode=area ")


def test_the_tensor_forms_apply_the_spec_rules_behind_the_plan(native):
    ok = spec_of(native, 1, (0.5, 0.5, 0.5), (2.0, 2.0, 2.0))
    d, c, text = request(native, planes=PLANAR, norm=1, tensor=True, spec=ok)
    assert d == OK and c == ERROR and " out=f16_planar " in text and "kernel=vpp_rois_sized_tensor<M_BILINEAR,PLANAR,EL_HALF,vec," in text
    assert " out=bf16_y800 " in request(native, fcc=Y800, norm=1, tensor=True, spec=spec_of(native, 2))[2]
    assert request(native, planes=PLANAR, norm=1, tensor=True, spec=None)[:2] == (ERROR, ERROR)                                     # rule 2
    assert request(native, planes=PLANAR, norm=1, tensor=True, spec=spec_of(native, 0, scale=(1.0, 0.0, 1.0)))[:2] == (ERROR, ERROR)
    assert request(native, planes=PLANAR, norm=1, tensor=True, spec=spec_of(native, 5))[:2] == (UNSUPPORTED, UNSUPPORTED)           # rule 3
    assert request(native, planes=PLANAR, norm=0, tensor=True, spec=ok)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert request(native, planes=MERGED, norm=1, tensor=True, spec=ok)[:2] == (UNSUPPORTED, UNSUPPORTED)
    # rule 1 first: the plan's UNSUPPORTED wins over the spec's ERROR, the plan's ERROR over the spec's UNSUPPORTED
    assert request(native, planes=PLANAR, norm=1, tensor=True, spec=None, rois=[(0, 0, 0, 63, 64, 32, 32)])[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert request(native, planes=MERGED, norm=1, tensor=True, spec=ok, dst=(2, 2))[:2] == (ERROR, ERROR)


def test_rois_sized_bytes_against_out_bytes_and_tensor_bytes(native):
    L = native.lib()
    for fcc, planes, norm in U.FLAVOURS:
        for w, h in [(2, 2), (30, 2), (96, 32), (640, 48), (1920, 1080)]:
            p0, pd = U.params(native, BILINEAR, fcc, planes, norm), U.params(native, BILINEAR, fcc, planes, norm, dst=(w, h))
            want = L.tsvpp_out_bytes(ctypes.byref(pd), w, h)
            assert want == U.channels(fcc) * w * h * (4 if norm else 1)
            assert L.tsvpp_rois_sized_bytes(ctypes.byref(p0), None, w, h) == want
            for dt in (0, 1, 2):
                spec = spec_of(native, dt)
                assert L.tsvpp_rois_sized_bytes(ctypes.byref(p0), ctypes.byref(spec), w, h) == L.tsvpp_tensor_bytes(ctypes.byref(pd), ctypes.byref(spec))
    p0 = U.params(native, BILINEAR, RGB24, PLANAR, 1)
    f16 = spec_of(native, 1)
    assert L.tsvpp_rois_sized_bytes(ctypes.byref(p0), ctypes.byref(f16), 96, 32) == 3 * 96 * 32 * 2
    # 0 for what the entry points refuse
    for bad in (U.params(native, AREA), U.params(native, BILINEAR, NV12), U.params(native, BILINEAR, dst=(96, 32)), U.params(native, BILINEAR, crop=(0, 0, 2, 2)),
                U.params(native, 9)):
        assert L.tsvpp_rois_sized_bytes(ctypes.byref(bad), None, 96, 32) == 0
    good = U.params(native)
    for w, h in [(0, 32), (96, -2), (95, 32), (96, 31)]:
        assert L.tsvpp_rois_sized_bytes(ctypes.byref(good), None, w, h) == 0
    assert L.tsvpp_rois_sized_bytes(None, None, 96, 32) == 0
    y8 = U.params(native, BILINEAR, Y800, MERGED, 1)
    assert L.tsvpp_rois_sized_bytes(ctypes.byref(y8), None, 32768, 32768) == 0 and L.tsvpp_rois_sized_bytes(ctypes.byref(y8), None, 32768, 32766) == 4 * 32768 * 32766
    assert L.tsvpp_rois_sized_bytes(ctypes.byref(y8), ctypes.byref(f16), 32768, 32768) == 0  # the limit is stated on fp32


def test_describe_grid_is_the_sum_of_the_tile_counts(native):
    rois = [b + s for b, s in zip(U.BOXES, U.SIZES)]
    d = U.describe(native, U.params(native), U.FRAMES, rois, aligned=0)
    assert d["launches"] == 1 and d["vec"] == 0 and d["grid"] == sum(U.tiles(w, h) for w, h in U.SIZES) == 1 + 1 + 1 + 4 + 2 + 6 + 4 + 6 + 8 + 20 + 2 + 3
    assert d["dst"] == "var" and d["rois"] == 12 and d["frames"] == 2 and d["sizes"] == 12 and d["maxdst"] == "160x100" and d["limit"] == 48 and d["shape"] == "8x16"
    assert d["kernel"].startswith("vpp_rois_sized<M_BILINEAR,O_U8_MERGED,elem,")
    # aligned: the three narrow tails (2, 30 and 2 columns) leave for a launch of their own, the first launch is the other nine
    d = U.describe(native, U.params(native), U.FRAMES, rois, aligned=1)
    narrow = [s for s in U.SIZES if U.narrow_tail(s[0])]
    assert len(narrow) == 3
    assert d["launches"] == 2 and d["vec"] == 9 and d["grid"] == sum(U.tiles(w, h) for w, h in U.SIZES if not U.narrow_tail(w))
    assert d["kernel"].startswith("vpp_rois_sized<M_BILINEAR,O_U8_MERGED,vec,")
    assert d["sizes"] == 12  # (distinct sizes of the request, not of the launch)
    same = [b + (64, 32) for b in U.BOXES]
    assert U.describe(native, U.params(native), U.FRAMES, same)["sizes"] == 1


@pytest.mark.parametrize("n,launches", [(1, 1), (48, 1), (49, 2), (96, 2), (97, 3)])
def test_describe_launches_at_the_chunk_boundaries(native, n, launches):
    frames, rois = U.seeded_request(n, n=n, max_side=64)
    rois = [r[:5] + (4 * ((r[5] + 3) // 4), r[6]) for r in rois]  # widths 4 k: every box is vector-eligible when aligned
    for aligned in (1, 0):
        d = U.describe(native, U.params(native), frames, rois, aligned=aligned)
        assert d["launches"] == launches and d["vec"] == (n if aligned else 0) and d["rois"] == n
        assert d["grid"] == sum(U.tiles(r[5], r[6]) for r in rois[:LIMIT])


@pytest.mark.parametrize("n", [2, 12, 48, 49])
def test_one_narrow_box_among_aligned_others_is_a_launch_of_its_own(native, n):
    frames, rois = U.seeded_request(300 + n, n=n, max_side=64)
    rois = [r[:5] + (4 * ((r[5] + 3) // 4), r[6]) for r in rois]
    k = n // 2
    rois[k] = rois[k][:5] + (30, rois[k][6])
    d = U.describe(native, U.params(native), frames, rois, aligned=1)
    assert d["vec"] == n - 1 and d["launches"] == (n - 1 + LIMIT - 1) // LIMIT + 1
    first = [r for i, r in enumerate(rois) if i != k][:LIMIT]
    assert d["grid"] == sum(U.tiles(r[5], r[6]) for r in first) and ",vec," in d["kernel"]
    assert U.describe(native, U.params(native), frames, rois, aligned=0)["launches"] == (n + LIMIT - 1) // LIMIT


@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
@pytest.mark.parametrize("fcc,planes,norm", [(RGB24, MERGED, 0), (BGR24, PLANAR, 1), (RGB24, MERGED, 1), (Y800, MERGED, 0)])
@pytest.mark.parametrize("aligned", [1, 0])
def test_boxes_that_share_one_size_report_describe_rois_lds_and_staged(native, rt, fcc, planes, norm, aligned):
    """the planning is tsvpp_describe_rois's arithmetic with the box's own output: boxes that all go to 224 x 224 -- some staged, the 1920 x 1080 box gathering --
    report its lds=, staged=, grid= and nt="""
    W, H = 1920, 1080
    boxes = [(100, 50, 700, 550), (300, 200, 364, 248), (400, 300, 624, 524), (101, 40, 401, 300), (200, 33, 480, 333), (0, 0, 256, 256), (W - 310, 400, W, 700),
             (0, 100, W, 324), (800, 0, 1000, H), (W - 2, H - 2, W, H), (1000, 500, 1800, 600), (50, 300, 130, 1000), (0, 0, W, H)]
    L = native.lib()
    buf = ctypes.create_string_buffer(512)
    fr = U.nv12_records(native, [F1080])
    bx = (native.Roi * len(boxes))(*[native.Roi(0, *b) for b in boxes])
    p = U.params(native, rt, fcc, planes, norm, dst=(224, 224))
    assert L.tsvpp_describe_rois(ctypes.byref(p), 1, fr, len(boxes), bx, aligned, buf, len(buf)) == OK
    old = dict(item.split("=", 1) for item in buf.value.decode().split(" "))
    new = U.describe(native, U.params(native, rt, fcc, planes, norm), [F1080], [(0,) + b + (224, 224) for b in boxes], aligned=aligned)
    if not knob_run():
        assert 0 < int(old["staged"]) < len(boxes)
    assert (new["lds"], new["staged"], new["grid"], new["nt"]) == (int(old["lds"]), int(old["staged"]), int(old["grid"]), int(old["nt"]))
    assert new["kernel"] == old["kernel"].replace("vpp_rois<", "vpp_rois_sized<")


def expected_tile(w, txi, tyi, vec):
    """roi_tile_col0 / tyi * 32 for a box `w` columns wide, with its own shifted last column (vector launches only)"""
    last_col0 = w - U.TILE if (vec and w % 4 != 0 and w >= U.TILE) else 0
    j = txi * U.TILE
    return (last_col0 if (last_col0 > 0 and j + U.TILE > w) else j), tyi * U.TILE


@pytest.mark.parametrize("seed", range(20))
def test_every_workgroup_has_exactly_one_tile(native, seed):
    """Exact cover: over wg = 0 .. grid - 1 of the first launch every (box, tile column, tile row) of every box of that launch appears exactly once, boxes ascend
    with wg, tiles are row-major inside a box, and the tile's first column / row are the box's own; wg = grid is TSVPP_ERROR"""
    L = native.lib()
    frames, rois = U.seeded_request(9000 + seed)
    assert 1 <= len(rois) <= LIMIT
    p = U.params(native)
    fr, bx = U.nv12_records(native, frames), U.roi_records(native, rois)
    out5 = (ctypes.c_int32 * 5)()
    for aligned in (0, 1):
        # the first launch: every box (element-wise), or the vector-eligible ones -- all of them narrow tails: the element-wise launch is the first
        members = [i for i, r in enumerate(rois) if not (aligned and U.narrow_tail(r[5]))]
        vec = bool(aligned) and bool(members)
        members = members or list(range(len(rois)))
        d = U.describe(native, p, frames, rois, aligned=aligned)
        grid = sum(U.tiles(rois[i][5], rois[i][6]) for i in members)
        assert d["grid"] == grid and ("vec" in d["kernel"].split(",")) == vec
        walked = []
        for wg in range(grid):
            assert L.tsvpp_rois_sized_tile(ctypes.byref(p), len(frames), fr, len(rois), bx, aligned, wg, out5) == OK, wg
            walked.append(tuple(out5))
        want = []
        for i in members:
            w, h = rois[i][5], rois[i][6]
            for tyi in range((h + U.TILE - 1) // U.TILE):
                for txi in range((w + U.TILE - 1) // U.TILE):
                    want.append((i, txi, tyi) + expected_tile(w, txi, tyi, vec))
        assert walked == want  # every tile once, boxes ascending, row-major inside a box, the box's own first column / row
        assert len(set(w[:3] for w in walked)) == grid
        for wg in (grid, grid + 1, 0xFFFFFFFF):
            assert L.tsvpp_rois_sized_tile(ctypes.byref(p), len(frames), fr, len(rois), bx, aligned, wg, out5) == ERROR
    assert L.tsvpp_rois_sized_tile(ctypes.byref(p), len(frames), fr, len(rois), bx, 1, 0, None) == ERROR
    bad = U.params(native, AREA)
    assert L.tsvpp_rois_sized_tile(ctypes.byref(bad), len(frames), fr, len(rois), bx, 1, 0, out5) == UNSUPPORTED


def test_the_seeded_requests_reach_what_the_lookup_can_get_wrong():
    """the 20 requests hold 1-box and 48-box launches, single-tile boxes, shifted last columns, narrow tails and more than 2000 workgroups in all"""
    reqs = [U.seeded_request(9000 + s)[1] for s in range(20)]
    ns = [len(r) for r in reqs]
    assert min(ns) <= 4 and max(ns) >= 44
    flat = [r for rq in reqs for r in rq]
    assert any(U.tiles(r[5], r[6]) == 1 for r in flat) and any(r[5] % 4 and r[5] >= 32 for r in flat) and any(U.narrow_tail(r[5]) for r in flat)
    assert max(r[5] for r in flat) >= 190 and max(r[6] for r in flat) >= 190 and min(r[5] for r in flat) == 2
    assert sum(U.tiles(r[5], r[6]) for r in flat) > 2000


def test_sizes_for_height():
    import tensor_stream as ts
    # w = m * max(1, (2 * bw * height + bh * m) // (2 * bh * m))
    assert ts.sizes_for_height([(0, 0, 200, 40)], 32) == [(160, 32)]                       # 12880 // 160 = 80
    assert ts.sizes_for_height([(3, 10, 20, 40, 60)], 48) == [(36, 48)]                    # bw 30, bh 40: (2880 + 80) // 160 = 18
    assert ts.sizes_for_height([(0, 0, 100, 30)], 32) == [(106, 32)]                       # 106.67: (6400 + 60) // 120 = 53
    assert ts.sizes_for_height([(0, 0, 100, 30)], 32, multiple=8) == [(104, 32)]           # (6400 + 240) // 480 = 13
    assert ts.sizes_for_height([(0, 0, 36, 32)], 32, multiple=8) == [(40, 32)]             # 4.5 multiples: the tie goes up, (2304 + 256) // 512 = 5
    assert ts.sizes_for_height([(0, 0, 2, 64)], 32) == [(2, 32)]                           # at least one multiple
    assert ts.sizes_for_height([(0, 0, 640, 32), (0, 0, 64, 32)], 32, max_width=321, multiple=4) == [(320, 32), (64, 32)]
    with pytest.raises(ValueError):
        ts.sizes_for_height([(0, 0, 64, 32)], 32, multiple=3)
    with pytest.raises(ValueError):
        ts.sizes_for_height([(0, 0, 0, 32)], 32)


def test_pyramid_sizes():
    import tensor_stream as ts
    assert ts.pyramid_sizes(1920, 1080, 5) == [(1920, 1080), (960, 540), (480, 270), (240, 134), (120, 66)]  # 135 & ~1 = 134, 67 & ~1 = 66
    assert ts.pyramid_sizes(1921, 1081, 2) == [(1920, 1080), (960, 540)]
    assert ts.pyramid_sizes(6, 20, 4) == [(6, 20), (2, 10), (2, 4), (2, 2)]                                     # 6 >> 1 = 3 -> 2; 6 >> 2 = 1 -> 0 -> 2
    assert ts.pyramid_sizes(64, 64, 0) == []


def test_the_python_facade_checks_its_lists_before_any_device():
    import tensor_stream as ts
    from tensor_stream import vpp as V
    fp = ts.FrameParameters(resize_type=BILINEAR)
    with pytest.raises(ValueError):
        V._normalize_sizes([(32, 32)], 2)
    with pytest.raises(ValueError):
        V._normalize_sizes([(32, 32, 1)], 1)
    d = ts.describe_rois_sized(fp, [(320, 180, 328), (192, 108, 200)], U.BOXES, U.SIZES)
    assert d["dst"] == "var" and d["rois"] == 12 and d["vec"] == 9 and d["launches"] == 2
    d = ts.describe_rois_sized(ts.FrameParameters(resize_type=BICUBIC, pixel_format=BGR24, planes_pos=PLANAR, normalization=True), (320, 180), [(0, 0, 64, 64)],
                               [(96, 32)], dtype=__import__("torch").float16, mean=0.5, std=0.25)
    assert d["out"] == "f16_planar" and d["kernel"].startswith("vpp_rois_sized_tensor<M_BICUBIC,PLANAR,EL_HALF,vec,")
    with pytest.raises(RuntimeError, match="-3"):
        ts.describe_rois_sized(ts.FrameParameters(width=96, height=32), (320, 180), [(0, 0, 64, 64)], [(96, 32)])
    with pytest.raises(RuntimeError, match="-2"):
        ts.describe_rois_sized(ts.FrameParameters(resize_type=AREA), (320, 180), [(0, 0, 64, 64)], [(96, 32)])
