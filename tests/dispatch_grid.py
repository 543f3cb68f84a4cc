"""The request grid of the dispatcher coverage tests (tests/test_dispatch_cover_cpu.py, tests/test_gpu_dispatch_cover.py): a few hundred thousand requests
whose tsvpp_describe answers (the dry run of launch_fused) are grouped by SIGNATURE -- everything describe decides about a launch except its size
(src, dst, grid, tiles, frames, lds), plus whether the outputs are 16-byte aligned.  Host logic only: no GPU, no oracle.

Under A/B knob runs (util.knob_run()) the signatures are whatever describe answers with those knobs: the grid is the same."""
import ctypes
import glob
import os
import re
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# describe's keys that depend on the request's size rather than on the selection (frames: the launch's batch; lds: the LDS bytes of the chosen tile)
SIZE_KEYS = ("src", "dst", "grid", "tiles", "frames", "lds")

# (width, height, pitch_y, pitch_uv)
SOURCES = [
    (1920, 1080, 2048, 2048), (1920, 1080, 1922, 1922), (1926, 1080, 1926, 1926), (1280, 720, 1280, 1280), (3840, 2160, 3840, 3840),
    (1080, 608, 1088, 1088), (1366, 768, 1376, 1376), (960, 540, 960, 960), (640, 360, 640, 640), (320, 240, 320, 320),
    # chroma pitch other than the luma pitch
    (1920, 1080, 1920, 2048), (1280, 720, 1296, 1280), (640, 360, 656, 704),
]
RATIO_SOURCES = [SOURCES[0], SOURCES[1], SOURCES[4], SOURCES[5], SOURCES[8], SOURCES[12]]  # (the integer ratio pairs: one source per pitch class and size class)
NFRAMES = (1, 2, 8, 64, 128)
RT = (0, 1, 2, 3)  # NEAREST, BILINEAR, BICUBIC, AREA
# (fourcc, planes, normalization): the 7 FourCCs x planar / merged x uint8 / fp32 (HSV is fp32 whatever `normalization` says)
FLAVOURS = tuple((fcc, planes, norm) for fcc in range(7) for planes in (0, 1) for norm in (False, True) if not (fcc == 6 and not norm))
# the flavours that steer the selection most (element size x layout): the dimensions that multiply the grid (frames, alignment) take these only
CORE_FLAVOURS = ((2, 0, True), (1, 1, False), (1, 0, False), (1, 1, True), (3, 0, False), (0, 0, True), (6, 1, True), (4, 0, False), (5, 0, False))
MAX_DEVICE_BYTES = 1 << 30  # inputs + outputs of one batch: the GPU test allocates them (twice the outputs, plus guards)

# A/B-knob independent output sizes: the BASELINE configurations, the network input sizes, 4 k + 2 widths, multiples of 64 / 256 and widths that are not
FIXED_DST = [(1280, 720), (640, 360), (256, 256), (224, 224), (300, 300), (416, 416), (640, 640), (1282, 720), (1366, 768), (854, 480), (1024, 576),
             (768, 432), (1536, 864), (1344, 756), (1360, 768), (1376, 774), (1368, 770), (800, 450), (1918, 1080), (960, 540), (1440, 810),
             (608, 342), (2560, 1440), (1920, 1080), (320, 180), (480, 360), (0, 0)]


def _even(x):
    return max(2, int(x) // 2 * 2)


def _crops(w, h):
    """none, an odd left origin, flush to the right / bottom edge, a quarter of the frame"""
    return [(0, 0, 0, 0), (1, 2, 1 + _even(w * 3 // 4), 2 + _even(h * 3 // 4)), (w - _even(w * 5 // 8), h - _even(h * 5 // 8), w, h),
            (_even(w // 4), _even(h // 4), _even(w // 4) + _even(w // 2), _even(h // 4) + _even(h // 2))]


def _geometries():
    """(source, crop, dst) triples: every source with the fixed sizes, the up-scales and the ratio families; crops on a subset"""
    out = []
    for src in SOURCES:
        w, h = src[0], src[1]
        dsts = list(FIXED_DST)
        dsts += [(_even(w * 1.5), _even(h * 1.5)), (2 * w, 2 * h), (3 * w, 3 * h)]  # up-scales
        dsts += [(_even(w / r), _even(h / r)) for r in (2.25, 2.4, 2.5, 2.6, 2.7)]  # non-integer AREA ratios
        dsts += [(_even(w / rx), _even(h / ry)) for rx, ry in ((2, 2), (2.5, 2.5), (3, 2.25), (2, 3.5), (4, 4), (1.25, 1.25), (1.5, 2))]  # BICUBIC around 6.5
        dsts += [(_even(w / rx), _even(h / ry)) for rx, ry in ((1.5, 2.4), (2.4, 1.5), (28, 30))]  # AREA: float weights, 2 x 3 taps; 28+ taps a row
        for dst in dsts:
            out.append((src, (0, 0, 0, 0), dst))
        for crop in _crops(w, h)[1:]:
            cw, ch = crop[2] - crop[0], crop[3] - crop[1]
            for dst in [(0, 0), (_even(cw / 2), _even(ch / 2)), (_even(cw / 1.5), _even(ch / 1.5)), (_even(cw / 3.3), _even(ch / 2.7)), (2 * cw, 2 * ch), (300, 300), (854, 480)]:
                out.append((src, crop, dst))
        # every integer ratio pair (a, b), a, b in 1..8, exact: the source is cropped to (a * dw) x (b * dh) -- the AREA box / stream / cols instances are keyed on these
        for a in (range(1, 9) if src in RATIO_SOURCES else ()):
            for b in range(1, 9):
                dw, dh = _even(w / a), _even(h / b)
                cw, ch = a * dw, b * dh
                crop = (0, 0, cw, ch) if (cw < w and ch < h) else (0, 0, 0, 0)
                if crop == (0, 0, 0, 0) and (cw, ch) != (w, h):
                    continue  # (a crop must be strictly smaller on both axes)
                out.append((src, crop, (dw, dh)))
    return out


class _Describer:
    def __init__(self):
        import tensor_stream  # noqa: F401  (puts the package's sources on the path the library is found by)
        from tensor_stream import _native as N
        self.N = N
        self.L = N.lib()
        self.p = N.Params()
        self.buf = ctypes.create_string_buffer(512)

    def __call__(self, req):
        src, crop, dst, rt, fcc, planes, norm, n, aligned = req
        p = self.p
        p.crop_left, p.crop_top, p.crop_right, p.crop_bottom = crop
        p.dst_width, p.dst_height = dst
        p.resize_type, p.fourcc, p.planes, p.normalization = rt, fcc, planes, 1 if norm else 0
        sts = self.L.tsvpp_describe(ctypes.byref(p), src[0], src[1], src[2], src[3], n, aligned, self.buf, len(self.buf))
        if sts != 0:
            return None
        out = {}
        for item in self.buf.value.decode().split(" "):
            k, _, v = item.partition("=")
            out[k] = v
        return out


def signature_of(answer, aligned):
    """describe's answer (a dict of strings or ints) minus the size keys, plus the output alignment, as one hashable string"""
    return " ".join(f"{k}={answer[k]}" for k in sorted(answer) if k not in SIZE_KEYS) + f" aligned={int(aligned)}"


def out_bytes(req):
    """bytes of one output frame (tsvpp_out_bytes)"""
    from tensor_stream import _native as N
    src, crop, dst, rt, fcc, planes, norm, n, aligned = req
    p = N.Params(*crop, *dst, rt, fcc, planes, 1 if norm else 0)
    return int(N.lib().tsvpp_out_bytes(ctypes.byref(p), src[0], src[1]))


def oracle_bytes(req):
    """what the oracle reads and writes for one frame: the logical source plus the output"""
    src, crop, dst, rt, fcc, planes, norm, n, aligned = req
    cw, ch = (crop[2] - crop[0], crop[3] - crop[1]) if crop != (0, 0, 0, 0) else (src[0], src[1])
    return cw * ch * 3 // 2 + out_bytes(req)


def _requests():
    for src, crop, dst in _geometries():
        in_bytes = src[1] * max(src[2], src[3]) * 3 // 2
        for rt in RT:
            if dst == (0, 0) and rt != 0:
                continue  # no resize: the resize type plays no part
            for fl in FLAVOURS:
                yield (src, crop, dst, rt, fl[0], fl[1], fl[2], 1, 1), in_bytes
                if fl in CORE_FLAVOURS:
                    yield (src, crop, dst, rt, fl[0], fl[1], fl[2], 1, 0), in_bytes
                    for n in NFRAMES[1:]:
                        yield (src, crop, dst, rt, fl[0], fl[1], fl[2], n, 1), in_bytes


# Every kernel family the grid reaches, as describe names them (the kernel name up to its template arguments; "(none)": a crop + format conversion that is
# the second pass alone).  tests/test_gpu_dispatch_cover.py runs each family; tests/test_dispatch_cover_cpu.py checks that this list is what the grid reaches.
FAMILIES = ("(none)", "vpp_area_box_kernel", "vpp_area_cols_kernel", "vpp_area_direct_float_kernel", "vpp_area_direct_kernel", "vpp_area_dyadic_kernel",
            "vpp_area_stream_kernel", "vpp_areaf_kernel", "vpp_bicubic_cols_kernel", "vpp_bicubic_int_kernel", "vpp_bicubic_r32_kernel", "vpp_bilinear_kernel",
            "vpp_bilinear_r32_kernel", "vpp_bilinear_rows_kernel", "vpp_bilinear_up2_kernel", "vpp_color_kernel", "vpp_copy16_kernel", "vpp_fused_gather_kernel",
            "vpp_point_kernel", "vpp_point_rn_kernel", "vpp_rep2_kernel")

_CACHE = {}


def signatures():
    """{signature: [requests]}; a request is (src (w, h, pitch_y, pitch_uv), crop, dst, resize type, fourcc, planes, normalization, n_frames, aligned_outputs)"""
    if "sigs" in _CACHE:
        return _CACHE["sigs"]
    t0 = time.perf_counter()
    desc = _Describer()
    sigs = {}
    obytes = {}
    for req, in_bytes in _requests():
        key = req[:7]
        if key not in obytes:
            obytes[key] = out_bytes(req[:7] + (1, 1))
        if req[7] * (in_bytes + 2 * obytes[key]) > MAX_DEVICE_BYTES:
            continue  # (the GPU test allocates the batch: its device footprint stays bounded)
        a = desc(req)
        if a is None:
            continue  # refused (too large an output, odd sizes): not a launch
        sigs.setdefault(signature_of(a, req[8]), []).append(req)
    _CACHE["sigs"] = sigs
    _CACHE["seconds"] = time.perf_counter() - t0  # (tests/test_dispatch_cover_cpu.py bounds it)
    return sigs


def family(sig):
    """the kernel family of a signature: the kernel name up to its template arguments"""
    k = re.search(r"\bkernel=(\S+)", sig).group(1)
    return k.split("<")[0]


def kernel_name(sig):
    return re.search(r"\bkernel=(\S+)", sig).group(1)


def representative(sig):
    """the cheapest request of a signature, deterministically: fewest oracle bytes, then fewest frames, then the request's own order"""
    reqs = signatures()[sig]
    return min(reqs, key=lambda r: (oracle_bytes(r), r[7], repr(r)))


# ---- launches of more than TSVPP_MAX_BATCH frames out of a frame table (tests/test_gpu_dispatch_cover.py: test_table_launches_past_128_frames...) -------------
MAX_BATCH = 128          # include/tsvpp.h: TSVPP_MAX_BATCH (tests/test_dispatch_cover_cpu.py compares both with the header)
MAX_TABLE_LAUNCH = 1024  # include/tsvpp.h: TSVPP_MAX_TABLE_LAUNCH
TABLE_POOL = 7           # distinct source frames behind a big table: coprime to the 8 XCDs and to 128, so a wrapped or permuted frame index reads another frame
TABLE_PER_FAMILY = 4
TABLE_N_WANTED = MAX_TABLE_LAUNCH + 1  # two launch groups: 1024 + 1
TABLE_N_MIN = MAX_BATCH + 3            # the least that is still a launch the batch path cannot make


def out_kind(sig):
    return re.search(r"\bout=(\S+)", sig).group(1)


def pool_bytes(req):
    """device bytes of TABLE_POOL source frames, each plane in its own 256-byte aligned slot (test_gpu_dispatch_cover._fill_inputs)"""
    w, h, py, puv = req[0]
    return TABLE_POOL * ((h * py + 255) // 256 * 256 + ((h // 2) * puv + 255) // 256 * 256)


def table_launch_cap(dst_w, dst_h):
    """frames per launch out of a table for a single-pass request (tsvpp_api.cpp: convert_impl): TSVPP_MAX_TABLE_LAUNCH, less where the grid of the smallest
    tile (64 x 4 output pixels per workgroup of 256) would outgrow 2^31 threads, and never less than TSVPP_MAX_BATCH"""
    wg = ((dst_w + 63) // 64) * ((dst_h + 3) // 4)
    cap = min(((1 << 31) // 256) // max(wg, 1), MAX_TABLE_LAUNCH)
    return cap if cap > MAX_BATCH else MAX_BATCH


def table_candidates():
    """{family: [(signature, n_big, launch_cap)]}: up to TABLE_PER_FAMILY signatures per family of FAMILIES (all but "(none)") whose representative is converted out
    of a table of n_big entries.  Deterministic host logic.  A signature qualifies if
      * it is a single pass (no pass2=: the two-pass formats go through the table's host mirror in kernarg launches of <= 128 frames, which the table leg of
        every signature already runs -- they cannot make the launch this is about);
      * n_big outputs + TABLE_POOL source frames fit MAX_DEVICE_BYTES, n_big = TABLE_N_WANTED if that fits, else the largest count that does, >= TABLE_N_MIN;
      * one launch takes TABLE_N_MIN frames (table_launch_cap), and describe still answers with the family at the 128 frames it clamps to (the selection
        reads the frame count; the launch itself is checked on the GPU).
    Distinct out= kinds first, the fewest output bytes first among them; a family with fewer kinds than TABLE_PER_FAMILY fills up with its next smallest signatures."""
    if "table" in _CACHE:
        return _CACHE["table"]
    desc = _Describer()
    by_family = {}
    for sig in sorted(signatures()):
        fam = family(sig)
        if fam == "(none)" or " pass2=" in f" {sig}":
            continue
        req = representative(sig)
        ob = out_bytes(req)
        room = MAX_DEVICE_BYTES - pool_bytes(req)
        n_big = min(TABLE_N_WANTED, room // ob if room > 0 else 0)
        if n_big < TABLE_N_MIN:
            continue
        a = desc(req[:7] + (MAX_BATCH, req[8]))
        if a is None or family(signature_of(a, req[8])) != fam:
            continue
        dw, dh = (int(v) for v in a["dst"].split("x"))
        cap = table_launch_cap(dw, dh)
        if cap < TABLE_N_MIN:
            continue
        by_family.setdefault(fam, []).append((ob, sig, n_big, cap))
    out = {}
    for fam in FAMILIES:
        if fam == "(none)":
            continue
        ranked = sorted(by_family.get(fam, []))  # fewest output bytes, then the signature's own order
        first_of_kind, rest, kinds = [], [], set()
        for c in ranked:
            if out_kind(c[1]) in kinds:
                rest.append(c)
            else:
                kinds.add(out_kind(c[1]))
                first_of_kind.append(c)
        out[fam] = [(sig, n_big, cap) for ob, sig, n_big, cap in (first_of_kind + rest)[:TABLE_PER_FAMILY]]
    _CACHE["table"] = out
    return out


def table_unaligned_case():
    """(signature, request, kernel describe names for the same request with outputs that are NOT 16-byte aligned): the fp32 planar signature of a vector-store
    kernel -- one whose kernel differs between the two alignment classes -- with the fewest output bytes, for a full launch group of MAX_TABLE_LAUNCH frames
    followed by a second group of MAX_BATCH.  Under A/B knobs that leave no such signature (TSVPP_FORCE_GATHER=1: every request takes the element-wise
    kernel, whatever the alignment) the smallest fp32 planar signature whose two kernels are the same: the GPU test then still runs and still asserts the
    aligned=0 kernel and the bits.  None only if no single-pass fp32 planar signature fits at all."""
    desc = _Describer()
    differs, same = None, None
    for sig in sorted(signatures()):
        if out_kind(sig) != "f32_planar" or not sig.endswith(" aligned=1") or " pass2=" in f" {sig}":
            continue
        req = representative(sig)
        ob = out_bytes(req)
        if (MAX_TABLE_LAUNCH + MAX_BATCH) * (ob + 4) + pool_bytes(req) > MAX_DEVICE_BYTES:
            continue
        a1, a0 = desc(req[:7] + (MAX_BATCH, 1)), desc(req[:7] + (MAX_BATCH, 0))
        if a1 is None or a0 is None or a1["kernel"] != kernel_name(sig):
            continue
        dw, dh = (int(v) for v in a1["dst"].split("x"))
        if table_launch_cap(dw, dh) < MAX_TABLE_LAUNCH:
            continue
        if a1["kernel"] != a0["kernel"]:
            if differs is None or ob < differs[0]:
                differs = (ob, sig, req, a0["kernel"])
        elif same is None or ob < same[0]:
            same = (ob, sig, req, a0["kernel"])
    best = differs or same
    return None if best is None else best[1:]


def kernel_literals():
    """every kernel name the launchers report, as describe spells it (no blanks): the "vpp_..._kernel<...>" literals of csrc/*.hip"""
    names = set()
    for f in glob.glob(os.path.join(ROOT, "tensor-stream_amd", "csrc", "*.hip")):
        for m in re.findall(r'"(vpp_[A-Za-z0-9_]*_kernel<[^"]*)"', open(f).read()):
            names.add(m.replace(" ", ""))
    return names
