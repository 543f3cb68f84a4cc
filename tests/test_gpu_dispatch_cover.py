"""GPU: every kernel selection the dispatcher makes on the request grid of tests/dispatch_grid.py, run once and checked bit-for-bit against the oracle.

For each signature (what tsvpp_describe decides about a launch, minus its size) the cheapest request of the grid runs as a batch of n DISTINCT random frames:
  * inputs: one 256-byte aligned slot per plane (what describe assumes for in4=); the pitch padding and everything outside the crop box hold a poison --
    0x00 on even frames, 0xFF on odd ones -- and the oracle sees the same planes, so a read outside the legal footprint mismatches on one parity;
  * outputs: one slot per frame in one buffer, 16-byte aligned (or 1 / 4 bytes off for aligned=0), >= 256 guard bytes of a known pattern on both sides,
    the slot itself prefilled with a poison;
  * checks: the launch that went out (tsvpp_debug_last_launch) is the described one; frames 0, n - 1 (and a seeded middle one for small outputs) equal
    oracle.convert byte for byte; every guard is intact; a second call with the frames in reverse order and another prefill gives out2[k] == out1[n - 1 - k]
    (frame-index mix-ups, pixels a launch leaves unwritten) -- and, where the replay cache applies, runs the replayed launch;
  * the table leg: the same n frames once more out of a frame table (tsvpp_convert_table, include/tsvpp.h: "same results, same status codes"), entries
    [5, 5 + n) of a table whose entries 0 .. 4 were never set, into a third guarded buffer: the same launch, intact guards, out3[k] == out1[k].  The pointer
    triples then come from device memory and the crop origin is added in the kernel (vpp_kernels.h: PtrCol), on every cropped signature.

test_table_launches_past_128_frames_... : what only a table can launch.  For up to four signatures of every family (dispatch_grid.table_candidates) a table of
n_big = 1025 entries (fewer where 1025 outputs do not fit) over a pool of 7 distinct source frames -- entry k reads frame k % 7 and writes its own guarded
slot -- is converted in a run of 131 frames (one launch, frame indices >= 128) and then as a whole (launch groups of 1024 + 1).  Every slot of a run must hold
the batch path's image of its pool frame (itself compared with the oracle), every other slot its prefill.  7 is coprime to the 8 XCDs and to 128: a frame
index that wraps or is permuted lands on another frame.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import dispatch_grid as G
from util import knob_run

pytestmark = pytest.mark.gpu

GUARD = 256
TABLE_FIRST = 5  # the table leg converts a run that starts inside its table
# families large enough to split into several tests (each stays well inside the per-test time limit)
CHUNKS = {"vpp_bicubic_cols_kernel": 4, "vpp_bilinear_kernel": 3, "vpp_area_dyadic_kernel": 3, "vpp_bilinear_rows_kernel": 2, "vpp_area_box_kernel": 2,
          "vpp_fused_gather_kernel": 2, "vpp_point_kernel": 2}
# requests the oracle refuses (RuntimeError): {(src, crop, dst, resize type): reason}.  Anything else the oracle refuses fails the test.
ORACLE_REFUSES = {}


@pytest.fixture(scope="module")
def grid():
    by_family = {}
    for sig in sorted(G.signatures()):
        by_family.setdefault(G.family(sig), []).append(sig)
    return by_family


def _live_signature(aligned):
    import tensor_stream as ts
    return G.signature_of(ts.vpp.debug_last_launch(), aligned)


def _first_diff(a, b):
    bad = np.flatnonzero(a != b)
    return (int(bad[0]), int(bad.size)) if bad.size else None


def _fill_inputs(req, gen, dev):
    """n frames of distinct random planes, each in its own 256-byte aligned slot, padding and the area outside the crop box poisoned by frame parity"""
    (w, h, py, puv), crop, dst, rt, fcc, planes, norm, n, aligned = req
    ys_b, uvs_b = h * py, (h // 2) * puv
    sy, suv = (ys_b + 255) // 256 * 256, (uvs_b + 255) // 256 * 256
    buf = torch.randint(0, 256, (n * (sy + suv),), generator=gen, dtype=torch.uint8, device=dev)
    l, t, r, b = crop if crop != (0, 0, 0, 0) else (0, 0, w, h)
    ys, uvs = [], []
    for k in range(n):
        y = buf[k * (sy + suv): k * (sy + suv) + ys_b].view(h, py)
        uv = buf[k * (sy + suv) + sy: k * (sy + suv) + sy + uvs_b].view(h // 2, puv)
        p = 0 if k % 2 == 0 else 255
        # legal footprint: luma rows [t, b) x columns [l, r); chroma rows [t / 2, t / 2 + (b - t) / 2) x bytes [l, r) (src/Crop.cu's pointer arithmetic)
        y[:t] = p
        y[b:] = p
        y[:, :l] = p
        y[:, r:] = p
        c0, c1 = t // 2, t // 2 + (b - t) // 2
        uv[:c0] = p
        uv[c1:] = p
        uv[:, :l] = p
        uv[:, r:] = p
        ys.append(y)
        uvs.append(uv)
    return buf, ys, uvs


def _outputs(nbytes, n, off, pattern, poison, dev):
    """one buffer: [guard | slot | guard] per frame, the slot `off` bytes past a 16-byte boundary; returns the buffer, the byte views of the slots, the
    untouched image of the buffer (guards = pattern) and the slot offsets"""
    stride = (GUARD + off + nbytes + 15) // 16 * 16 + GUARD
    stride = (stride + 255) // 256 * 256
    total = n * stride + GUARD
    tile = (torch.arange(4096, device=dev, dtype=torch.int32) * 131 + pattern).remainder(251).to(torch.uint8)  # (period 4096: no slot is a shifted copy of a guard)
    pat = tile.repeat((total + 4095) // 4096)[:total]
    buf = pat.clone()
    starts = [k * stride + GUARD + off for k in range(n)]
    slots = []
    for s in starts:
        buf[s: s + nbytes] = poison
        slots.append(buf[s: s + nbytes])
    return buf, slots, pat, starts


def _guards_intact(buf, pat, starts, nbytes):
    want = buf.clone()
    for s in starts:
        want[s: s + nbytes] = pat[s: s + nbytes]
    if torch.equal(want, pat):
        return None
    bad = torch.nonzero(want != pat).flatten()[0].item()
    for k, s in enumerate(starts):
        if bad < s:
            return f"guard BEFORE frame {k} damaged at byte {bad - s}"
        if bad < s + nbytes + GUARD:
            return f"guard AFTER frame {k} damaged at byte {bad - s - nbytes}"
    return f"guard byte {bad} damaged"


def _compare_with_oracle(oracle, req, ys, uvs, slots, frames, what):
    """frames `frames` of `slots` equal oracle.convert byte for byte; None, or the reason why the oracle refuses the request (ORACLE_REFUSES)"""
    (w, h, py, puv), crop, dst, rt, fcc, planes, norm, n, aligned = req
    for k in frames:
        y, uv = ys[k].cpu().numpy(), uvs[k].cpu().numpy()
        try:
            ref, _, _ = oracle.convert(y, uv, crop=crop, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=16, width=w)
        except RuntimeError:
            reason = ORACLE_REFUSES.get((req[0], crop, dst, rt))
            assert reason is not None, f"the oracle refuses {what}: not listed in ORACLE_REFUSES"
            return reason
        got = slots[k].cpu().numpy()
        assert got.size == ref.view(np.uint8).size, f"frame {k}: {got.size} bytes, oracle {ref.view(np.uint8).size}: {what}"
        d = _first_diff(got, ref.view(np.uint8))
        assert d is None, f"frame {k} of {n} differs from the oracle at byte {d[0]} ({d[1]} bytes): {what}"
    return None


class _Table:
    """a frame table through the C ABI (tensor_stream._native): the tests choose the capacity, the entries they set and the runs they convert"""

    def __init__(self, vpp, capacity):
        from tensor_stream import _native as N
        self.N, self.vpp, self.lib = N, vpp, vpp._lib
        self.handle = ctypes.c_void_p()
        N.check(self.lib.tsvpp_table_create(vpp._ctx, capacity, ctypes.byref(self.handle)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()  # (a conversion may still be reading the table)
        self.lib.tsvpp_table_destroy(self.handle)
        self.handle = None

    def set(self, first, ys, uvs, slots, width, height):
        n = len(ys)
        fr = (self.N.NV12 * n)(*[self.vpp._frame(ys[i], uvs[i], width, height) for i in range(n)])
        outs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in slots])
        self.N.check(self.lib.tsvpp_table_set(self.handle, first, n, fr, outs, torch.cuda.current_stream().cuda_stream))

    def convert(self, first, n, fp):
        self.N.check(self.lib.tsvpp_convert_table(self.vpp._ctx, self.handle, first, n, ctypes.byref(fp.parameters), torch.cuda.current_stream().cuda_stream))


def _run(vpp, oracle, sig, req, seed):
    """None, or the reason why the oracle refuses the request (ORACLE_REFUSES)"""
    import tensor_stream as ts
    dev = torch.device("cuda", 0)
    (w, h, py, puv), crop, dst, rt, fcc, planes, norm, n, aligned = req
    fp = ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
    f32 = bool(norm) or fcc == 6
    nbytes = G.out_bytes(req)
    off = 0 if aligned else (4 if f32 else 1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    inp, ys, uvs = _fill_inputs(req, gen, dev)
    what = f"signature [{sig}] request {req}"

    def as_out(slots):
        return [s.view(torch.float32) if f32 else s for s in slots]

    buf1, slots1, pat1, starts1 = _outputs(nbytes, n, off, 17, 0xA5, dev)
    vpp.convert_batch(ys, uvs, fp, out=as_out(slots1), width=w, height=h)
    torch.cuda.synchronize()
    live = _live_signature(aligned)
    assert live == sig, f"live launch [{live}] differs from the described {what}"
    g = _guards_intact(buf1, pat1, starts1, nbytes)
    assert g is None, f"{g}: {what}"

    frames = sorted({0, n - 1} | ({int(np.random.default_rng(seed).integers(1, n - 1))} if n > 2 and nbytes <= (1 << 20) else set()))
    reason = _compare_with_oracle(oracle, req, ys, uvs, slots1, frames, what)
    if reason is not None:
        return reason

    # the same batch in reverse order into another buffer with another prefill: frame k of it is frame n - 1 - k of the first
    buf2, slots2, pat2, starts2 = _outputs(nbytes, n, off, 91, 0x5A, dev)
    vpp.convert_batch(ys[::-1], uvs[::-1], fp, out=as_out(slots2), width=w, height=h)
    torch.cuda.synchronize()
    live = _live_signature(aligned)
    assert live == sig, f"second (replayed) launch [{live}] differs from the described {what}"
    g = _guards_intact(buf2, pat2, starts2, nbytes)
    assert g is None, f"second call: {g}: {what}"
    for k in range(n):
        if not torch.equal(slots2[k], slots1[n - 1 - k]):
            d = _first_diff(slots2[k].cpu().numpy(), slots1[n - 1 - k].cpu().numpy())
            raise AssertionError(f"reversed batch: frame {k} != frame {n - 1 - k} of the first call at byte {d[0]} ({d[1]} bytes): {what}")

    # the table leg: the same frames out of entries [TABLE_FIRST, TABLE_FIRST + n) of a frame table whose first entries were never set, into a third buffer.
    # A table launch of n <= 128 frames is the batch launch with the pointer triples in device memory (convert_impl hands launch_fused the same descriptor and
    # the same alignment class; the two-pass formats and "(none)" run over the table's host mirror): EVERY key of the signature is compared, none is exempt.
    buf3, slots3, pat3, starts3 = _outputs(nbytes, n, off, 53, 0x3C, dev)
    with _Table(vpp, n + TABLE_FIRST) as tab:
        tab.set(TABLE_FIRST, ys, uvs, slots3, w, h)
        tab.convert(TABLE_FIRST, n, fp)
        torch.cuda.synchronize()
        live = _live_signature(aligned)
    assert live == sig, f"table launch [{live}] differs from the described {what}"
    g = _guards_intact(buf3, pat3, starts3, nbytes)
    assert g is None, f"table launch: {g}: {what}"
    for k in range(n):
        if not torch.equal(slots3[k], slots1[k]):
            d = _first_diff(slots3[k].cpu().numpy(), slots1[k].cpu().numpy())
            raise AssertionError(f"table launch (entries {TABLE_FIRST} .. {TABLE_FIRST + n - 1}): frame {k} != frame {k} of the batch call at byte {d[0]} ({d[1]} bytes): {what}")
    del inp, ys, uvs, buf1, slots1, pat1, buf2, slots2, pat2, buf3, slots3, pat3
    return None


def _params():
    out = []
    for fam in G.FAMILIES:
        for c in range(CHUNKS.get(fam, 1)):
            out.append(pytest.param(fam, c, id=f"{fam}-{c}"))
    return out


@pytest.mark.parametrize("family,chunk", _params())
def test_every_selection_of_the_family_matches_the_oracle(vpp, oracle, grid, family, chunk):
    sigs = grid.get(family, [])
    n_chunks = CHUNKS.get(family, 1)
    mine = sigs[chunk::n_chunks]
    if not mine:
        # under A/B knobs (tools/knob_matrix*.sh) the grid follows the knobs, and a knob may route a whole family elsewhere (TSVPP_R32=0, TSVPP_AREA_BOX=0, ...)
        if knob_run():
            pytest.skip(f"this knob setting routes no request of the grid to {family}")
        raise AssertionError(f"the grid reaches no {family} launch for chunk {chunk} of {n_chunks}")
    refused = []
    for sig in mine:
        req = G.representative(sig)
        reason = _run(vpp, oracle, sig, req, seed=zlib.crc32(sig.encode()))
        if reason is not None:
            refused.append(f"{req}: {reason}")
    torch.cuda.empty_cache()
    if refused:  # (every other signature of the chunk has been checked by now)
        pytest.skip(f"{len(refused)} of {len(mine)} signatures not compared, the oracle refuses their request: " + "; ".join(refused))


# ---- launches only a frame table can make: more than TSVPP_MAX_BATCH frames -------------------------------------------------------------------------------
BIG_FIRST = 3  # the 131-frame run starts inside its table too


def _slot_view(buf, starts, nbytes):
    """the slots of _outputs as one (n, nbytes) strided view of the buffer"""
    stride = starts[1] - starts[0]
    return buf.as_strided((len(starts), nbytes), (stride, 1), starts[0])


def _check_run(view, expected, first, cnt, poison, what):
    """slot k of the run [first, first + cnt) holds expected[k % TABLE_POOL], every other slot the prefill; one device reduction per pool frame"""
    n_all, P = view.shape[0], expected.shape[0]
    bad = torch.zeros(n_all, dtype=torch.bool, device=view.device)
    for r in range(P):
        k0 = first + (r - first) % P
        if k0 < first + cnt:
            bad[k0: first + cnt: P] = (view[k0: first + cnt: P] != expected[r]).any(dim=1)
    if first > 0:
        bad[:first] = (view[:first] != poison).any(dim=1)
    if first + cnt < n_all:
        bad[first + cnt:] = (view[first + cnt:] != poison).any(dim=1)
    if not bool(bad.any()):
        return
    k = int(torch.nonzero(bad).flatten()[0])
    inside = first <= k < first + cnt
    holds = [f"pool frame {j}" for j in range(P) if torch.equal(view[k], expected[j])]
    if bool((view[k] == poison).all()):
        holds.append("its prefill (never written)")
    want = f"pool frame {k % P}" if inside else "its prefill (outside the run)"
    if inside:
        d = _first_diff(view[k].cpu().numpy(), expected[k % P].cpu().numpy())
        where = f"first difference at byte {d[0]} ({d[1]} bytes)"
    else:
        where = f"{int((view[k] != poison).sum())} bytes written"
    raise AssertionError(f"run of {cnt} entries from {first}: slot {k} must hold {want}, holds {' / '.join(holds) or 'something else'}, {where}; "
                         f"{int(bad.sum())} of {n_all} slots wrong: {what}")


def _pool_and_expected(vpp, oracle, sig, seed):
    """TABLE_POOL distinct poisoned source frames of the signature's representative and their images by the batch path (frames 0 and P - 1 compared with the
    oracle, guards checked): the request, its FrameParameters, the planes and a (P, nbytes) tensor"""
    import tensor_stream as ts
    dev = torch.device("cuda", 0)
    P = G.TABLE_POOL
    req = G.representative(sig)[:7] + (P, G.representative(sig)[8])
    (w, h, py, puv), crop, dst, rt, fcc, planes, norm, n, aligned = req
    fp = ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
    f32 = bool(norm) or fcc == 6
    nbytes = G.out_bytes(req)
    off = 0 if aligned else (4 if f32 else 1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    inp, ys, uvs = _fill_inputs(req, gen, dev)
    what = f"signature [{sig}] request {req}"
    bufe, slotse, pate, startse = _outputs(nbytes, P, off, 17, 0xA5, dev)
    vpp.convert_batch(ys, uvs, fp, out=[s.view(torch.float32) if f32 else s for s in slotse], width=w, height=h)
    torch.cuda.synchronize()
    g = _guards_intact(bufe, pate, startse, nbytes)
    assert g is None, f"{g}: {what}"
    reason = _compare_with_oracle(oracle, req, ys, uvs, slotse, (0, P - 1), what)
    assert reason is None, f"the oracle refuses {what}: {reason}"
    return req, fp, inp, ys, uvs, torch.stack(slotse), off, what


def _run_big(vpp, oracle, family, sig, n_big, cap, seed):
    import tensor_stream as ts
    dev = torch.device("cuda", 0)
    P = G.TABLE_POOL
    req, fp, inp, ys, uvs, expected, off, what = _pool_and_expected(vpp, oracle, sig, seed)
    (w, h, py, puv) = req[0]
    nbytes = expected.shape[1]
    what = f"table of {n_big} entries, {what}"
    poison = 0xC3
    buf, slots, pat, starts = _outputs(nbytes, n_big, off, 29, poison, dev)
    view = _slot_view(buf, starts, nbytes)
    with _Table(vpp, n_big) as tab:
        tab.set(0, [ys[k % P] for k in range(n_big)], [uvs[k % P] for k in range(n_big)], slots, w, h)  # the inputs alias, the outputs do not
        runs = ((min(BIG_FIRST, n_big - G.TABLE_N_MIN), G.TABLE_N_MIN, G.TABLE_N_MIN),   # one launch, frame indices of 128 and above
                (0, n_big, (n_big - 1) % cap + 1))           # launch groups of `cap` frames: debug_last_launch describes the last one (1025: 1024 + 1)
        for first, cnt, last_frames in runs:
            view.fill_(poison)
            tab.convert(first, cnt, fp)
            torch.cuda.synchronize()
            live = ts.vpp.debug_last_launch()
            assert live["frames"] == last_frames, f"run of {cnt} entries from {first}: the last launch took {live['frames']} frames, not {last_frames}: {what}"
            assert live["kernel"].split("<")[0] == family, f"run of {cnt} entries from {first}: the launch went to {live['kernel']}, not to {family}: {what}"
            _check_run(view, expected, first, cnt, poison, what)
            g = _guards_intact(buf, pat, starts, nbytes)
            assert g is None, f"run of {cnt} entries from {first}: {g}: {what}"
    del inp, ys, uvs, buf, slots, pat, view, expected


@pytest.mark.parametrize("family", [f for f in G.FAMILIES if f != "(none)"])
def test_table_launches_past_128_frames_give_every_slot_its_own_frame(vpp, oracle, grid, family):
    cands = G.table_candidates().get(family, [])
    if not cands:
        if knob_run() and not grid.get(family):
            pytest.skip(f"this knob setting routes no request of the grid to {family}")
        raise AssertionError(f"no signature of {family} can be converted out of a table of more than {G.MAX_BATCH} frames (dispatch_grid.table_candidates)")
    for sig, n_big, cap in cands:
        _run_big(vpp, oracle, family, sig, n_big, cap, seed=zlib.crc32(sig.encode()) ^ 0x7AB1E)
    torch.cuda.empty_cache()


def test_one_misaligned_output_moves_its_whole_launch_group_to_the_element_wise_kernel(vpp, oracle):
    """convert_impl decides the store alignment per launch group from the table's host mirror (outs_aligned16 over the group's entries): ONE output that is
    not 16-byte aligned -- entry 700 of a 1024-entry group, 4 bytes off -- puts the whole group into the aligned=0 class, i.e. onto the kernel describe names
    for outputs that are not aligned, and only that group: a run of 1024 + 128 entries converts its second group, whose outputs are all aligned, with the
    aligned=1 kernel again (check_frames' all_vec covers the whole run, but only decides whether UYVY / YUV444 take one pass: no part in an fp32 planar
    request).  The bits of every slot stay the same.  debug_last_launch carries no aligned= key: the class shows in the kernel's name."""
    import tensor_stream as ts
    case = G.table_unaligned_case()
    assert case is not None, "the grid holds no single-pass fp32 planar signature that fits a table launch of 1024 + 128 frames"
    sig, _, unaligned_kernel = case
    aligned_kernel = G.kernel_name(sig)
    if not knob_run():  # (TSVPP_FORCE_GATHER=1 leaves one kernel for both classes: the test then still checks that kernel, the bits and the guards)
        assert unaligned_kernel != aligned_kernel, f"the kernel of [{sig}] does not depend on the output alignment"
    dev = torch.device("cuda", 0)
    P, group, n, odd = G.TABLE_POOL, G.MAX_TABLE_LAUNCH, G.MAX_TABLE_LAUNCH + G.MAX_BATCH, 700
    req, fp, inp, ys, uvs, expected, off, what = _pool_and_expected(vpp, oracle, sig, seed=zlib.crc32(sig.encode()) ^ 0x0DD)
    assert off == 0
    (w, h, py, puv) = req[0]
    nbytes = expected.shape[1]
    poison = 0x3C
    # every slot 16-byte aligned with 4 spare bytes behind it, still inside the slot's own stride (the guards follow the spare bytes); entry `odd` starts 4 bytes later
    buf, slots, pat, starts = _outputs(nbytes + 4, n, 0, 71, poison, dev)
    starts = [s + (4 if k == odd else 0) for k, s in enumerate(starts)]
    slots = [buf[s: s + nbytes] for s in starts]
    for k, s in enumerate(starts):  # the 4 bytes of each slot that no frame covers are guard again
        lo = s - 4 if k == odd else s + nbytes
        buf[lo: lo + 4] = pat[lo: lo + 4]
    assert [s.data_ptr() % 16 for s in slots] == [4 if k == odd else 0 for k in range(n)]
    prefilled = buf.clone()
    with _Table(vpp, n) as tab:
        tab.set(0, [ys[k % P] for k in range(n)], [uvs[k % P] for k in range(n)], slots, w, h)
        # (entries, frames of the last launch, its kernel): the group that holds entry 700 alone; then that group and an aligned one behind it
        for cnt, last_frames, kernel in ((group, group, unaligned_kernel), (n, n - group, aligned_kernel)):
            buf.copy_(prefilled)
            tab.convert(0, cnt, fp)
            torch.cuda.synchronize()
            live = ts.vpp.debug_last_launch()
            assert live["frames"] == last_frames, f"run of {cnt} entries: {live['frames']} frames in the last launch, not {last_frames}: {what}"
            assert live["kernel"] == kernel, \
                f"run of {cnt} entries, entry {odd} misaligned: the last launch ({last_frames} frames) ran {live['kernel']}, not {kernel}; describe names " \
                f"{unaligned_kernel} for aligned=0 and {aligned_kernel} for aligned=1: {what}"
            g = _guards_intact(buf, pat, starts, nbytes)
            assert g is None, f"run of {cnt} entries: {g}: {what}"
            for k in range(n):
                want = expected[k % P] if k < cnt else None
                if not (torch.equal(slots[k], want) if k < cnt else bool((slots[k] == poison).all())):
                    if want is None:
                        raise AssertionError(f"run of {cnt} entries: slot {k} lies outside the run and was written: {what}")
                    d = _first_diff(slots[k].cpu().numpy(), want.cpu().numpy())
                    raise AssertionError(f"run of {cnt} entries: slot {k} != pool frame {k % P} at byte {d[0]} ({d[1]} bytes): {what}")
    del inp, ys, uvs, buf, slots, pat, expected, prefilled
