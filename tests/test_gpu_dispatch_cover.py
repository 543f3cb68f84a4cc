"""GPU: every kernel selection the dispatcher makes on the request grid of tests/dispatch_grid.py, run once and checked bit-for-bit against the oracle.

For each signature (what tsvpp_describe decides about a launch, minus its size) the cheapest request of the grid runs as a batch of n DISTINCT random frames:
  * inputs: one 256-byte aligned slot per plane (what describe assumes for in4=); the pitch padding and everything outside the crop box hold a poison --
    0x00 on even frames, 0xFF on odd ones -- and the oracle sees the same planes, so a read outside the legal footprint mismatches on one parity;
  * outputs: one slot per frame in one buffer, 16-byte aligned (or 1 / 4 bytes off for aligned=0), >= 256 guard bytes of a known pattern on both sides,
    the slot itself prefilled with a poison;
  * checks: the launch that went out (tsvpp_debug_last_launch) is the described one; frames 0, n - 1 (and a seeded middle one for small outputs) equal
    oracle.convert byte for byte; every guard is intact; a second call with the frames in reverse order and another prefill gives out2[k] == out1[n - 1 - k]
    (frame-index mix-ups, pixels a launch leaves unwritten) -- and, where the replay cache applies, runs the replayed launch.
"""
import zlib

import numpy as np
import pytest
import torch

import dispatch_grid as G
from util import knob_run

pytestmark = pytest.mark.gpu

GUARD = 256
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
    for k in frames:
        y, uv = ys[k].cpu().numpy(), uvs[k].cpu().numpy()
        try:
            ref, _, _ = oracle.convert(y, uv, crop=crop, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=16, width=w)
        except RuntimeError:
            reason = ORACLE_REFUSES.get((req[0], crop, dst, rt))
            assert reason is not None, f"the oracle refuses {what}: not listed in ORACLE_REFUSES"
            return reason
        got = slots1[k].cpu().numpy()
        assert got.size == ref.view(np.uint8).size, f"frame {k}: {got.size} bytes, oracle {ref.view(np.uint8).size}: {what}"
        d = _first_diff(got, ref.view(np.uint8))
        assert d is None, f"frame {k} of {n} differs from the oracle at byte {d[0]} ({d[1]} bytes): {what}"

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
    del inp, ys, uvs, buf1, slots1, pat1, buf2, slots2, pat2
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
