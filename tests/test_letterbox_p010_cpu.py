"""No GPU: the host side of tsvpp_convert_letterbox_p010 / tsvpp_describe_letterbox_p010 (include/tsvpp.h) -- every status of the contract through the describe
call (and the convert call with a null context: the request is checked before the context is touched), the describe line -- and the model of tests/p010_util.py
held to a plain float64 evaluation of the same formulas."""
import ctypes

import numpy as np
import pytest

import p010_util as M

OK, UNSUPPORTED, ERROR = 0, -2, -3
BICUBIC, AREA = 2, 3
SPAN = 0xFFFFFFF0  # TSVPP_SOURCE_SPAN_LIMIT


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def both(native, frames=((1920, 1080, 4096),), dst=(640, 640), rt=M.BILINEAR, fcc=M.RGB24, planes=M.PLANAR, norm=1, rects=None, pad=(64, 512, 512), spec=None, n=None,
         ptr=(0, 0)):
    L = native.lib()
    p = native.Params(0, 0, 0, 0, dst[0], dst[1], rt, fcc, planes, norm)
    fr = (native.P010 * max(len(frames), 1))(*[native.P010(ptr[0] or None, ptr[1] or None, f[2] if len(f) > 2 else 0, f[3] if len(f) > 3 else (f[2] if len(f) > 2 else 0),
                                                           f[0], f[1]) for f in frames])
    rc = None if rects is None else (native.Rect * len(rects))(*[native.Rect(*r) for r in rects])
    sp = None if spec is None else ctypes.byref(native.TensorSpec(spec, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)))
    outs = (ctypes.c_void_p * max(len(frames), 1))()
    buf = ctypes.create_string_buffer(512)
    cnt = len(frames) if n is None else n
    d = L.tsvpp_describe_letterbox_p010(ctypes.byref(p), sp, cnt, fr, rc, 1, buf, len(buf))
    c = L.tsvpp_convert_letterbox_p010(None, cnt, fr, ctypes.byref(p), sp, rc, pad[0], pad[1], pad[2], outs, None)
    return d, c, buf.value.decode()


# (request, status of the describe call, status of the convert call with a null context -- TSVPP_ERROR where the request itself is accepted)
STATUS = [
    (dict(), OK, ERROR),
    (dict(spec=1), OK, ERROR),
    (dict(n=0), ERROR, ERROR),
    (dict(frames=((1920, 1080, 3838),)), ERROR, ERROR),                       # a pitch below 2 * width
    (dict(frames=((1920, 1080, 4096, 3838),)), ERROR, ERROR),                 # ... of the chroma plane
    (dict(frames=((1920, 1080, 4097),)), ERROR, ERROR),                       # an odd pitch
    (dict(frames=((1920, 1080, 4097),), rt=BICUBIC), ERROR, ERROR),           # TSVPP_ERROR comes first
    (dict(pad=(1024, 512, 512)), OK, ERROR),                                  # (the describe call takes no pad)
    (dict(pad=(64, -1, 512), rt=BICUBIC), UNSUPPORTED, ERROR),
    (dict(rects=[(0, 0, 642, 640)]), ERROR, ERROR),
    (dict(frames=((1921, 1080, 4096),)), UNSUPPORTED, UNSUPPORTED),           # the evenness rules
    (dict(rects=[(1, 0, 638, 360)]), UNSUPPORTED, UNSUPPORTED),
    (dict(rt=BICUBIC), UNSUPPORTED, UNSUPPORTED),
    (dict(rt=AREA), UNSUPPORTED, UNSUPPORTED),
    (dict(rt=9), UNSUPPORTED, UNSUPPORTED),
    (dict(frames=((64, 4098, 2 * (SPAN // 4097 // 2 + 1)),)), UNSUPPORTED, UNSUPPORTED),  # a plane span at the limit
    (dict(fcc=3), UNSUPPORTED, UNSUPPORTED),                                  # NV12 output: not a letterbox flavour
    (dict(spec=1, planes=M.MERGED), UNSUPPORTED, UNSUPPORTED),                # merged tensors
    (dict(spec=7), UNSUPPORTED, UNSUPPORTED),                                 # tensor rule 3: an unknown dtype
    (dict(ptr=(0x1001, 0x2000)), OK, ERROR),                                  # converting: a plane pointer that is not 2-byte aligned
]


@pytest.mark.parametrize("req,describe,convert", STATUS)
def test_status_table(native, req, describe, convert):
    d, c, _ = both(native, **req)
    assert (d, c) == (describe, convert), req


def test_describe_line(native):
    d, _, text = both(native, frames=[(1920, 1080, 4096)] * 33, planes=M.MERGED, norm=0)
    kv = dict(item.partition("=")[::2] for item in text.split(" "))
    assert d == OK and kv["src"] == "p010" and kv["frames"] == "33" and kv["launches"] == "2" and kv["limit"] == "32" and kv["mode"] == "bilinear"
    assert kv["kernel"] == "vpp_letterbox_p010<M_BILINEAR,O_U8_MERGED,vec,staged>" and kv["staged"] == "33" and kv["inner"] == "640x360+0+140"
    _, _, text = both(native, spec=1, rt=M.NEAREST)
    assert "kernel=vpp_letterbox_p010_tensor<M_NEAREST,PLANAR,EL_HALF,vec,staged>" in text and "out=f16_planar" in text


def test_model_against_float64():
    """The model's channel values k against a float64 evaluation of the same formulas WITHOUT the truncations, on one seeded 16 x 8 frame into 24 x 12 (BILINEAR).
    The bound per channel, in units of k, follows from the contract alone: the truncation of the resized luma moves Y by less than 1, hence the channel by less
    than y_scale = 1.164; the truncations of U and V move the chroma term by less than v_to_r = 1.596 (R), u_to_b = 2.018 (B), |v_to_g| + |u_to_g| = 1.204 (G);
    the final truncation by less than 1; the clamps are contractions.  The coefficients are used at their float32 values in both evaluations; float32 rounding of
    the coordinates, weights and sums (a few ulp of values up to 2^11, i.e. below 1e-3 each over some ten operations) is covered by a slack of 0.05."""
    rng = np.random.default_rng(7)
    w, h, cw, ch = 16, 8, 24, 12
    y, uv = rng.integers(0, 65536, (h, w), dtype=np.uint16), rng.integers(0, 65536, (h // 2, w), dtype=np.uint16)
    k = M.channels(*M.virtual_frame(y, uv, w, h, (0, 0, cw, ch), (cw, ch), M.BILINEAR, (0, 0, 0)), M.RGB24)

    def plane(S, n_out_r, n_out_c, taps_r, taps_c):
        def axis(n, ratio, limit, taps):
            f = (np.arange(n) + 0.5) * ratio - 0.5
            p = np.floor(f)
            wgt = np.where((p < 0) | (p > limit - 1), 0.0, f - p)
            p = np.clip(p, 0, limit - 1).astype(int)
            return p, np.where(p + 1 >= taps, p, p + 1), wgt
        r, r2, wy = axis(n_out_r, h / ch, h, taps_r)
        c, c2, wx = axis(n_out_c, w / cw, w, taps_c)
        S = S.astype(np.float64)
        wx, wy = wx[None, :], wy[:, None]
        return S[np.ix_(r, c)] * (1 - wx) * (1 - wy) + S[np.ix_(r, c2)] * wx * (1 - wy) + S[np.ix_(r2, c)] * (1 - wx) * wy + S[np.ix_(r2, c2)] * wx * wy

    Ys, UVs = M.samples(y), M.samples(uv)
    Y = plane(Ys, ch, cw, h, w)
    U, V = (np.repeat(np.repeat(plane(UVs[:, o::2], ch // 2, cw // 2, h // 2, w // 2), 2, 0), 2, 1) for o in (0, 1))
    y_scale, v_to_r, u_to_b, v_to_g, u_to_g, bias, y_off, c_off = (float(v) for v in M.COEFFS)
    yv = np.maximum(0.0, Y - 4 * y_off) * y_scale
    real = [np.clip(yv + t, 0, 1023) for t in (v_to_r * (V - 4 * c_off) + bias, v_to_g * (V - 4 * c_off) + u_to_g * (U - 4 * c_off) + bias, u_to_b * (U - 4 * c_off) + bias)]
    for name, kc, rc, chroma in zip("RGB", k, real, (1.596, 1.204, 2.018)):
        err = np.abs(kc - rc).max()
        print(name, "max |k - real| =", err)
        assert err <= 1 + 1.164 + chroma + 0.05, name
    assert np.array_equal(M.quotient(np.arange(1024)), np.array([np.float32(i / 1023) for i in range(1024)]))
