"""Shared by the tensor tests (tsvpp_convert_rois_tensor / tsvpp_convert_letterbox_tensor): the expected bits, built from the existing oracle only.

The contract (include/tsvpp.h): with q the fp32 value the existing entry point stores (the oracle's fp32 planar result; letterbox_util.expected_canvas for a
canvas), the element of stored channel c is cvt(dtype, (q - mean[c]) * scale[c]) -- a float32 subtraction, a float32 multiplication, one conversion that rounds
to nearest even.  numpy's float32 arithmetic and .astype(np.float16), and torch's .to(torch.bfloat16), are exactly those operations.  Everything is compared
with np.array_equal on raw bytes: there is no tolerance anywhere."""
import zlib

import numpy as np
import torch

F32, F16, BF16 = "f32", "f16", "bf16"
DTYPES = (F32, F16, BF16)
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
CODE = {F32: 0, F16: 1, BF16: 2}  # enum tsvpp_dtype
ESIZE = {F32: 4, F16: 2, BF16: 2}

# (mean, std) per STORED channel; the facade's scale is np.float32(1) / np.float32(std)
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
# means that are exactly a q (k / 255 for k = 0, 114, 255: exact zeros occur); scales -1 (negative values), 2^-12 (fp16 subnormals), 3
CORNER = (tuple(float(np.float32(k) / np.float32(255)) for k in (0, 114, 255)), (-1.0, 4096.0, float(np.float32(1) / np.float32(3))))
SPECS = {"identity": IDENTITY, "imagenet": IMAGENET, "corner": CORNER}


def scales(std):
    """what the Python facade hands the library for `std`"""
    with np.errstate(over="ignore", divide="ignore"):
        return [np.float32(1) / np.float32(s) for s in std]


assert [float(s) for s in scales(CORNER[1])] == [-1.0, 2.0 ** -12, 3.0]


def apply(q, channels, mean, scale, dtype):
    """q: the oracle's fp32 PLANAR result (flat or (channels, ...)), mean / scale per stored channel -> the expected output as raw bytes"""
    q = np.ascontiguousarray(q, np.float32).reshape(channels, -1)
    v = np.empty_like(q)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(channels):
            v[c] = (q[c] - np.float32(mean[c])) * np.float32(scale[c])
        if dtype == F32:
            out = v
        elif dtype == F16:
            out = v.astype(np.float16)
        else:
            out = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy()
    return np.ascontiguousarray(out).ravel().view(np.uint8)


def expected(q, channels, spec, dtype):
    """apply() for a (mean, std) pair, with the facade's scale"""
    return apply(q, channels, spec[0], scales(spec[1]), dtype)


def bits(t):
    """raw bytes of a torch tensor of any element type"""
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy().ravel().view(np.uint8)


def crc32_zlib(buf):
    """the CRC cpp/vpp_letterbox.cpp prints"""
    return zlib.crc32(bytes(buf)) & 0xFFFFFFFF
