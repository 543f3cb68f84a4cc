"""Python host side of the VPP path: enums + FrameParameters mirroring the reference's Python
surface (tensor_stream/tensor_stream.py:48-136), and `VideoProcessor`, the counterpart of the C++
class (include/VideoProcessor.h:120-149) that drives the HIP kernels through the C ABI.

PyTorch is plumbing here: it owns device memory and the current stream; all compute is in libtsvpp.so.
"""
import ctypes
from enum import Enum

import numpy as np
import torch

from . import _native as N


OPT_INPUTS_READY = N.TSVPP_OPT_INPUTS_READY
OPT_COLOR_G_TERM = N.TSVPP_OPT_COLOR_G_TERM
OPT_UNSAFE_COEFFS = N.TSVPP_OPT_UNSAFE_COEFFS


class FourCC(Enum):  # reference tensor_stream/tensor_stream.py:48-62
    Y800 = 0
    RGB24 = 1
    BGR24 = 2
    NV12 = 3
    UYVY = 4
    YUV444 = 5
    HSV = 6


class ResizeType(Enum):  # :67-75
    NEAREST = 0
    BILINEAR = 1
    BICUBIC = 2
    AREA = 3


class Planes(Enum):  # :79-83
    PLANAR = 0
    MERGED = 1


def _v(x):
    return x.value if isinstance(x, Enum) else int(x)


class FrameParameters:
    """Same constructor as the reference's FrameParameters (tensor_stream/tensor_stream.py:101-136).
    normalization=None keeps the C++ default: False, except True for HSV (include/VideoProcessor.h:40-47)."""

    def __init__(self, width=0, height=0, crop_coords=(0, 0, 0, 0), resize_type=ResizeType.NEAREST,
                 pixel_format=FourCC.RGB24, planes_pos=Planes.MERGED, normalization=None):
        if normalization is None:
            normalization = _v(pixel_format) == FourCC.HSV.value
        self.parameters = N.Params(int(crop_coords[0]), int(crop_coords[1]), int(crop_coords[2]), int(crop_coords[3]),
                                   int(width), int(height), _v(resize_type), _v(pixel_format), _v(planes_pos),
                                   int(bool(normalization)))

    def __repr__(self):
        p = self.parameters
        return (f"FrameParameters(width={p.dst_width}, height={p.dst_height}, "
                f"crop=({p.crop_left},{p.crop_top},{p.crop_right},{p.crop_bottom}), resize_type={p.resize_type}, "
                f"pixel_format={p.fourcc}, planes_pos={p.planes}, normalization={bool(p.normalization)})")


_TENSOR_DTYPES = {torch.float32: N.TSVPP_F32, torch.float16: N.TSVPP_F16, torch.bfloat16: N.TSVPP_BF16}


def tensor_spec(dtype=None, mean=None, std=None):
    """The tsvpp_tensor_spec of the keyword arguments dtype / mean / std that convert_rois, convert_rois_area, convert_letterbox and their describe functions
    take, or None when all three are None (then those run the entry points they always ran).  dtype: torch.float16 / torch.bfloat16 / torch.float32 (default
    float32); mean / std: a number for every channel or one per STORED channel (plane 0, 1, 2 after the RGB / BGR choice; Y800 reads the first), defaults 0 and 1.
    The library multiplies, it never divides: the scale it is given is np.float32(1) / np.float32(std), rounded once, so an element is
    cvt(dtype, (q - float32(mean)) * scale) with q the fp32 value the call stores without these arguments (k / 255) -- the bits of `(q - mean) * (1 / std)` in
    float32, which can differ in the last bit from `(q - mean) / std`."""
    if dtype is None and mean is None and std is None:
        return None
    dt = torch.float32 if dtype is None else dtype
    if dt not in _TENSOR_DTYPES:
        raise RuntimeError(f"-3: tensor outputs are torch.float16, torch.bfloat16 or torch.float32, not {dt}")

    def three(v, default):
        if v is None:
            v = default
        v = [v] * 3 if isinstance(v, (int, float, np.floating)) else list(v)
        if len(v) == 1:
            v = v * 3
        if len(v) != 3:
            raise ValueError(f"mean / std hold one value or three, not {len(v)}")
        return [np.float32(x) for x in v]

    m, sd = three(mean, 0.0), three(std, 1.0)
    with np.errstate(divide="ignore", over="ignore"):
        sc = [np.float32(1) / x for x in sd]  # (std = 0 gives an infinite scale: the library answers TSVPP_ERROR)
    return N.TensorSpec(_TENSOR_DTYPES[dt], (ctypes.c_float * 3)(*m), (ctypes.c_float * 3)(*sc))


def _torch_dtype(spec):
    return {v: k for k, v in _TENSOR_DTYPES.items()}[spec.dtype]


def output_shape(p, out_w, out_h):
    """Tensor shape of TensorStream::getFrame (reference src/Wrappers/WrapperPython.cpp:317-341)."""
    ch = N.lib().tsvpp_channels(p.fourcc)
    if p.fourcc in (FourCC.RGB24.value, FourCC.BGR24.value):
        return (out_h, out_w, 3) if p.planes == Planes.MERGED.value else (3, out_h, out_w)
    if p.fourcc in (FourCC.YUV444.value, FourCC.HSV.value):
        return (out_h, out_w, 3)
    return (1, int(out_h * ch), out_w)


class VideoProcessor:
    """Counterpart of the reference's `VideoProcessor` (Init / Convert / Close), with
    caller-visible torch tensors instead of AVFrame::opaque.

    Convert() takes the NV12 planes as uint8 CUDA tensors (2-D: rows x pitch) and returns a new
    tensor, or fills `out`.  Work is enqueued on torch's current stream unless a consumer name is
    given, in which case that consumer's pooled stream is used (reference src/VideoProcessor.cpp:98-104)
    after making it wait for the current stream.
    """

    def __init__(self, device=None, max_consumers=5):
        self._ctx = ctypes.c_void_p()
        self._tables = []    # persistent frame tables (make_table): destroyed before the context
        self._lib = N.lib()  # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise RuntimeError("VideoProcessor needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        N.check(self._lib.tsvpp_create(self.device, int(max_consumers), ctypes.byref(self._ctx)))

    # reference naming
    def Close(self):
        if self._ctx:
            if self._tables:
                torch.cuda.synchronize(self.device)
                for h in self._tables:
                    self._lib.tsvpp_table_destroy(h)
                self._tables = []
            self._lib.tsvpp_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    close = Close

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass

    def out_dims(self, params, in_w, in_h):
        p = params.parameters if isinstance(params, FrameParameters) else params
        w, h = ctypes.c_int(0), ctypes.c_int(0)
        N.check(self._lib.tsvpp_out_dims(ctypes.byref(p), in_w, in_h, ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def prepare(self, params, in_w, in_h, n_frames=0, stream=None):
        """Pre-builds what the request needs (AREA tables, the geometry tables of the 2x2-tap kernel for a batch of `n_frames`;
        with n_frames > 0 also the UYVY / YUV444 scratch of `stream`, default torch's current stream) so that later
        conversions allocate nothing -- e.g. before graph capture."""
        p = params.parameters if isinstance(params, FrameParameters) else params
        if n_frames and stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self._lib.tsvpp_prepare_batch(self._ctx, ctypes.byref(p), in_w, in_h, int(n_frames), stream or 0))

    def enable_markers(self, on=True):
        """roctx ranges around every conversion (the reference's NVTX ranges); RuntimeError if no roctx library exists."""
        N.check(self._lib.tsvpp_enable_markers(self._ctx, 1 if on else 0))

    def consumer_stream(self, name):
        s = ctypes.c_void_p()
        N.check(self._lib.tsvpp_consumer_stream(self._ctx, name.encode(), ctypes.byref(s)))
        return s.value or 0

    def consumer_next_stream(self, name, launch_bytes=0):
        """The stream the consumer's next conversion should go to (tsvpp_consumer_next_stream): its one stream by default; under OPT_INPUTS_READY small launches
        alternate between the consumer's two streams."""
        s = ctypes.c_void_p()
        N.check(self._lib.tsvpp_consumer_next_stream(self._ctx, name.encode(), int(launch_bytes), ctypes.byref(s)))
        return s.value or 0

    def consumer_synchronize(self, name):
        N.check(self._lib.tsvpp_consumer_synchronize(self._ctx, name.encode()))

    def set_option(self, option, value):
        """Context options of include/tsvpp.h, e.g. set_option(OPT_INPUTS_READY, 1)."""
        N.check(self._lib.tsvpp_set_option(self._ctx, int(option), int(value)))

    def get_option(self, option):
        v = ctypes.c_int(0)
        N.check(self._lib.tsvpp_get_option(self._ctx, int(option), ctypes.byref(v)))
        return v.value

    def _alloc(self, p, in_w, in_h, n=None, dtype=None):
        ow, oh = self.out_dims(p, in_w, in_h)
        shape = output_shape(p, ow, oh)
        if dtype is None:  # (else: the element of a tensor entry point)
            dtype = torch.float32 if (p.normalization or p.fourcc == FourCC.HSV.value) else torch.uint8
        if n is None:
            return torch.empty(shape, dtype=dtype, device=f"cuda:{self.device}")
        # batch: every frame must start 16-byte aligned or its launch group falls back to the element-wise kernel
        # (uint8 frames of e.g. 250 x 250 x 3 bytes are not a multiple of 16): pad the frame stride, return a view
        numel = 1
        for d in shape:
            numel *= d
        esz = torch.empty((), dtype=dtype).element_size()
        stride = (numel * esz + 15) // 16 * 16 // esz
        flat = torch.empty(n * stride, dtype=dtype, device=f"cuda:{self.device}")
        inner = []
        acc = 1
        for d in reversed(shape):
            inner.insert(0, acc)
            acc *= d
        return flat.as_strided((n,) + tuple(shape), (stride,) + tuple(inner))

    def _alloc_items(self, p, n, spec, needs):
        """The outputs of convert_rois / convert_letterbox: n frames of the parameters' own size (no stage changes it), in the spec's element if there is one."""
        if p.dst_width <= 0 or p.dst_height <= 0 or (p.dst_width | p.dst_height) & 1:
            raise RuntimeError(f"-3: {needs} (width / height of the parameters)")
        return self._alloc(p, p.dst_width, p.dst_height, n, None if spec is None else _torch_dtype(spec))

    @staticmethod
    def _frame(y, uv, width, height):
        assert y.is_cuda and uv.is_cuda and y.dtype == torch.uint8 and uv.dtype == torch.uint8
        assert y.dim() == 2 and uv.dim() == 2 and y.stride(1) == 1 and uv.stride(1) == 1
        h = y.shape[0] if height is None else height
        w = y.shape[1] if width is None else width
        return N.NV12(y.data_ptr(), uv.data_ptr(), y.stride(0), uv.stride(0), w, h)

    def Convert(self, y, uv, params, out=None, width=None, height=None, consumer=None):
        p = params.parameters if isinstance(params, FrameParameters) else params
        fr = self._frame(y, uv, width, height)
        if out is None:
            out = self._alloc(p, fr.width, fr.height)
        cur = torch.cuda.current_stream(self.device)
        stream = cur.cuda_stream
        ext = None
        if consumer is not None:
            stream, ext = self._on_consumer_stream(consumer)
        N.check(self._lib.tsvpp_convert(self._ctx, ctypes.byref(fr), ctypes.byref(p), out.data_ptr(), stream))
        if ext is not None:
            cur.wait_stream(ext)  # later work on torch's stream sees the finished tensor (no host sync)
        return out

    convert = Convert

    def convert_batch(self, ys, uvs, params, out=None, width=None, height=None):
        """ys / uvs: 3-D uint8 tensors (n, rows, pitch) or lists of 2-D tensors; one launch per 128 frames.
        Returns (or fills `out`, indexed out[i]) a tensor of shape (n, ...frame shape).  NOTE the frame stride of the tensor this
        method allocates: every frame starts 16-byte aligned (the vector-store kernels need that), so when a frame's bytes are
        not a multiple of 16 (e.g. 250 x 250 x 3 uint8) the batch tensor is a strided VIEW with a padded stride(0) -- out[i] is
        contiguous, the batch as a whole is not (`.contiguous()` compacts it; pass your own `out` to choose the layout: frames
        that are not 16-byte aligned then take the element-wise kernel)."""
        p = params.parameters if isinstance(params, FrameParameters) else params
        n = len(ys)
        frames = (N.NV12 * n)(*[self._frame(ys[i], uvs[i], width, height) for i in range(n)])
        if out is None:
            out = self._alloc(p, frames[0].width, frames[0].height, n)
        outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self._lib.tsvpp_convert_batch(self._ctx, n, frames, ctypes.byref(p), outs, stream))
        return out

    def convert_rois(self, ys, uvs, rois, params, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """The cascade behind a detector (tsvpp_convert_rois): every box of `rois` is cut out of its frame, resized to params' width x height,
        colour-converted and stored to its own output, one launch per 64 boxes.  ys / uvs: the NV12 planes of ONE frame (a pair of 2-D uint8
        tensors: rows x pitch) or lists of them -- the frames may differ in size and pitch; rois: (left, top, right, bottom) boxes of frame 0 or
        (frame, left, top, right, bottom); width / height: the frames' picture size (an int for all frames or one per frame; default: the planes'
        own).  Returns (or fills `out`, indexed out[i]) a tensor of shape (n, ...frame shape) with the padded frame stride of convert_batch
        (every box starts 16-byte aligned), on torch's current stream.  AREA has its own method, convert_rois_area; this one refuses it.
        dtype / mean / std (see tensor_spec): with any of them given the boxes come out as what a network takes -- (x / 255 - mean[c]) * (1 / std[c]) in
        torch.float16 / bfloat16 / float32, planar RGB24 / BGR24 or Y800 with normalization=True -- through tsvpp_convert_rois_tensor, which accepts AREA too."""
        return self._convert_rois(self._lib.tsvpp_convert_rois, ys, uvs, rois, params, out, width, height, tensor_spec(dtype, mean, std))

    def convert_rois_area(self, ys, uvs, rois, params, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """convert_rois for ResizeType.AREA (tsvpp_convert_rois_area), same arguments and result: every box with both ratios above 1 is averaged with the AREA
        down-scale, any other box takes AREA's up-scale rule; the weight rows are generated inside the kernel, so the call allocates and caches nothing however
        many distinct box sizes it sees.  Any other resize type is refused.  dtype / mean / std: as convert_rois (the same tensor entry point, which then
        takes every resize type)."""
        return self._convert_rois(self._lib.tsvpp_convert_rois_area, ys, uvs, rois, params, out, width, height, tensor_spec(dtype, mean, std))

    def _convert_rois(self, entry, ys, uvs, rois, params, out, width, height, spec=None):
        p = params.parameters if isinstance(params, FrameParameters) else params
        ys, uvs, boxes = _normalize_rois(ys, uvs, rois)
        widths, heights = _per_frame(width, len(ys)), _per_frame(height, len(ys))
        frames = (N.NV12 * len(ys))(*[self._frame(ys[i], uvs[i], widths[i], heights[i]) for i in range(len(ys))])
        n = len(boxes)
        if n == 0:
            raise RuntimeError("-3: convert_rois needs at least one box")
        if out is None:
            out = self._alloc_items(p, n, spec, "convert_rois needs an even, positive output size")
        recs = (N.Roi * n)(*[N.Roi(*b) for b in boxes])
        outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if spec is None:
            N.check(entry(self._ctx, len(ys), frames, n, recs, ctypes.byref(p), outs, stream))
        else:
            N.check(self._lib.tsvpp_convert_rois_tensor(self._ctx, len(ys), frames, n, recs, ctypes.byref(p), ctypes.byref(spec), outs, stream))
        return out

    def convert_rois_sized(self, ys, uvs, rois, params, sizes, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """convert_rois with the output size PER BOX (tsvpp_convert_rois_sized): text lines of one height and their own widths (sizes_for_height), the levels of
        a pyramid (pyramid_sizes), the inputs of several heads behind one detector pass -- one call, one launch per 48 boxes of a store class.  ys / uvs / rois /
        width / height: as convert_rois; sizes: one (w, h) per box, positive and even; params: resize type (NEAREST / BILINEAR / BICUBIC; AREA is refused), pixel
        format, planes and normalization -- its width and height MUST be 0, the sizes are the boxes'.  Returns a LIST of tensors, box i's of
        output_shape(params, w_i, h_i): without `out` they are views into ONE allocation, each starting at a multiple of 256 bytes (so every box takes the vector
        stores); with `out`, a list of the caller's tensors, each contiguous and of its box's size, is filled (a tensor that is not 16-byte aligned takes the
        element-wise kernel; the call splits its boxes by that).  On torch's current stream.  Output i equals, bit for bit, convert_rois of box i alone at size i.
        dtype / mean / std (see tensor_spec): as convert_rois, through tsvpp_convert_rois_sized_tensor."""
        spec = tensor_spec(dtype, mean, std)
        p = params.parameters if isinstance(params, FrameParameters) else params
        ys, uvs, boxes = _normalize_rois(ys, uvs, rois)
        sizes = _normalize_sizes(sizes, len(boxes))
        widths, heights = _per_frame(width, len(ys)), _per_frame(height, len(ys))
        frames = (N.NV12 * len(ys))(*[self._frame(ys[i], uvs[i], widths[i], heights[i]) for i in range(len(ys))])
        n = len(boxes)
        if n == 0:
            raise RuntimeError("-3: convert_rois_sized needs at least one box")
        if out is None:
            tdt = _torch_dtype(spec) if spec is not None else (torch.float32 if p.normalization else torch.uint8)
            esz = torch.empty((), dtype=tdt).element_size()
            shapes = [output_shape(p, w, h) for (w, h) in sizes]
            offs, total = [], 0
            for sh in shapes:  # every box at a multiple of 256 bytes
                offs.append(total // esz)
                total += (int(np.prod(sh)) * esz + 255) // 256 * 256
            flat = torch.empty(max(total // esz, 1), dtype=tdt, device=f"cuda:{self.device}")
            out = [flat[o:o + int(np.prod(sh))].view(sh) for o, sh in zip(offs, shapes)]
        else:
            if len(out) != n:
                raise ValueError(f"{len(out)} outputs for {n} boxes")
            for i, (o, (w, h)) in enumerate(zip(out, sizes)):  # a tensor of another size would be written past its end
                need = self._lib.tsvpp_rois_sized_bytes(ctypes.byref(p), None if spec is None else ctypes.byref(spec), w, h)
                if need and o.numel() * o.element_size() != need:
                    raise ValueError(f"output {i} holds {o.numel() * o.element_size()} bytes, box {i} at {w} x {h} needs {need}")
        recs = (N.RoiSized * n)(*[N.RoiSized(*b, *s) for b, s in zip(boxes, sizes)])
        outs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in out])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if spec is None:
            N.check(self._lib.tsvpp_convert_rois_sized(self._ctx, len(ys), frames, n, recs, ctypes.byref(p), outs, stream))
        else:
            N.check(self._lib.tsvpp_convert_rois_sized_tensor(self._ctx, len(ys), frames, n, recs, ctypes.byref(p), ctypes.byref(spec), outs, stream))
        return out

    def convert_letterbox(self, ys, uvs, params, pad=(114, 128, 128), rects=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """The frame in front of a detector (tsvpp_convert_letterbox): every frame is resized with its aspect kept into an inner rectangle of ONE canvas of params'
        width x height, the rest of the canvas is `pad`, one launch per 32 frames.  ys / uvs: 3-D uint8 tensors (n, rows, pitch) or lists of 2-D tensors -- the
        frames may differ in size and pitch; pad: (Y, U, V), each 0..255 ((114, 128, 128): gray 114, (16, 128, 128): black); rects: one (left, top, width,
        height) per frame, all even and inside the canvas, or None for letterbox_rect's; width / height: the frames' picture size (an int for all frames or one per
        frame; default: the planes' own).  Returns (out, rects): `out` (filled, or allocated with convert_batch's padded frame stride) has shape (n, ...frame shape),
        on torch's current stream; `rects` is the list of (left, top, width, height) that was used, to map detections back.
        dtype / mean / std (see tensor_spec): with any of them given the canvases come out as what a network takes (tsvpp_convert_letterbox_tensor), the pad
        included: it goes through (x / 255 - mean[c]) * (1 / std[c]) like every sample."""
        return self._convert_letterbox(False, ys, uvs, params, pad, rects, out, width, height, tensor_spec(dtype, mean, std))

    def convert_letterbox_area(self, ys, uvs, params, pad=(114, 128, 128), rects=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """convert_letterbox for ResizeType.AREA (tsvpp_convert_letterbox_area), same arguments and result (out, rects): every frame with both ratios above 1 is
        averaged with the AREA down-scale -- the filter a 1080p or 4K frame into a 640 x 640 canvas should get, where BILINEAR point-samples --, any other frame
        takes AREA's up-scale rule.  The inner rectangle equals Convert(AREA) to the rectangle's size bit for bit; the weight rows are generated inside the kernel,
        so the call allocates and caches nothing and can be captured into a graph the first time it sees a scale.  Any other resize type is refused.
        dtype / mean / std: as convert_letterbox (the same entry point with a tensor spec)."""
        return self._convert_letterbox(True, ys, uvs, params, pad, rects, out, width, height, tensor_spec(dtype, mean, std))

    def _convert_letterbox(self, area, ys, uvs, params, pad, rects, out, width, height, spec):
        p = params.parameters if isinstance(params, FrameParameters) else params
        n = len(ys)
        if n == 0:
            raise RuntimeError("-3: convert_letterbox needs at least one frame")
        widths, heights = _per_frame(width, n), _per_frame(height, n)
        frames = (N.NV12 * n)(*[self._frame(ys[i], uvs[i], widths[i], heights[i]) for i in range(n)])
        if out is None:
            out = self._alloc_items(p, n, spec, "convert_letterbox needs an even, positive canvas size")
        recs = None if rects is None else _rects(rects, n)
        outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if area:
            N.check(self._lib.tsvpp_convert_letterbox_area(self._ctx, n, frames, ctypes.byref(p), None if spec is None else ctypes.byref(spec), recs, int(pad[0]),
                                                           int(pad[1]), int(pad[2]), outs, stream))
        elif spec is None:
            N.check(self._lib.tsvpp_convert_letterbox(self._ctx, n, frames, ctypes.byref(p), recs, int(pad[0]), int(pad[1]), int(pad[2]), outs, stream))
        else:
            N.check(self._lib.tsvpp_convert_letterbox_tensor(self._ctx, n, frames, ctypes.byref(p), ctypes.byref(spec), recs, int(pad[0]), int(pad[1]), int(pad[2]),
                                                             outs, stream))
        if recs is None:  # (the request was accepted: sizes are positive, the canvas is even)
            used = [letterbox_rect(frames[i].width, frames[i].height, p.dst_width, p.dst_height) for i in range(n)]
        else:
            used = [(r.left, r.top, r.width, r.height) for r in recs]
        return out, used

    def convert_warp(self, ys, uvs, warps, params, border=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """Rotated and affine-warped boxes behind a detector (tsvpp_convert_warp): every entry of `warps` samples its frame BILINEAR through its own 2 x 3
        output -> source matrix into params' width x height, colour-converted and stored to its own output, one launch per 32 outputs.  ys / uvs: as
        convert_rois (one frame as a pair of planes, or lists; the frames may differ in size and pitch); warps: (m0, m1, m2, m3, m4, m5) of frame 0 or
        (frame, m0, ..., m5) -- X = m0 u + m1 v + m2, Y = m3 u + m4 v + m5 with (u, v) = (column + 0.5, row + 0.5) the output pixel's centre, in luma pixels of
        the whole frame (warp_rotated_box, warp_from_opencv make them); border: None replicates the frame's edge, (Y, U, V), each 0..255, is the sample
        outside the frame.  params' resize_type must be BILINEAR.  Returns (or fills `out`, indexed out[i]) a tensor of shape (n, ...frame shape) with
        convert_batch's padded frame stride, on torch's current stream.  dtype / mean / std: as convert_rois (tsvpp_convert_warp_tensor); the border sample goes
        through them like every sample."""
        def items(p, ys, uvs):
            ys, uvs, recs = _normalize_warps(ys, uvs, warps)
            return ys, uvs, len(recs), (len(recs), recs)
        return self._convert_coord("convert_warp", "matrix", (self._lib.tsvpp_convert_warp, self._lib.tsvpp_convert_warp_tensor), items, ys, uvs, params, border, out,
                                   width, height, dtype, mean, std)

    def convert_remap(self, ys, uvs, maps, params, remaps=None, border=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """Per-pixel coordinate maps -- lens undistortion, rectification, unwraps, mesh warps (tsvpp_convert_remap): every output samples one frame BILINEAR where
        one map says, into params' width x height, colour-converted and stored to its own output, one launch per 32 outputs.  ys / uvs: as convert_rois (one frame
        as a pair of planes, or lists; the frames may differ in size and pitch).  maps: one CUDA float32 tensor (height, width, 2) of (x, y) source positions --
        OpenCV's remap convention, pixel k centred at k (remap_from_opencv, remap_from_grid make them) -- or a list of them; the last dimension is contiguous, a
        row stride of >= 2 * width elements becomes the pitch; each may be paired as (tensor, lds_bytes) with the hint of remap_lds_hint.  The tensors are read
        when the kernel runs: keep them alive, and a captured graph sees their updates.  remaps: a list of (frame, map); None with one map sends every frame
        through it in order, None with as many maps as frames pairs them up.  border, out, width, height, dtype / mean / std and the result: as convert_warp."""
        def items(p, ys, uvs):
            ys, uvs, _ = _normalize_rois(ys, uvs, [])
            recs_m = _normalize_maps(maps, p.dst_width, p.dst_height, self.device)
            recs = _normalize_remaps(remaps, len(ys), len(recs_m))
            return ys, uvs, len(recs), (len(recs_m), recs_m, len(recs), recs)
        return self._convert_coord("convert_remap", None, (self._lib.tsvpp_convert_remap, self._lib.tsvpp_convert_remap_tensor), items, ys, uvs, params, border, out,
                                   width, height, dtype, mean, std)

    def convert_mesh(self, ys, uvs, meshes, params, cell=(16, 16), remaps=None, border=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """Sparse control-grid warps -- a warp mesh per lens, per stabilised frame (tsvpp_convert_mesh): convert_remap with the coordinate interpolated from one
        control point per cell of cw x ch output pixels instead of read per pixel; bit for bit convert_remap of mesh_expand(mesh).  meshes: one CUDA float32 tensor
        (rows, cols, 2) of (x, y) source positions, (rows, cols) = mesh_dims(width, height, cell) -- control point (r, c) belongs to output pixel (r * ch, c * cw),
        index-based as a dense map's entry (mesh_from_map, mesh_undistort make them) -- or a list of them; the last dimension is contiguous, a row stride of
        >= 2 * cols elements becomes the pitch; each may be paired as (tensor, lds_bytes) with the hint of mesh_lds_hint.  cell: (cw, ch), powers of two 4..256,
        for all meshes or a list with one per mesh.  The tensors are read when the kernel runs: keep them alive, and a captured graph sees their updates.
        remaps: a list of (frame, mesh), None as for convert_remap.  Everything else: as convert_remap."""
        def items(p, ys, uvs):
            ys, uvs, _ = _normalize_rois(ys, uvs, [])
            recs_m = _normalize_meshes(meshes, cell, p.dst_width, p.dst_height, self.device)
            recs = _normalize_remaps(remaps, len(ys), len(recs_m))
            return ys, uvs, len(recs), (len(recs_m), recs_m, len(recs), recs)
        return self._convert_coord("convert_mesh", None, (self._lib.tsvpp_convert_mesh, self._lib.tsvpp_convert_mesh_tensor), items, ys, uvs, params, border, out,
                                   width, height, dtype, mean, std)

    def convert_perspective(self, ys, uvs, persps, params, border=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """Homography-warped outputs (tsvpp_convert_perspective): every entry of `persps` samples its frame BILINEAR through its own 3 x 3 output -> source
        homography into params' width x height, colour-converted and stored to its own output, one launch per 32 outputs.  ys / uvs, border, out, width, height,
        dtype / mean / std: as convert_warp.  persps: (h0, ..., h8) of frame 0 or (frame, h0, ..., h8), row-major -- X = (h0 u + h1 v + h2) / (h6 u + h7 v + h8),
        Y = (h3 u + h4 v + h5) / (h6 u + h7 v + h8) with (u, v) = (column + 0.5, row + 0.5) the output pixel's centre, in luma pixels of the whole frame
        (perspective_from_quad, perspective_from_opencv make them).  A homography whose horizon crosses the output is refused (-2)."""
        def items(p, ys, uvs):
            ys, uvs, recs = _normalize_persps(ys, uvs, persps)
            return ys, uvs, len(recs), (len(recs), recs)
        return self._convert_coord("convert_perspective", "homography", (self._lib.tsvpp_convert_perspective, self._lib.tsvpp_convert_perspective_tensor), items, ys,
                                   uvs, params, border, out, width, height, dtype, mean, std)

    def convert_warp_bicubic(self, ys, uvs, warps, params, border=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """convert_warp sampled with the library's BICUBIC (tsvpp_convert_warp_bicubic): the coordinate is convert_warp's bit for bit, the 4 x 4 taps follow the
        reference's edge rule and the sums are Convert(BICUBIC)'s -- the scale-only matrix gives Convert(BICUBIC) of the whole frame bit for bit.  params'
        resize_type must be BICUBIC; every argument and the result: as convert_warp (dtype / mean / std: the same entry point with a spec)."""
        def items(p, ys, uvs):
            ys, uvs, recs = _normalize_warps(ys, uvs, warps)
            return ys, uvs, len(recs), (len(recs), recs)
        return self._convert_coord("convert_warp_bicubic", "matrix", _convert_pair(self._lib.tsvpp_convert_warp_bicubic), items, ys, uvs, params, border, out, width,
                                   height, dtype, mean, std)

    def convert_perspective_bicubic(self, ys, uvs, persps, params, border=None, out=None, width=None, height=None, dtype=None, mean=None, std=None):
        """convert_perspective sampled with the library's BICUBIC (tsvpp_convert_perspective_bicubic): the coordinate is convert_perspective's bit for bit, the
        sample convert_warp_bicubic's -- a homography with last row (0, 0, 1) gives that call's bits.  params' resize_type must be BICUBIC; every argument and the
        result: as convert_perspective."""
        def items(p, ys, uvs):
            ys, uvs, recs = _normalize_persps(ys, uvs, persps)
            return ys, uvs, len(recs), (len(recs), recs)
        return self._convert_coord("convert_perspective_bicubic", "homography", _convert_pair(self._lib.tsvpp_convert_perspective_bicubic), items, ys, uvs, params,
                                   border, out, width, height, dtype, mean, std)

    def _convert_coord(self, name, one, entries, items, ys, uvs, params, border, out, width, height, dtype, mean, std):
        """convert_warp, convert_perspective, convert_remap and convert_mesh, once.  entries: the call's (colour, tensor) entry points; items(p, ys, uvs): the
        path's own arguments as (luma planes, chroma planes, number of outputs, the arguments that sit between `frames` and `params` in the C call); one: what an
        empty call lacks ("matrix"), None where items() has said so already."""
        spec = tensor_spec(dtype, mean, std)
        p = params.parameters if isinstance(params, FrameParameters) else params
        ys, uvs, n, between = items(p, ys, uvs)
        widths, heights = _per_frame(width, len(ys)), _per_frame(height, len(ys))
        frames = (N.NV12 * len(ys))(*[self._frame(ys[i], uvs[i], widths[i], heights[i]) for i in range(len(ys))])
        if n == 0 and one is not None:
            raise RuntimeError(f"-3: {name} needs at least one {one}")
        if out is None:
            out = self._alloc_items(p, n, spec, f"{name} needs an even, positive output size")
        by, bu, bv = _border(border)
        outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if spec is None:
            N.check(entries[0](self._ctx, len(ys), frames, *between, ctypes.byref(p), by, bu, bv, outs, stream))
        else:
            N.check(entries[1](self._ctx, len(ys), frames, *between, ctypes.byref(p), ctypes.byref(spec), by, bu, bv, outs, stream))
        return out

    def make_batch(self, ys, uvs, params, out=None, width=None, height=None):
        """Pre-builds the descriptor arrays of a batch (the per-frame structs are built once, not per
        call): returns a handle for run_batch().  Keeps the tensors alive."""
        p = params.parameters if isinstance(params, FrameParameters) else params
        n = len(ys)
        frames = (N.NV12 * n)(*[self._frame(ys[i], uvs[i], width, height) for i in range(n)])
        if out is None:
            out = self._alloc(p, frames[0].width, frames[0].height, n)
        outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
        return {"n": n, "frames": frames, "outs": outs, "params": p, "out": out, "keep": (ys, uvs)}

    def run_batch(self, batch, stream=None):
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self._lib.tsvpp_convert_batch(self._ctx, batch["n"], batch["frames"], ctypes.byref(batch["params"]),
                                              batch["outs"], stream))
        return batch["out"]

    def make_table(self, ys, uvs, params, out=None, width=None, height=None):
        """A persistent, device-resident frame table (tsvpp_table_*, include/tsvpp.h) over a POOL of input frames and output tensors: registered once, any
        run of its entries is then converted by run_table() with launches of up to 1024 frames and no per-call pointer traffic.  ys / uvs / out as for
        convert_batch; the handle keeps the tensors alive; free_table() (or Close) releases the table."""
        p = params.parameters if isinstance(params, FrameParameters) else params
        n = len(ys)
        frames = (N.NV12 * n)(*[self._frame(ys[i], uvs[i], width, height) for i in range(n)])
        if out is None:
            out = self._alloc(p, frames[0].width, frames[0].height, n)
        outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
        h = ctypes.c_void_p()
        N.check(self._lib.tsvpp_table_create(self._ctx, n, ctypes.byref(h)))
        self._tables.append(h)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self._lib.tsvpp_table_set(h, 0, n, frames, outs, stream))
        return {"n": n, "handle": h, "params": p, "out": out, "keep": (ys, uvs), "width": frames[0].width}

    def run_table(self, table, first=0, n=None, params=None, stream=None):
        """Converts entries [first, first + n) of a table made by make_table (default: all of it, with the parameters it was made with)."""
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        p = table["params"] if params is None else (params.parameters if isinstance(params, FrameParameters) else params)
        cnt = table["n"] - first if n is None else n
        if params is not None:
            #  the table's output tensors were allocated for the parameters it was made with and their addresses live in the device table: other
            # parameters are fine only while every frame still fits its registered output
            y0 = table["keep"][0][0]
            w = table.get("width") or y0.shape[1]
            need = int(self._lib.tsvpp_out_bytes(ctypes.byref(p), int(w), int(y0.shape[0])))
            have = table["out"][0].numel() * table["out"].element_size()
            if need == 0 or need > have:
                raise RuntimeError(f"-3: run_table(params=...) needs {need} bytes per frame, the table's outputs hold {have}")
        N.check(self._lib.tsvpp_convert_table(self._ctx, table["handle"], first, cnt, ctypes.byref(p), stream))
        return table["out"]

    def free_table(self, table):
        h = table.get("handle")
        if h is not None and any(h is t for t in self._tables):
            torch.cuda.synchronize(self.device)
            self._lib.tsvpp_table_destroy(h)
            self._tables = [t for t in self._tables if t is not h]
            table["handle"] = None

    def trim(self):
        """Releases the memory the context has retired (geometry tables pushed out of its cache, outgrown scratch buffers): tsvpp_trim.  Synchronises the device
        first -- the C call itself leaves that to the caller."""
        torch.cuda.synchronize(self.device)
        n = ctypes.c_size_t(0)
        N.check(self._lib.tsvpp_trim(self._ctx, ctypes.byref(n)))
        return int(n.value)

    def _on_consumer_stream(self, name):
        raw = self.consumer_stream(name)
        ext = torch.cuda.ExternalStream(raw, device=self.device)
        ext.wait_stream(torch.cuda.current_stream(self.device))
        return raw, ext

    def get_coeffs(self):
        c = N.Coeffs()
        N.check(self._lib.tsvpp_get_coeffs(self._ctx, ctypes.byref(c)))
        return [getattr(c, f[0]) for f in N.Coeffs._fields_]

    def set_coeffs(self, values):
        c = N.Coeffs(*[float(v) for v in values])
        N.check(self._lib.tsvpp_set_coeffs(self._ctx, ctypes.byref(c)))


def _parse_selection(text):
    out = {}
    for item in text.split(" "):
        k, _, v = item.partition("=")
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


def describe(params, in_w, in_h, pitch=0, n_frames=64, aligned_outputs=True, pitch_uv=None):
    """What a convert_batch of this request would launch (stage selection, kernel, workgroup shape, LDS bytes, grid)
    as a dict -- host logic only, works without a GPU (tsvpp_describe).  `pitch_uv`: the chroma pitch (default: `pitch`)."""
    p = params.parameters if isinstance(params, FrameParameters) else params
    buf = ctypes.create_string_buffer(512)
    puv = pitch if pitch_uv is None else pitch_uv
    N.check(N.lib().tsvpp_describe(ctypes.byref(p), in_w, in_h, pitch, puv, n_frames, 1 if aligned_outputs else 0, buf, len(buf)))
    return _parse_selection(buf.value.decode())


def _per_frame(value, n):
    if value is None or isinstance(value, int):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{len(value)} sizes for {n} frames")
    return value


def _normalize_rois(ys, uvs, rois):
    """The argument forms of convert_rois / describe_rois as (list of luma planes, list of chroma planes, list of (frame, left, top, right, bottom)):
    one frame may be given as a bare pair of planes, a box of frame 0 as a 4-tuple.  Pure Python: touches no device."""
    if not isinstance(ys, (list, tuple)):
        ys, uvs = [ys], [uvs]
    elif isinstance(uvs, (list, tuple)):
        ys, uvs = list(ys), list(uvs)
    else:
        raise ValueError("ys is a list of planes but uvs is not")
    if len(ys) != len(uvs) or not ys:
        raise ValueError(f"{len(ys)} luma planes and {len(uvs)} chroma planes")
    boxes = []
    for b in rois:
        b = tuple(int(v) for v in b)
        if len(b) == 4:
            b = (0,) + b
        if len(b) != 5:
            raise ValueError(f"a box is (left, top, right, bottom) or (frame, left, top, right, bottom), not {b}")
        boxes.append(b)
    return ys, uvs, boxes


def describe_rois(params, frames, rois, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_rois of this request would launch, as a dict (tsvpp_describe_rois: mode, out, rois, launches, kernel, grid, lds, staged, ...) -- host logic
    only, works without a GPU.  frames: (width, height) or (width, height, pitch) or (width, height, pitch_y, pitch_uv), one or a list; rois as for convert_rois.
    dtype / mean / std: as convert_rois (tsvpp_describe_rois_tensor: out= names the element, kernel= the tensor instantiation)."""
    return _describe_rois(N.lib().tsvpp_describe_rois, params, frames, rois, aligned_outputs, tensor_spec(dtype, mean, std))


def describe_rois_area(params, frames, rois, aligned_outputs=True, dtype=None, mean=None, std=None):
    """describe_rois for convert_rois_area (tsvpp_describe_rois_area): the same keys, then down (boxes on the down-scale path) and taps ("<x>x<y>", the largest)."""
    return _describe_rois(N.lib().tsvpp_describe_rois_area, params, frames, rois, aligned_outputs, tensor_spec(dtype, mean, std))


def _normalize_sizes(sizes, n):
    sizes = [tuple(int(v) for v in s) for s in sizes]
    if len(sizes) != n or any(len(s) != 2 for s in sizes):
        raise ValueError(f"{n} boxes need {n} sizes (width, height)")
    return sizes


def describe_rois_sized(params, frames, rois, sizes, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_rois_sized of this request would launch, as a dict (tsvpp_describe_rois_sized: mode, out, dst="var", rois, frames, launches, kernel, shape,
    lds, grid, sizes, maxdst, staged, vec, nt, limit) -- host logic only, works without a GPU.  frames: as describe_rois; rois / sizes: as convert_rois_sized;
    aligned_outputs: every output 16-byte aligned (what convert_rois_sized allocates) or none.  dtype / mean / std: the tensor form."""
    spec = tensor_spec(dtype, mean, std)
    p = params.parameters if isinstance(params, FrameParameters) else params
    recs = _geometry_records(frames)
    _, _, boxes = _normalize_rois([None] * len(recs), [None] * len(recs), rois)
    sizes = _normalize_sizes(sizes, len(boxes))
    fr = (N.NV12 * len(recs))(*recs)
    bx = (N.RoiSized * max(len(boxes), 1))(*[N.RoiSized(*b, *s) for b, s in zip(boxes, sizes)])
    buf = ctypes.create_string_buffer(512)
    if spec is None:
        N.check(N.lib().tsvpp_describe_rois_sized(ctypes.byref(p), len(recs), fr, len(boxes), bx, 1 if aligned_outputs else 0, buf, len(buf)))
    else:
        N.check(N.lib().tsvpp_describe_rois_sized_tensor(ctypes.byref(p), ctypes.byref(spec), len(recs), fr, len(boxes), bx, 1 if aligned_outputs else 0, buf, len(buf)))
    return _parse_selection(buf.value.decode())


def sizes_for_height(boxes, height, max_width=None, multiple=2):
    """Output sizes for text lines (convert_rois_sized): every box goes to `height` rows and to the width that keeps its aspect, rounded to the nearest multiple
    of `multiple` (m, even; ties go up) and at least m.  boxes: (left, top, right, bottom) or (frame, left, top, right, bottom).  Integers only, with
    bw = right - left and bh = bottom - top:
        w = m * max(1, (2 * bw * height + bh * m) // (2 * bh * m))
    clipped to `max_width` rounded down to a multiple of m (if given).  Returns a list of (w, height).  A 200 x 40 box to height 32, m = 2:
    (2 * 200 * 32 + 40 * 2) // (2 * 40 * 2) = 12880 // 160 = 80, w = 160."""
    m, height = int(multiple), int(height)
    if m <= 0 or m & 1:
        raise ValueError(f"multiple must be positive and even, not {multiple}")
    cap = None if max_width is None else int(max_width) // m * m
    if cap is not None and cap < m:
        raise ValueError(f"max_width {max_width} is below the multiple {m}")
    out = []
    for b in boxes:
        b = tuple(int(v) for v in b)[-4:]
        bw, bh = b[2] - b[0], b[3] - b[1]
        if bw <= 0 or bh <= 0:
            raise ValueError(f"empty box {b}")
        w = m * max(1, (2 * bw * height + bh * m) // (2 * bh * m))
        out.append((w if cap is None else min(w, cap), height))
    return out


def pyramid_sizes(w, h, levels):
    """The sizes of a dyadic pyramid or preview ladder (convert_rois_sized with the whole frame as every box): level k is
        (max(2, (w >> k) & ~1), max(2, (h >> k) & ~1))
    for k = 0 .. levels - 1; level 0 is the frame's own size rounded down to even.  pyramid_sizes(1920, 1080, 4) = [(1920, 1080), (960, 540), (480, 270), (240, 134)]."""
    return [(max(2, (int(w) >> k) & ~1), max(2, (int(h) >> k) & ~1)) for k in range(int(levels))]


def _geometry_records(frames):
    """The frames argument of the describe functions -- (width, height), (width, height, pitch) or (width, height, pitch_y, pitch_uv), one or a list -- as NV12
    records without planes."""
    if frames and isinstance(frames[0], int):
        frames = [frames]
    recs = []
    for f in frames:
        f = tuple(int(v) for v in f)
        py = f[2] if len(f) > 2 else 0
        recs.append(N.NV12(None, None, py, f[3] if len(f) > 3 else py, f[0], f[1]))
    return recs


def _describe_rois(entry, params, frames, rois, aligned_outputs, spec=None):
    p = params.parameters if isinstance(params, FrameParameters) else params
    recs = _geometry_records(frames)
    _, _, boxes = _normalize_rois([None] * len(recs), [None] * len(recs), rois)
    fr = (N.NV12 * len(recs))(*recs)
    bx = (N.Roi * max(len(boxes), 1))(*[N.Roi(*b) for b in boxes])
    buf = ctypes.create_string_buffer(512)
    if spec is None:
        N.check(entry(ctypes.byref(p), len(recs), fr, len(boxes), bx, 1 if aligned_outputs else 0, buf, len(buf)))
    else:
        N.check(N.lib().tsvpp_describe_rois_tensor(ctypes.byref(p), ctypes.byref(spec), len(recs), fr, len(boxes), bx, 1 if aligned_outputs else 0, buf, len(buf)))
    return _parse_selection(buf.value.decode())


def _rects(rects, n):
    rects = [tuple(int(v) for v in r) for r in rects]
    if len(rects) != n or any(len(r) != 4 for r in rects):
        raise ValueError(f"{n} frames need {n} rectangles (left, top, width, height)")
    return (N.Rect * n)(*[N.Rect(*r) for r in rects])


def letterbox_rect(in_w, in_h, dst_w, dst_h):
    """The default inner rectangle (left, top, width, height) of an in_w x in_h frame in a dst_w x dst_h canvas (tsvpp_letterbox_rect): integer arithmetic only."""
    r = N.Rect()
    N.check(N.lib().tsvpp_letterbox_rect(int(in_w), int(in_h), int(dst_w), int(dst_h), ctypes.byref(r)))
    return (r.left, r.top, r.width, r.height)


def describe_letterbox(params, frames, rects=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_letterbox of this request would launch, as a dict (tsvpp_describe_letterbox: describe_rois's keys, then inner = "WxH+left+top" of the first
    frame) -- host logic only, works without a GPU.  frames: (width, height) or (width, height, pitch) or (width, height, pitch_y, pitch_uv), one or a list."""
    p = params.parameters if isinstance(params, FrameParameters) else params
    recs = _geometry_records(frames)
    fr = (N.NV12 * max(len(recs), 1))(*recs)
    rc = None if rects is None else _rects(rects, len(recs))
    buf = ctypes.create_string_buffer(512)
    spec = tensor_spec(dtype, mean, std)  # (tsvpp_describe_letterbox_tensor: out= names the element, kernel= the tensor instantiation)
    if spec is None:
        N.check(N.lib().tsvpp_describe_letterbox(ctypes.byref(p), len(recs), fr, rc, 1 if aligned_outputs else 0, buf, len(buf)))
    else:
        N.check(N.lib().tsvpp_describe_letterbox_tensor(ctypes.byref(p), ctypes.byref(spec), len(recs), fr, rc, 1 if aligned_outputs else 0, buf, len(buf)))
    return _parse_selection(buf.value.decode())


def describe_letterbox_area(params, frames, rects=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_letterbox_area of this request would launch, as a dict (tsvpp_describe_letterbox_area: describe_letterbox's keys, then down = frames on the
    down-scale path, taps = "XxY" and chain = the most generator steps a chain of the first launch runs in front of its tile) -- host logic only, works without
    a GPU.  Arguments as describe_letterbox."""
    p = params.parameters if isinstance(params, FrameParameters) else params
    recs = _geometry_records(frames)
    fr = (N.NV12 * max(len(recs), 1))(*recs)
    rc = None if rects is None else _rects(rects, len(recs))
    buf = ctypes.create_string_buffer(512)
    spec = tensor_spec(dtype, mean, std)
    N.check(N.lib().tsvpp_describe_letterbox_area(ctypes.byref(p), None if spec is None else ctypes.byref(spec), len(recs), fr, rc, 1 if aligned_outputs else 0, buf,
                                                  len(buf)))
    return _parse_selection(buf.value.decode())


def _border(border):
    """border=None: replicate (-1, -1, -1); else (Y, U, V)"""
    if border is None:
        return -1, -1, -1
    y, u, v = (int(c) for c in border)
    return y, u, v


def _convert_pair(entry):
    """An entry point whose `spec` may be null (tsvpp_convert_warp_bicubic) as _convert_coord's (colour, tensor) pair: the colour form passes no spec.  The spec
    sits behind `params`, in front of the last five arguments."""
    return (lambda *a: entry(*a[:-5], None, *a[-5:])), entry


def _describe_pair(entry):
    """... and a describe call of that kind as _describe_coord's pair: the spec sits behind `params`, the first argument"""
    return (lambda p, *a: entry(p, None, *a)), entry


def _describe_coord(entries, items, params, frames, border, aligned_outputs, dtype, mean, std):
    """describe_warp, describe_perspective, describe_remap and describe_mesh, once.  entries: the call's (colour, tensor) entry points; items(p, frame records):
    the arguments that sit between `frames` and the border in the C call."""
    p = params.parameters if isinstance(params, FrameParameters) else params
    recs = _geometry_records(frames)
    between = items(p, recs)
    fr = (N.NV12 * len(recs))(*recs)
    by, bu, bv = _border(border)
    buf = ctypes.create_string_buffer(512)
    spec = tensor_spec(dtype, mean, std)
    if spec is None:
        N.check(entries[0](ctypes.byref(p), len(recs), fr, *between, by, bu, bv, 1 if aligned_outputs else 0, buf, len(buf)))
    else:
        N.check(entries[1](ctypes.byref(p), ctypes.byref(spec), len(recs), fr, *between, by, bu, bv, 1 if aligned_outputs else 0, buf, len(buf)))
    return _parse_selection(buf.value.decode())


def _normalize_warps(ys, uvs, warps):
    """The argument forms of convert_warp / describe_warp as (list of luma planes, list of chroma planes, array of tsvpp_warp): one frame may be given as a bare
    pair of planes, a matrix of frame 0 as six numbers.  Pure Python: touches no device."""
    ys, uvs, _ = _normalize_rois(ys, uvs, [])
    recs = []
    for w in warps:
        w = tuple(w)
        if len(w) == 6:
            w = (0,) + w
        if len(w) != 7:
            raise ValueError(f"a warp is (m0, ..., m5) or (frame, m0, ..., m5), not {w}")
        recs.append(N.Warp(int(w[0]), (ctypes.c_float * 6)(*[float(v) for v in w[1:]])))
    return ys, uvs, (N.Warp * max(len(recs), 1))(*recs) if recs else []


def describe_warp(params, frames, warps, border=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_warp of this request would launch, as a dict (tsvpp_describe_warp: describe_rois's keys with warps= for rois=, then border = "replicate" or
    "Y,U,V") -- host logic only, works without a GPU.  frames: as describe_rois; warps and border as for convert_warp."""
    def items(p, recs):
        _, _, ws = _normalize_warps([None] * len(recs), [None] * len(recs), warps)
        return len(ws), ws or None
    return _describe_coord((N.lib().tsvpp_describe_warp, N.lib().tsvpp_describe_warp_tensor), items, params, frames, border, aligned_outputs, dtype, mean, std)


def describe_warp_bicubic(params, frames, warps, border=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_warp_bicubic of this request would launch, as a dict (tsvpp_describe_warp_bicubic: describe_warp's keys, mode warp_bicubic) -- host logic
    only, works without a GPU.  Arguments as describe_warp."""
    def items(p, recs):
        _, _, ws = _normalize_warps([None] * len(recs), [None] * len(recs), warps)
        return len(ws), ws or None
    return _describe_coord(_describe_pair(N.lib().tsvpp_describe_warp_bicubic), items, params, frames, border, aligned_outputs, dtype, mean, std)


def warp_rotated_box(cx, cy, box_w, box_h, angle_rad, dst_w, dst_h):
    """The matrix (m0, ..., m5), as float32 values, that maps a dst_w x dst_h output onto the box of box_w x box_h luma pixels centred at (cx, cy) and rotated
    by angle_rad, clockwise on screen (tsvpp_warp_rotated_box: evaluated in double, each entry rounded once)."""
    w = N.Warp()
    N.check(N.lib().tsvpp_warp_rotated_box(float(cx), float(cy), float(box_w), float(box_h), float(angle_rad), int(dst_w), int(dst_h), ctypes.byref(w)))
    return tuple(w.m)


def warp_from_opencv(M):
    """OpenCV's index-based inverse matrix [[a, b, c], [d, e, f]] (output index -> source index: what cv2.warpAffine takes with WARP_INVERSE_MAP, or
    cv2.invertAffineTransform of the forward one) as this library's centre-based (m0, ..., m5): m2 = c + 0.5 - 0.5 (a + b), m5 = f + 0.5 - 0.5 (d + e)."""
    (a, b, c), (d, e, f) = [[float(v) for v in row] for row in M]
    return (a, b, c + 0.5 - 0.5 * (a + b), d, e, f + 0.5 - 0.5 * (d + e))


def _normalize_persps(ys, uvs, persps):
    """_normalize_warps for convert_perspective / describe_perspective: a homography of frame 0 is nine numbers"""
    ys, uvs, _ = _normalize_rois(ys, uvs, [])
    recs = []
    for q in persps:
        q = tuple(q)
        if len(q) == 9:
            q = (0,) + q
        if len(q) != 10:
            raise ValueError(f"a homography is (h0, ..., h8) or (frame, h0, ..., h8), not {q}")
        recs.append(N.Persp(int(q[0]), (ctypes.c_float * 9)(*[float(v) for v in q[1:]])))
    return ys, uvs, (N.Persp * max(len(recs), 1))(*recs) if recs else []


def describe_perspective(params, frames, persps, border=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_perspective of this request would launch, as a dict (tsvpp_describe_perspective: describe_warp's keys, mode persp_bilinear) -- host logic
    only, works without a GPU.  frames: as describe_rois; persps and border as for convert_perspective."""
    def items(p, recs):
        _, _, qs = _normalize_persps([None] * len(recs), [None] * len(recs), persps)
        return len(qs), qs or None
    return _describe_coord((N.lib().tsvpp_describe_perspective, N.lib().tsvpp_describe_perspective_tensor), items, params, frames, border, aligned_outputs, dtype, mean,
                           std)


def describe_perspective_bicubic(params, frames, persps, border=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_perspective_bicubic of this request would launch, as a dict (tsvpp_describe_perspective_bicubic: describe_perspective's keys, mode
    persp_bicubic) -- host logic only, works without a GPU.  Arguments as describe_perspective."""
    def items(p, recs):
        _, _, qs = _normalize_persps([None] * len(recs), [None] * len(recs), persps)
        return len(qs), qs or None
    return _describe_coord(_describe_pair(N.lib().tsvpp_describe_perspective_bicubic), items, params, frames, border, aligned_outputs, dtype, mean, std)


def perspective_from_quad(quad, dst_w, dst_h):
    """The homography (h0, ..., h8), as float32 values, that maps the corners of a dst_w x dst_h output onto the source points quad = [(x0, y0), (x1, y1), (x2, y2),
    (x3, y3)] (or eight numbers), top-left, top-right, bottom-right, bottom-left, in luma pixels (tsvpp_persp_from_quad: Heckbert's closed form in double, each
    entry rounded once).  Whether it is usable -- a convex quad, the horizon off the output -- is convert_perspective's decision."""
    flat = [float(v) for pt in quad for v in (pt if hasattr(pt, "__len__") else (pt,))]
    if len(flat) != 8:
        raise ValueError(f"a quad is four points, not {quad}")
    q = N.Persp()
    N.check(N.lib().tsvpp_persp_from_quad((ctypes.c_double * 8)(*flat), int(dst_w), int(dst_h), ctypes.byref(q)))
    return tuple(q.h)


def perspective_from_opencv(M):
    """OpenCV's index-based inverse matrix [[a, b, c], [d, e, f], [g, h, k]] (output index -> source index: what cv2.warpPerspective takes with WARP_INVERSE_MAP)
    as this library's centre-based (h0, ..., h8): with k' = k - 0.5 (g + h), rows (a + 0.5 g, b + 0.5 h, c - 0.5 (a + b) + 0.5 k'),
    (d + 0.5 g, e + 0.5 h, f - 0.5 (d + e) + 0.5 k'), (g, h, k').  With last row (0, 0, 1) this is warp_from_opencv."""
    (a, b, c), (d, e, f), (g, h, k) = [[float(v) for v in row] for row in M]
    k2 = k - 0.5 * (g + h)
    return (a + 0.5 * g, b + 0.5 * h, c - 0.5 * (a + b) + 0.5 * k2, d + 0.5 * g, e + 0.5 * h, f - 0.5 * (d + e) + 0.5 * k2, g, h, k2)


def _normalize_maps(maps, dst_w, dst_h, device=None):
    """The maps argument of convert_remap / describe_remap as an array of tsvpp_map.  A map is a CUDA float32 tensor (dst_h, dst_w, 2) whose last dimension is
    contiguous (device given: convert_remap), optionally paired as (tensor, lds_bytes); without a device (describe_remap) it may also be (pitch, lds_bytes)
    integers.  Anything else raises ValueError: nothing reaches the C call."""
    if isinstance(maps, torch.Tensor) or (isinstance(maps, tuple) and len(maps) == 2 and not isinstance(maps[1], (torch.Tensor, tuple, list))):
        maps = [maps]
    recs = []
    for m in maps:
        hint = 0
        if isinstance(m, (tuple, list)):
            if len(m) != 2:
                raise ValueError(f"a map is a tensor, (tensor, lds_bytes) or (pitch, lds_bytes), not {m}")
            m, hint = m[0], int(m[1])
        if not isinstance(m, torch.Tensor):
            if device is not None:
                raise ValueError(f"convert_remap needs its maps as tensors, not {type(m).__name__}")
            recs.append(N.Map(None, int(m), hint))
            continue
        if m.dtype != torch.float32:
            raise ValueError(f"a map is a float32 tensor, not {m.dtype}")
        if m.dim() != 3 or tuple(m.shape) != (dst_h, dst_w, 2):
            raise ValueError(f"a map for a {dst_w} x {dst_h} output has shape ({dst_h}, {dst_w}, 2), not {tuple(m.shape)}")
        if m.stride(2) != 1 or m.stride(1) != 2 or m.stride(0) < 2 * dst_w:
            raise ValueError(f"a map's last two dimensions are contiguous and its row stride is at least {2 * dst_w} elements: strides {tuple(m.stride())}")
        if device is not None and (not m.is_cuda or m.device.index != device):
            raise ValueError(f"a map lives on cuda:{device}, not on {m.device}")
        recs.append(N.Map(m.data_ptr() if m.is_cuda else None, 4 * m.stride(0), hint))
    if not recs:
        raise ValueError("at least one map is needed")
    return (N.Map * len(recs))(*recs)


def _normalize_remaps(remaps, n_frames, n_maps):
    """The remaps argument of convert_remap / describe_remap as an array of tsvpp_remap: (frame, map) pairs; None with one map sends every frame through it in
    order, None with as many maps as frames pairs them up."""
    if remaps is None:
        if n_maps == 1:
            remaps = [(f, 0) for f in range(n_frames)]
        elif n_maps == n_frames:
            remaps = [(f, f) for f in range(n_frames)]
        else:
            raise ValueError(f"{n_frames} frames and {n_maps} maps do not pair up: say which with remaps=[(frame, map), ...]")
    pairs = []
    for r in remaps:
        r = tuple(int(v) for v in r)
        if len(r) != 2:
            raise ValueError(f"a remap is (frame, map), not {r}")
        pairs.append(r)
    if not pairs:
        raise ValueError("at least one (frame, map) is needed")
    return (N.Remap * len(pairs))(*[N.Remap(*r) for r in pairs])


def describe_remap(params, frames, maps, remaps=None, border=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_remap of this request would launch, as a dict (tsvpp_describe_remap: describe_warp's keys with remaps= and maps= for warps= and without
    staged=, which the host cannot know; lds is the launch's dynamic LDS) -- host logic only, works without a GPU.  frames: as describe_rois; maps: as for
    convert_remap (tensors on any device: only strides and hints are read) or (pitch, lds_bytes) integers; remaps and border as for convert_remap."""
    def items(p, recs):
        ms = _normalize_maps(maps, p.dst_width, p.dst_height)
        rs = _normalize_remaps(remaps, len(recs), len(ms))
        return len(ms), ms, len(rs), rs
    return _describe_coord((N.lib().tsvpp_describe_remap, N.lib().tsvpp_describe_remap_tensor), items, params, frames, border, aligned_outputs, dtype, mean, std)


def remap_from_opencv(map_x, map_y):
    """OpenCV's pair of (H, W) maps (what cv2.initUndistortRectifyMap returns as CV_32FC1, what cv2.remap takes) as one (H, W, 2) float32 map of convert_remap:
    [..., 0] = x, [..., 1] = y.  OpenCV's convention is the contract's -- no arithmetic.  numpy arrays give a numpy array, tensors a tensor on their device."""
    if isinstance(map_x, torch.Tensor) or isinstance(map_y, torch.Tensor):
        map_x, map_y = torch.as_tensor(map_x), torch.as_tensor(map_y)
        if map_x.dim() != 2 or map_x.shape != map_y.shape:
            raise ValueError(f"map_x and map_y are (H, W) and alike, not {tuple(map_x.shape)} and {tuple(map_y.shape)}")
        return torch.stack((map_x.to(torch.float32), map_y.to(device=map_x.device, dtype=torch.float32)), dim=-1).contiguous()
    map_x, map_y = np.asarray(map_x, dtype=np.float32), np.asarray(map_y, dtype=np.float32)
    if map_x.ndim != 2 or map_x.shape != map_y.shape:
        raise ValueError(f"map_x and map_y are (H, W) and alike, not {map_x.shape} and {map_y.shape}")
    return np.ascontiguousarray(np.stack((map_x, map_y), axis=-1))


def remap_from_grid(grid, w, h):
    """A torch.nn.functional.grid_sample grid (H, W, 2) with align_corners=False, for a source of w x h pixels, as a map of convert_remap, in fp32 and in this
    operation order: x = ((gx + 1) * w - 1) * 0.5, y = ((gy + 1) * h - 1) * 0.5.  numpy arrays give a numpy array, tensors a tensor on their device."""
    if isinstance(grid, torch.Tensor):
        g = grid.to(torch.float32)
        if g.dim() != 3 or g.shape[2] != 2:
            raise ValueError(f"a grid is (H, W, 2), not {tuple(g.shape)}")
        return torch.stack((((g[..., 0] + 1.0) * float(w) - 1.0) * 0.5, ((g[..., 1] + 1.0) * float(h) - 1.0) * 0.5), dim=-1).contiguous()
    g = np.asarray(grid, dtype=np.float32)
    if g.ndim != 3 or g.shape[2] != 2:
        raise ValueError(f"a grid is (H, W, 2), not {g.shape}")
    one, half = np.float32(1.0), np.float32(0.5)
    return np.ascontiguousarray(np.stack((((g[..., 0] + one) * np.float32(w) - one) * half, ((g[..., 1] + one) * np.float32(h) - one) * half), axis=-1))


def remap_lds_hint(map, frame_w, frame_h, luma_only=False):
    """The LDS hint of a map on a frame_w x frame_h frame (tsvpp_remap_lds_need): the largest staging need, in bytes, over all of its 32 x 32 tiles -- what
    convert_remap takes as (tensor, lds_bytes).  Copies the map to the host once; luma_only: for Y800 outputs.  map: a tensor or array (H, W, 2) float32."""
    host = map.detach().cpu().numpy() if isinstance(map, torch.Tensor) else np.asarray(map)
    if host.dtype != np.float32 or host.ndim != 3 or host.shape[2] != 2:
        raise ValueError(f"a map is float32 (H, W, 2), not {host.dtype} {host.shape}")
    host = np.ascontiguousarray(host)
    need = N.lib().tsvpp_remap_lds_need(host.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 0, host.shape[1], host.shape[0], int(frame_w), int(frame_h), 1 if luma_only else 0)
    if need < 0:
        N.check(need)
    return need


def _cell_logs(cell):
    """(cw, ch) in output pixels as (log2_cw, log2_ch): positive powers of two (the range 4..256 is the C call's rule)"""
    try:
        cw, ch = (int(v) for v in cell)
    except (TypeError, ValueError):
        raise ValueError(f"a cell is (cw, ch), not {cell}") from None
    for v in (cw, ch):
        if v <= 0 or v & (v - 1):
            raise ValueError(f"a cell size is a power of two, not {v}")
    return cw.bit_length() - 1, ch.bit_length() - 1


def mesh_dims(dst_w, dst_h, cell):
    """(rows, cols) of the control grid of a dst_w x dst_h output at cell = (cw, ch) (tsvpp_mesh_dims): one point beyond the cell of the last pixel on each axis."""
    lw, lh = _cell_logs(cell)
    cols, rows = ctypes.c_int(0), ctypes.c_int(0)
    N.check(N.lib().tsvpp_mesh_dims(int(dst_w), int(dst_h), lw, lh, ctypes.byref(cols), ctypes.byref(rows)))
    return rows.value, cols.value


def _normalize_meshes(meshes, cell, dst_w, dst_h, device=None):
    """The meshes argument of convert_mesh / describe_mesh as an array of tsvpp_mesh: _normalize_maps for control grids.  cell: (cw, ch) for all meshes, or a list
    with one (cw, ch) per mesh.  A mesh is a float32 tensor (rows, cols, 2) of mesh_dims' shape whose last dimension is contiguous, optionally paired as
    (tensor, lds_bytes); without a device (describe_mesh) it may also be (pitch, lds_bytes) integers.  Anything else raises ValueError: nothing reaches the C call."""
    if isinstance(meshes, torch.Tensor) or (isinstance(meshes, tuple) and len(meshes) == 2 and not isinstance(meshes[1], (torch.Tensor, tuple, list))):
        meshes = [meshes]
    meshes = list(meshes)
    if not meshes:
        raise ValueError("at least one mesh is needed")
    if not isinstance(cell, (tuple, list)):
        raise ValueError(f"a cell is (cw, ch), not {cell}")
    cells = list(cell)
    if cells and not isinstance(cells[0], (tuple, list)):
        cells = [tuple(cells)] * len(meshes)
    if len(cells) != len(meshes):
        raise ValueError(f"{len(meshes)} meshes and {len(cells)} cells: give one (cw, ch) or one per mesh")
    recs = []
    for m, cl in zip(meshes, cells):
        lw, lh = _cell_logs(cl)
        rows, cols = ((dst_h - 1) >> lh) + 2, ((dst_w - 1) >> lw) + 2
        hint = 0
        if isinstance(m, (tuple, list)):
            if len(m) != 2:
                raise ValueError(f"a mesh is a tensor, (tensor, lds_bytes) or (pitch, lds_bytes), not {m}")
            m, hint = m[0], int(m[1])
        if not isinstance(m, torch.Tensor):
            if device is not None:
                raise ValueError(f"convert_mesh needs its meshes as tensors, not {type(m).__name__}")
            recs.append(N.Mesh(None, int(m), lw, lh, hint))
            continue
        if m.dtype != torch.float32:
            raise ValueError(f"a mesh is a float32 tensor, not {m.dtype}")
        if m.dim() != 3 or tuple(m.shape) != (rows, cols, 2):
            raise ValueError(f"a mesh for a {dst_w} x {dst_h} output at cell {tuple(cl)} has shape ({rows}, {cols}, 2), not {tuple(m.shape)}")
        if m.stride(2) != 1 or m.stride(1) != 2 or m.stride(0) < 2 * cols:
            raise ValueError(f"a mesh's last two dimensions are contiguous and its row stride is at least {2 * cols} elements: strides {tuple(m.stride())}")
        if device is not None and (not m.is_cuda or m.device.index != device):
            raise ValueError(f"a mesh lives on cuda:{device}, not on {m.device}")
        recs.append(N.Mesh(m.data_ptr() if m.is_cuda else None, 4 * m.stride(0), lw, lh, hint))
    return (N.Mesh * len(recs))(*recs)


def describe_mesh(params, frames, meshes, cell=(16, 16), remaps=None, border=None, aligned_outputs=True, dtype=None, mean=None, std=None):
    """What a convert_mesh of this request would launch, as a dict (tsvpp_describe_mesh: describe_remap's keys with meshes= and cell= for maps=, mode
    mesh_bilinear) -- host logic only, works without a GPU.  frames: as describe_rois; meshes: as for convert_mesh (tensors on any device: only strides and hints
    are read) or (pitch, lds_bytes) integers; cell, remaps and border as for convert_mesh."""
    def items(p, recs):
        ms = _normalize_meshes(meshes, cell, p.dst_width, p.dst_height)
        rs = _normalize_remaps(remaps, len(recs), len(ms))
        return len(ms), ms, len(rs), rs
    return _describe_coord((N.lib().tsvpp_describe_mesh, N.lib().tsvpp_describe_mesh_tensor), items, params, frames, border, aligned_outputs, dtype, mean, std)


def _host_pairs(a, what):
    """a tensor or array (H, W, 2) float32 as a contiguous numpy array, and whether it came as a tensor"""
    host = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if host.dtype != np.float32 or host.ndim != 3 or host.shape[2] != 2:
        raise ValueError(f"a {what} is float32 (H, W, 2), not {host.dtype} {host.shape}")
    return np.ascontiguousarray(host)


def _like(host, src):
    return torch.from_numpy(host).to(src.device) if isinstance(src, torch.Tensor) else host


_PF = ctypes.POINTER(ctypes.c_float)


def mesh_from_map(xy, cell):
    """A dense map (H, W, 2) of convert_remap as the warp mesh (rows, cols, 2) of convert_mesh at cell = (cw, ch) (tsvpp_mesh_from_map): the map sampled at the
    control positions; a position past the last pixel of an axis is extrapolated linearly from that axis's last two entries, in double, x first and then y.
    mesh_error says what the mesh loses.  numpy arrays give a numpy array, tensors a tensor on their device."""
    lw, lh = _cell_logs(cell)
    host = _host_pairs(xy, "map")
    h, w = host.shape[:2]
    rows, cols = mesh_dims(w, h, cell)
    out = np.empty((rows, cols, 2), np.float32)
    N.check(N.lib().tsvpp_mesh_from_map(host.ctypes.data_as(_PF), 0, w, h, lw, lh, out.ctypes.data_as(_PF), 0))
    return _like(out, xy)


def mesh_expand(mesh, dst_size, cell):
    """E(mesh): the dense map (dst_h, dst_w, 2) that convert_mesh samples through, from the function the kernel calls (tsvpp_mesh_expand); convert_remap of it is
    convert_mesh of the mesh, bit for bit.  dst_size: (dst_w, dst_h).  numpy arrays give a numpy array, tensors a tensor on their device."""
    lw, lh = _cell_logs(cell)
    w, h = (int(v) for v in dst_size)
    host = _host_pairs(mesh, "mesh")
    if host.shape[:2] != mesh_dims(w, h, cell):
        raise ValueError(f"a mesh for a {w} x {h} output at cell {tuple(cell)} has shape {mesh_dims(w, h, cell) + (2,)}, not {host.shape}")
    out = np.empty((h, w, 2), np.float32)
    N.check(N.lib().tsvpp_mesh_expand(host.ctypes.data_as(_PF), 0, w, h, lw, lh, out.ctypes.data_as(_PF), 0))
    return _like(out, mesh)


def mesh_error(xy, mesh, cell):
    """The largest |E(mesh) - map| in pixels over the finite entries of a dense map (H, W, 2) and a mesh for it (tsvpp_mesh_error): pick the largest cell whose
    error the application tolerates."""
    lw, lh = _cell_logs(cell)
    host, hm = _host_pairs(xy, "map"), _host_pairs(mesh, "mesh")
    h, w = host.shape[:2]
    if hm.shape[:2] != mesh_dims(w, h, cell):
        raise ValueError(f"a mesh for a {w} x {h} map at cell {tuple(cell)} has shape {mesh_dims(w, h, cell) + (2,)}, not {hm.shape}")
    worst = ctypes.c_float(0.0)
    N.check(N.lib().tsvpp_mesh_error(host.ctypes.data_as(_PF), 0, w, h, hm.ctypes.data_as(_PF), 0, lw, lh, ctypes.byref(worst)))
    return worst.value


def mesh_lds_hint(mesh, dst_size, cell, frame_w, frame_h, luma_only=False):
    """The LDS hint of a mesh for a dst_size = (dst_w, dst_h) output on a frame_w x frame_h frame (tsvpp_mesh_lds_need: remap_lds_hint of mesh_expand(mesh)) --
    what convert_mesh takes as (tensor, lds_bytes).  Copies the mesh to the host once; luma_only: for Y800 outputs."""
    lw, lh = _cell_logs(cell)
    w, h = (int(v) for v in dst_size)
    hm = _host_pairs(mesh, "mesh")
    if hm.shape[:2] != mesh_dims(w, h, cell):
        raise ValueError(f"a mesh for a {w} x {h} output at cell {tuple(cell)} has shape {mesh_dims(w, h, cell) + (2,)}, not {hm.shape}")
    need = N.lib().tsvpp_mesh_lds_need(hm.ctypes.data_as(_PF), 0, w, h, lw, lh, int(frame_w), int(frame_h), 1 if luma_only else 0)
    if need < 0:
        N.check(need)
    return need


def mesh_undistort(K, dist, new_K, dst_size, cell):
    """The undistortion mesh of a camera, as a numpy array (rows, cols, 2) float32: OpenCV's distortion model evaluated at the control positions in float64 -- the
    direct forward formula behind cv2.initUndistortRectifyMap (no rectification), no iteration, no dense map.  K, new_K: 3 x 3 camera matrices of the distorted
    frame and of the output; dist: (k1, k2, p1, p2[, k3[, k4, k5, k6]]); dst_size: (dst_w, dst_h); cell: (cw, ch).  For the output pixel (u, v):
    x = (u - cx') / fx', y = (v - cy') / fy', r2 = x x + y y, a = k1 r2 + k2 r2^2 + k3 r2^3, b = k4 r2 + k5 r2^2 + k6 r2^3, g = (a - b) / (1 + b) (the radial
    factor less one), dx = x g + 2 p1 x y + p2 (r2 + 2 x x), dy = y g + p1 (r2 + 2 y y) + 2 p2 x y, and the source position is
    ((u - cx') (fx / fx') + cx + fx dx, (v - cy') (fy / fy') + cy + fy dy): with no distortion and K = new_K exactly (u, v)."""
    _cell_logs(cell)
    K, new_K = np.asarray(K, np.float64), np.asarray(new_K, np.float64)
    d = [float(v) for v in np.asarray(dist, np.float64).ravel()]
    if K.shape != (3, 3) or new_K.shape != (3, 3):
        raise ValueError("K and new_K are 3 x 3 camera matrices")
    if len(d) not in (4, 5, 8):
        raise ValueError(f"dist is (k1, k2, p1, p2), with k3, or with k3 .. k6: not {len(d)} numbers")
    d += [0.0] * (8 - len(d))
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    w, h = (int(v) for v in dst_size)
    rows, cols = mesh_dims(w, h, cell)
    u = (np.arange(cols, dtype=np.float64) * int(cell[0]))[None, :]
    v = (np.arange(rows, dtype=np.float64) * int(cell[1]))[:, None]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    nfx, nfy, ncx, ncy = new_K[0, 0], new_K[1, 1], new_K[0, 2], new_K[1, 2]
    x, y = (u - ncx) / nfx + 0.0 * v, (v - ncy) / nfy + 0.0 * u
    r2 = x * x + y * y
    a = r2 * (k1 + r2 * (k2 + r2 * k3))
    b = r2 * (k4 + r2 * (k5 + r2 * k6))
    g = (a - b) / (1.0 + b)
    dx = x * g + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = y * g + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    mx = (u - ncx) * (fx / nfx) + cx + fx * dx
    my = (v - ncy) * (fy / nfy) + cy + fy * dy
    return np.ascontiguousarray(np.stack((mx, my), axis=-1).astype(np.float32))


def debug_last_launch():
    """DEBUG ONLY (TSVPP_DEBUG_KNOBS=1): what this thread's last conversion launched, in describe()'s keys (tsvpp_debug_last_launch)."""
    buf = ctypes.create_string_buffer(512)
    N.check(N.lib().tsvpp_debug_last_launch(buf, len(buf)))
    return _parse_selection(buf.value.decode())


def default_coeffs():
    c = N.Coeffs()
    N.lib().tsvpp_default_coeffs(ctypes.byref(c))
    return [getattr(c, f[0]) for f in N.Coeffs._fields_]
