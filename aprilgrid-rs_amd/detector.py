"""Host-side mirror of aprilgrid::detector (reference src/detector.rs) over the C ABI.

Same names, argument meaning and error behaviour as the reference where Python allows:
  TagFamily / TagFamily.from_str      src/tag_families.rs:5-28
  DetectorParams.default_params()     src/detector.rs:25-41
  Saddle                              src/saddle.rs:3-15
  TagDetector.new / __init__          src/detector.rs:364-406
  TagDetector.refined_saddle_points   src/detector.rs:408-446
  TagDetector.detect                  src/detector.rs:505-540
  TagDetector.detect_kornia           src/detector.rs:478-503
  TagDetector.rochade_refine          src/detector.rs:194-361 (the crate's pub fn, half_size_patch = 2)
  TagDetector.decode_quads            src/detector.rs:448-476 (try_decode_quad = the pub fns decode_positions, bit_code, best_tag)
  decode_positions, bit_code, best_tag  src/detector.rs:42-72, :74-122, :142-169 (the three pub fns themselves; on device tensors
                                      TagDetector.decode_positions_enqueue / bit_code_enqueue / best_tag_enqueue / decode_quads_staged)
  TagDetector.find_board              src/detector.rs:588-639 (the crate's pub fn try_find_best_board)
  TagDetector.detect_staged           src/detector.rs:505-540 as the staged chain on device tensors; its rounds (:510-539) by
                                      TagDetector.collect_tags_enqueue / collect_tags
  TagDetector.detect_tracked          the same from last call's tags: TagDetector.snap_points_enqueue / snap_points (no reference
                                      item: the prior corners snapped to this frame's saddles) -> grow boards -> decode -> collect
  TagDetector.gaussian_blur_f32       src/image_util.rs:110-206 (the crate's pub fn, any sigma up to 8)
  TagDetector.hessian_response        src/image_util.rs:72-109 (the crate's pub fn)
An image is a numpy array standing for the DynamicImage variants the reference is fed:
HxW uint8 (ImageLuma8), HxW uint16 (ImageLuma16), HxWx3 uint8 (ImageRgb8); HxWx2 / HxWx4 uint8 (ImageLumaA8, ImageRgba8),
HxWx2 / HxWx3 / HxWx4 uint16 (ImageLumaA16, ImageRgb16, ImageRgba16).  BGR / BGRA order and channel-first planes (3xHxW uint8)
are named with format=: the shape cannot tell them from RGB / RGBA or a three-row HxWx? image.
"""
import ctypes as C
import enum
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._ffi import LIB_PATH, build_library

SADDLE_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("k", "f4"), ("theta", "f4"), ("phi", "f4")])
_CLUSTER_DTYPE = np.dtype([("first_index", "u4"), ("size", "u4"), ("cx", "f4"), ("cy", "f4")])
CLUSTER_DTYPE = _CLUSTER_DTYPE  # agx_cluster_info

Saddle = namedtuple("Saddle", ["p", "k", "theta", "phi"])  # p = (x, y)


def library_path():
    return LIB_PATH


class AgxError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _ffi.lib().agx_status_string(status).decode()
        super().__init__("%s (%d)%s" % (msg, status, (": " + detail) if detail else ""))


class TagFamily(enum.IntEnum):
    T16H5 = 0
    T25H7 = 1
    T25H9 = 2
    T36H11 = 3
    T36H11B1 = 4

    @staticmethod
    def from_str(s):
        out = C.c_int(-1)
        st = _ffi.lib().agx_family_from_str(s.encode(), C.byref(out))
        if st != _ffi.AGX_OK:
            raise ValueError("unknown tag family %r" % (s,))  # reference: Err(std::fmt::Error)
        return TagFamily(out.value)


@dataclass
class DetectorParams:
    tag_spacing_ratio: float = 0.3
    min_saddle_angle: float = 30.0
    max_saddle_angle: float = 60.0
    max_num_of_boards: int = 2

    @staticmethod
    def default_params():
        p = _ffi.Params()
        _ffi.lib().agx_default_params(C.byref(p))
        return DetectorParams(p.tag_spacing_ratio, p.min_saddle_angle, p.max_saddle_angle, p.max_num_of_boards)

    def _c(self):
        return _ffi.Params(self.tag_spacing_ratio, self.min_saddle_angle, self.max_saddle_angle,
                           self.max_num_of_boards)


def _check_layout(shape, itemsize, kind, fmt):
    """format= override: the array / tensor [..., H, W(, C)] (or [..., 3, H, W] for the planar layout) must be what `fmt` says;
    -> (H, W, bytes per pixel of a row)."""
    if fmt not in _ffi.FORMAT_LAYOUT:
        raise AgxError(_ffi.AGX_ERR_FORMAT, "unknown format %r" % (fmt,))
    bpp, planes, dt = _ffi.FORMAT_LAYOUT[fmt]
    ch = bpp // int(dt[1])
    want_kind = {"u": "iu", "f": "f"}[dt[0]]  # (torch spells 16-bit pixels int16 where it has no uint16)
    ok = itemsize == int(dt[1]) and kind in want_kind
    if planes == 3:
        ok = ok and len(shape) >= 3 and shape[-3] == 3
    elif ch == 1:
        ok = ok and len(shape) >= 2
        shape = tuple(shape) + (1,)
    else:
        ok = ok and len(shape) >= 3 and shape[-1] == ch
        shape = tuple(shape)
    if not ok:
        raise AgxError(_ffi.AGX_ERR_FORMAT, "array %s of %d-byte elements is not format %d" % (tuple(shape), itemsize, fmt))
    return (shape[-2], shape[-1], bpp) if planes == 3 else (shape[-3], shape[-2], bpp)


def _image_args(img, format=None):
    a = np.ascontiguousarray(img)
    if format is not None:
        h, w, bpp = _check_layout(a.shape, a.dtype.itemsize, a.dtype.kind, format)
        if format == _ffi.AGX_RGB8P:  # the three planes one under the other, as the library reads them
            a = a.reshape(3 * h, w)
        return a, format, w * bpp
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
        a = np.ascontiguousarray(a)
    if a.ndim == 2 and a.dtype == np.uint8:
        return a, _ffi.AGX_L8, a.shape[1]
    if a.ndim == 2 and a.dtype == np.uint16:
        return a, _ffi.AGX_L16, a.shape[1] * 2
    if a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8:
        return a, _ffi.AGX_RGB8, a.shape[1] * 3
    if a.ndim == 2 and a.dtype == np.float32:  # the caller's own to_luma32f plane (any DynamicImage variant)
        return a, _ffi.AGX_LF32, a.shape[1] * 4
    if a.ndim == 3 and a.dtype == np.uint8 and a.shape[2] in (2, 4):
        return a, (_ffi.AGX_LA8 if a.shape[2] == 2 else _ffi.AGX_RGBA8), a.shape[1] * a.shape[2]
    if a.ndim == 3 and a.dtype == np.uint16 and a.shape[2] in (2, 3, 4):
        return a, {2: _ffi.AGX_LA16, 3: _ffi.AGX_RGB16, 4: _ffi.AGX_RGBA16}[a.shape[2]], a.shape[1] * a.shape[2] * 2
    raise AgxError(_ffi.AGX_ERR_FORMAT, "image must be HxW uint8/uint16/float32 or HxWx{2,3,4} uint8/uint16, got %s %s"
                   % (a.shape, a.dtype))


def _image_hw(a, fmt):
    """(H, W) of the array _image_args returned (the planar layout is a [3H, W] array)."""
    return (a.shape[0] // 3, a.shape[1]) if fmt == _ffi.AGX_RGB8P else a.shape[:2]


class TagDetector:
    """aprilgrid::detector::TagDetector on one MI355X (one handle = one device + stream;
    use one instance per thread)."""

    def __init__(self, tag_family, optional_detector_params=None, device=0, blur_sigma=None, half_size_patch=None):
        self._lib = _ffi.lib()
        self._h = C.c_void_p()
        self._saddle_buf = None  # refined_saddle_points' output buffer: (array [cap][5] f32, its address, count word)
        fam = TagFamily.from_str(tag_family) if isinstance(tag_family, str) else TagFamily(tag_family)
        prm = optional_detector_params._c() if optional_detector_params is not None else None
        st = self._lib.agx_detector_create(int(fam), C.byref(prm) if prm is not None else None, int(device),
                                           C.byref(self._h))
        if st != _ffi.AGX_OK:
            self._h = C.c_void_p()
            raise AgxError(st, "agx_detector_create(device=%d): %s" % (device, self._lib.agx_last_error(None).decode()))
        self.tag_family = fam
        self.detector_params = optional_detector_params or DetectorParams.default_params()
        self.device = device
        self._batch = None
        self._detect = None  # detect_batch_enqueue's batch: (n, cap, frames kept alive, device outputs or None)
        self._refine = None  # refine_points_enqueue's batch: (n, points per frame, tensors kept alive, device outputs or None)
        self._decode = None  # decode_quads_enqueue's batch: (n, quads per frame, tensors kept alive, device outputs or None)
        self._find = None    # find_boards_enqueue's batch: (n, quads per frame, tensors kept alive, device outputs or None)
        self._grow = None    # grow_boards_enqueue's batch: the tensors kept alive (the library itself knows whether it is in flight)
        self._init = None    # init_quads_enqueue's batch: likewise
        self._clusters = None  # clusters_enqueue's batch: (n, clusters per frame, tensors kept alive, device outputs or None)
        try:
            if blur_sigma is not None:
                self.set_blur_sigma(blur_sigma)
            if half_size_patch is not None:
                self.set_half_size_patch(half_size_patch)
        except AgxError:
            self.close()
            raise

    new = classmethod(lambda cls, tag_family, optional_detector_params=None, device=0, blur_sigma=None, half_size_patch=None:
                      cls(tag_family, optional_detector_params, device, blur_sigma, half_size_patch))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.agx_detector_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != _ffi.AGX_OK:
            raise AgxError(st, self._lib.agx_last_error(self._h).decode())

    # ---- reference API -------------------------------------------------------------------
    def refined_saddle_points(self, img, as_array=False, cap=16384, format=None):
        """-> Vec<Saddle> (list of Saddle) or, with as_array=True, a SADDLE_DTYPE array.  format: the agx_format of `img`
        instead of the one its shape and dtype suggest (BGR / BGRA order, 3xHxW planes)."""
        a, fmt, stride = _image_args(img, format)
        h, w = _image_hw(a, fmt)
        # the library writes into a buffer this handle keeps (plain f32 rows: allocating and slicing a structured array per call
        # cost 12 us of a 116 us call); the caller gets its own copy
        buf = self._saddle_buf
        if buf is None or buf[0].shape[0] < cap:
            arr = np.empty((cap, 5), np.float32)
            buf = self._saddle_buf = (arr, arr.ctypes.data, C.c_uint32(0))
        arr, ptr, n = buf
        img_ptr = a.__array_interface__["data"][0]
        st = self._lib.agx_refined_saddle_points(self._h, img_ptr, w, h, stride, fmt, ptr, arr.shape[0], C.byref(n))
        if st == _ffi.AGX_ERR_CAPACITY and n.value > arr.shape[0]:  # the reference's Vec has no limit: retry with room
            arr = np.empty((int(n.value), 5), np.float32)
            self._saddle_buf = (arr, arr.ctypes.data, n)
            ptr = arr.ctypes.data
            st = self._lib.agx_refined_saddle_points(self._h, img_ptr, w, h, stride, fmt, ptr, arr.shape[0], C.byref(n))
        self._check(st)
        res = arr[: n.value].copy().view(SADDLE_DTYPE).reshape(-1)
        if as_array:
            return res
        return [Saddle((float(s["x"]), float(s["y"])), float(s["k"]), float(s["theta"]), float(s["phi"]))
                for s in res]

    def detect(self, img, cap=4096, format=None):
        """-> HashMap<u32, [(f32,f32);4]> as {tag_id: 4x2 float32 array}.  format: as refined_saddle_points."""
        a, fmt, stride = _image_args(img, format)
        h, w = _image_hw(a, fmt)
        out = (_ffi.TagC * cap)()
        n = C.c_uint32(0)
        self._check(self._lib.agx_detect(self._h, a.ctypes.data, w, h, stride, fmt, out, cap, C.byref(n)))
        return {int(out[i].id): np.array(out[i].xy, np.float32).reshape(4, 2) for i in range(n.value)}

    def detect_planes(self, luma32f, luma8, cap=4096):
        """detect() of any DynamicImage variant from its two planes: img.to_luma32f() (HxW float32)
        for the saddle chain and img.to_luma8() (HxW uint8) for the decode."""
        f = np.ascontiguousarray(luma32f, np.float32)
        g = np.ascontiguousarray(luma8, np.uint8)
        assert f.shape == g.shape and f.ndim == 2
        h, w = f.shape
        out = (_ffi.TagC * cap)()
        n = C.c_uint32(0)
        self._check(self._lib.agx_detect_planes(self._h, f.ctypes.data, w * 4, g.ctypes.data, w, w, h, out, cap,
                                                C.byref(n)))
        return {int(out[i].id): np.array(out[i].xy, np.float32).reshape(4, 2) for i in range(n.value)}

    TAG_DTYPE = np.dtype([("id", "u4"), ("xy", "f4", (8,))])

    def detect_batch_raw(self, frames, n_threads=0, cap=1024, device_frames=None, out=None, counts=None, status=None, format=None):
        """agx_detect_batch as a C / Rust caller uses it: frames = numpy [N,H,W] uint8 / uint16 or [N,H,W,3] uint8 in
        host memory (optionally also resident on the GPU as the torch tensor device_frames); the tags go into the
        caller's arrays out [N, cap] of TAG_DTYPE, counts [N] uint32, status [N] int32 (allocated when None).
        -> (rc, out, counts, status); nothing is raised for a capacity status."""
        a = np.ascontiguousarray(frames)
        img0, fmt, stride = _image_args(a[0], format)
        if fmt == _ffi.AGX_LF32:
            raise AgxError(_ffi.AGX_ERR_FORMAT, "detect_batch takes frames of integer pixels")
        n = a.shape[0]
        h, w = _image_hw(img0, fmt)
        frame_stride = stride * h * _ffi.FORMAT_LAYOUT[fmt][1]
        if out is None:
            out = np.zeros((n, cap), self.TAG_DTYPE)
        if counts is None:
            counts = np.zeros(n, np.uint32)
        if status is None:
            status = np.zeros(n, np.int32)
        assert out.shape == (n, cap) and out.dtype == self.TAG_DTYPE and counts.shape == (n,) and status.shape == (n,)
        status[:] = _ffi.AGX_ERR_STATE  # (every slot is written by the call; one that is not stays an error)
        dptr = None
        if device_frames is not None:
            # the chain reads device_frames, the decode reads `frames`: they must be the same pixels
            t = device_frames
            if not (getattr(t, "is_cuda", False) and t.is_contiguous()):
                raise AgxError(_ffi.AGX_ERR_ARG, "device_frames must be a contiguous CUDA tensor")
            if t.device.index != self.device:
                raise AgxError(_ffi.AGX_ERR_ARG, "device_frames is on device %s, the detector on %d" % (t.device.index, self.device))
            if tuple(t.shape) != tuple(a.shape) or t.element_size() != a.dtype.itemsize:
                raise AgxError(_ffi.AGX_ERR_ARG, "device_frames %s / %d-byte elements differ from frames %s / %d-byte elements"
                               % (tuple(t.shape), t.element_size(), tuple(a.shape), a.dtype.itemsize))
            dptr = t.data_ptr()
        rc = self._lib.agx_detect_batch(self._h, a.ctypes.data, dptr, n, w, h, stride, frame_stride, fmt,
                                        out.ctypes.data, cap, counts.ctypes.data, status.ctypes.data, n_threads)
        return rc, out, counts, status

    def detect_batch(self, frames, n_threads=0, cap=1024, device_frames=None, raise_on_overflow=True, format=None):
        """detect() over a batch: frames = numpy [N,H,W] uint8 / uint16 or [N,H,W,3] uint8 in host
        memory (optionally also resident on the GPU as the torch tensor device_frames).  The chain
        runs on the device chunk by chunk while n_threads host threads (0 = agx_host_parallelism(): the
        CPUs this process may keep busy) run the uploads and the
        board search + decode.  -> list of {tag_id: 4x2 corners}.  A frame with more than `cap` tags (or
        over the detector's saddle capacity) raises by default; raise_on_overflow=False returns
        (results, status) instead: status[i] != 0 marks such a frame (its entry is None), every other
        frame keeps its result."""
        rc, out, counts, status = self.detect_batch_raw(frames, n_threads, cap, device_frames, format=format)
        n = len(counts)
        if rc != _ffi.AGX_OK and (raise_on_overflow or rc != _ffi.AGX_ERR_CAPACITY):
            self._check(rc)
        res = [None if status[i] != 0 else {int(t["id"]): t["xy"].reshape(4, 2).copy() for t in out[i, : counts[i]]} for i in range(n)]
        return res if raise_on_overflow else (res, status)

    def detect_kornia(self, img):
        """kornia::image::Image<u8, N>: an HxWxN uint8 array, N in {1, 3} (else the reference
        panics 'Only support u8c1 and u8c3')."""
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3):
            raise AgxError(_ffi.AGX_ERR_FORMAT, "Only support u8c1 and u8c3")
        return self.detect(a)

    def detect_from_saddles(self, saddles, luma8, cap=4096):
        """Host tail only (board search + decode) from a SADDLE_DTYPE array and the u8 luma."""
        s = np.ascontiguousarray(saddles, SADDLE_DTYPE)
        g = np.ascontiguousarray(luma8, np.uint8)
        h, w = g.shape
        out = (_ffi.TagC * cap)()
        n = C.c_uint32(0)
        self._check(self._lib.agx_detect_from_saddles(self._h, s.ctypes.data, len(s), g.ctypes.data, w, h, w, out,
                                                      cap, C.byref(n)))
        return {int(out[i].id): np.array(out[i].xy, np.float32).reshape(4, 2) for i in range(n.value)}

    @staticmethod
    def detect_tail(tag_family, saddles, luma8, optional_detector_params=None, cap=4096, n_threads=1):
        """Host tail without a device: board search + decode from a SADDLE_DTYPE array (n_threads > 1: the
        frame's board search on several host threads, same result)."""
        fam = TagFamily.from_str(tag_family) if isinstance(tag_family, str) else TagFamily(tag_family)
        prm = optional_detector_params._c() if optional_detector_params is not None else None
        s = np.ascontiguousarray(saddles, SADDLE_DTYPE)
        g = np.ascontiguousarray(luma8, np.uint8)
        h, w = g.shape
        out = (_ffi.TagC * cap)()
        n = C.c_uint32(0)
        st = _ffi.lib().agx_detect_tail_threads(int(fam), C.byref(prm) if prm is not None else None, s.ctypes.data, len(s),
                                                g.ctypes.data, w, h, w, out, cap, C.byref(n), int(n_threads))
        if st != _ffi.AGX_OK:
            raise AgxError(st)
        return {int(out[i].id): np.array(out[i].xy, np.float32).reshape(4, 2) for i in range(n.value)}

    @staticmethod
    def luma8(img, format=None):
        a, fmt, stride = _image_args(img, format)
        h, w = _image_hw(a, fmt)
        out = np.empty((h, w), np.uint8)
        st = _ffi.lib().agx_luma8(a.ctypes.data, w, h, stride, fmt, out.ctypes.data)
        if st != _ffi.AGX_OK:
            raise AgxError(st)
        return out

    # ---- batches resident in device memory ----------------------------------------------
    def set_limits(self, max_candidates=0, max_clusters=0, max_saddles=0):
        self._check(self._lib.agx_detector_set_limits(self._h, max_candidates, max_clusters, max_saddles))

    def set_stream(self, hip_stream_ptr, external=True):
        """external=True: launch on the given hipStream_t (0 = HIP's default stream);
        external=False: back to the detector's own stream."""
        self._check(self._lib.agx_detector_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0), 1 if external else 0))
        self._stream_ptr = hip_stream_ptr if external else "own"

    def set_blur_sigma(self, sigma):
        """The sigma of the chain's blur from the next enqueue on (the reference hard-codes 1.5, the default): positive,
        finite, at most 8.  Every entry that runs the chain on this detector follows it."""
        self._check(self._lib.agx_detector_set_blur_sigma(self._h, float(sigma)))

    @property
    def blur_sigma(self):
        v = C.c_float(0.0)
        self._check(self._lib.agx_detector_get_blur_sigma(self._h, C.byref(v)))
        return v.value

    @blur_sigma.setter
    def blur_sigma(self, sigma):
        self.set_blur_sigma(sigma)

    def set_half_size_patch(self, half_size_patch):
        """rochade_refine's half_size_patch inside the chain from the next enqueue on (the reference hard-codes 2, the default):
        1 .. 4.  Every entry that runs the chain on this detector follows it; refine_points / rochade_refine do not (they
        refine at 2, or at their own half_size_patch argument)."""
        self._check(self._lib.agx_detector_set_half_size_patch(self._h, int(half_size_patch)))

    @property
    def half_size_patch(self):
        v = C.c_int(0)
        self._check(self._lib.agx_detector_get_half_size_patch(self._h, C.byref(v)))
        return v.value

    @half_size_patch.setter
    def half_size_patch(self, half_size_patch):
        self.set_half_size_patch(half_size_patch)

    def set_option(self, name, value):
        self._check(self._lib.agx_detector_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int(0)
        self._check(self._lib.agx_detector_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def sync(self):
        self._check(self._lib.agx_detector_sync(self._h))

    def _follow_torch_stream(self, frames=None):
        """Stream-order the chain behind whatever produced `frames`: launch on torch's current
        stream of that device (a detector otherwise uses its own non-blocking stream, which
        does not wait for work queued on torch's streams).  frames None: the detector's own device."""
        import torch
        s = torch.cuda.current_stream(frames.device if frames is not None else self.device).cuda_stream
        if getattr(self, "_stream_ptr", "own") != s:
            self.set_stream(s)

    @staticmethod
    def _tensor_format(frames, format=None, strided=False):
        """-> (agx_format, bytes per pixel of a row); format: the caller's word instead of what the shape suggests.
        strided: the caller takes the strides from the tensor (planes_enqueue)."""
        import torch
        if not frames.is_cuda or not (strided or frames.is_contiguous()):
            raise AgxError(_ffi.AGX_ERR_ARG, "frames must be a contiguous device tensor")
        if format is not None:
            kind = "f" if frames.dtype.is_floating_point else "i"
            return format, _check_layout(tuple(frames.shape[1:]), frames.element_size(), kind, format)[2]
        sixteen = (torch.int16, getattr(torch, "uint16", torch.int16))
        if frames.dim() == 3 and frames.dtype == torch.uint8:
            return _ffi.AGX_L8, 1
        if frames.dim() == 3 and frames.dtype in sixteen:
            return _ffi.AGX_L16, 2
        if frames.dim() == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8:
            return _ffi.AGX_RGB8, 3
        if frames.dim() == 3 and frames.dtype == torch.float32:
            return _ffi.AGX_LF32, 4
        if frames.dim() == 4 and frames.dtype == torch.uint8 and frames.shape[3] in (2, 4):
            if frames.shape[1] == 3:  # [N,3,H,2|4]: three planes of a narrow image, or a 3-row LA8 / RGBA8 image?
                raise AgxError(_ffi.AGX_ERR_FORMAT, "frame tensor %s is ambiguous (channel-first or channel-last): name it with format="
                               % (tuple(frames.shape),))
            return (_ffi.AGX_LA8, 2) if frames.shape[3] == 2 else (_ffi.AGX_RGBA8, 4)
        if frames.dim() == 4 and frames.dtype == torch.uint8 and frames.shape[1] == 3:  # channel-first (shape[3] != 3 here)
            return _ffi.AGX_RGB8P, 1
        if frames.dim() == 4 and frames.dtype in sixteen and frames.shape[3] in (2, 3, 4):
            return {2: (_ffi.AGX_LA16, 4), 3: (_ffi.AGX_RGB16, 6), 4: (_ffi.AGX_RGBA16, 8)}[int(frames.shape[3])]
        raise AgxError(_ffi.AGX_ERR_FORMAT, "unsupported frame tensor %s %s" % (tuple(frames.shape), frames.dtype))

    @staticmethod
    def _tensor_geometry(frames, fmt, bpp):
        """-> (n, w, h, row stride, frame stride) of a contiguous batch tensor in format fmt."""
        planes = _ffi.FORMAT_LAYOUT[fmt][1]
        n = frames.shape[0]
        h, w = (frames.shape[2], frames.shape[3]) if planes == 3 else (frames.shape[1], frames.shape[2])
        return n, w, h, w * bpp, w * h * bpp * planes

    def saddles_batch_enqueue(self, frames, format=None):
        """frames: a torch tensor on this detector's GPU, contiguous -- [N,H,W] uint8 (L8), [N,H,W] int16/uint16 (L16),
        [N,H,W,3] uint8 (RGB8), [N,H,W,2] / [N,H,W,4] uint8 (LA8 / RGBA8), [N,3,H,W] uint8 with W > 4 (planar RGB8: what torch
        image decoders return; W = 3 reads as RGB8 as ever, W = 2 or 4 is ambiguous and must be named), [N,H,W,2|3|4] int16/uint16 (LA16 / RGB16 / RGBA16).  format: the agx_format instead of the one
        the shape suggests (AGX_BGR8 / AGX_BGRA8 can only be named).  Returns immediately; see saddles_batch_fetch."""
        fmt, bpp = self._tensor_format(frames, format)
        self._follow_torch_stream(frames)
        n, w, h, rs, fs = self._tensor_geometry(frames, fmt, bpp)
        self._check(self._lib.agx_saddles_batch_enqueue(self._h, frames.data_ptr(), n, w, h, rs, fs, fmt))
        self._batch = (n, frames)  # keep the tensor alive until fetched
        self._detect = None
        self._refine = None
        self._decode = self._grow = self._find = None

    def saddles_batch_enqueue_to(self, frames, out_saddles, frame_table, format=None):
        """Device-resident results: out_saddles float32 [capacity, 5] and frame_table int32
        [n_frames, 4] (count, offset, status, clusters) are torch tensors on the same GPU."""
        fmt, bpp = self._tensor_format(frames, format)
        self._follow_torch_stream(frames)
        n, w, h, rs, fs = self._tensor_geometry(frames, fmt, bpp)
        assert out_saddles.is_cuda and out_saddles.is_contiguous() and out_saddles.shape[1] == 5
        assert frame_table.is_cuda and frame_table.is_contiguous() and tuple(frame_table.shape) == (n, 4)
        self._check(self._lib.agx_saddles_batch_enqueue_to(
            self._h, frames.data_ptr(), n, w, h, rs, fs, fmt, out_saddles.data_ptr(),
            out_saddles.shape[0], frame_table.data_ptr()))
        self._batch = None
        self._detect = None
        self._refine = None
        self._decode = self._grow = self._find = None

    def saddles_batch_enqueue_ptr(self, dptr, n, w, h, row_stride, frame_stride, fmt, follow_torch_stream=True):
        """agx_saddles_batch_enqueue on a raw device address (any row / frame stride: a view cut out of a larger allocation).
        Like the tensor forms it is launched on torch's current stream of the detector's device, behind whatever torch has
        queued there to produce the frames (and torch events on that stream see the kernels); follow_torch_stream=False keeps
        the stream the detector is on (its own non-blocking one unless set_stream was called: the caller orders the work)."""
        if follow_torch_stream:
            self._follow_torch_stream()
        self._check(self._lib.agx_saddles_batch_enqueue(self._h, C.c_void_p(dptr), n, w, h, row_stride, frame_stride,
                                                        fmt))
        self._batch = (n, None)
        self._detect = None
        self._refine = None
        self._decode = self._grow = self._find = None

    def saddles_batch_fetch(self, cap_per_frame=None, raise_on_overflow=True):
        """-> (list of SADDLE_DTYPE arrays, one per frame; per-frame status array).  cap_per_frame None:
        sized from the batch's longest list."""
        if self._batch is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no batch enqueued")
        n = self._batch[0]
        if cap_per_frame is None:
            counts = np.zeros(n, np.uint32)
            st = self._lib.agx_saddles_batch_fetch(self._h, None, 0, counts.ctypes.data, None)  # counts only
            if st not in (_ffi.AGX_OK, _ffi.AGX_ERR_CAPACITY):
                self._check(st)
            cap_per_frame = max(1, int(counts.max()))
        out = np.zeros((n, cap_per_frame), SADDLE_DTYPE)
        counts = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        st = self._lib.agx_saddles_batch_fetch(self._h, out.ctypes.data, cap_per_frame, counts.ctypes.data,
                                               status.ctypes.data)
        if st != _ffi.AGX_OK and (raise_on_overflow or st != _ffi.AGX_ERR_CAPACITY):
            self._check(st)
        res = [out[i, : counts[i]].copy() if status[i] == 0 else out[i, :0].copy() for i in range(n)]
        return res, status

    def saddles_batch_fetch_into(self, out, counts, status):
        """agx_saddles_batch_fetch into caller-owned arrays (what a Rust / C caller does: no allocation per call): out
        SADDLE_DTYPE [n, cap], counts uint32 [n], status int32 [n].  Returns the call's status (0 or AGX_ERR_CAPACITY)."""
        if self._batch is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no batch enqueued")
        n = self._batch[0]
        assert out.dtype == SADDLE_DTYPE and out.shape[0] == n and out.flags.c_contiguous and counts.shape == (n,) and status.shape == (n,)
        st = self._lib.agx_saddles_batch_fetch(self._h, out.ctypes.data, out.shape[1], counts.ctypes.data, status.ctypes.data)
        if st not in (_ffi.AGX_OK, _ffi.AGX_ERR_CAPACITY):
            self._check(st)
        return st

    def detect_batch_enqueue(self, frames, cap=1024, out=None, format=None):
        """detect() over a batch resident on this detector's GPU: frames and format= as saddles_batch_enqueue (every integer
        layout, contiguous; float32 planes are refused), stream-ordered behind torch's current stream.
        Returns immediately; detect_batch_fetch waits.  out=(tags, counts, status): device-resident results instead --
        tags int32 [N, cap, 9] (id, then the 8 corner floats as bits: split_device_tags), counts int32 [N], status int32 [N],
        final once detect_batch_fetch has returned (a frame handed back to the host tail reads count 0 / AGX_ERR_STATE until then)."""
        fmt, bpp = self._tensor_format(frames, format)
        if fmt == _ffi.AGX_LF32:
            raise AgxError(_ffi.AGX_ERR_FORMAT, "detect_batch takes frames of integer pixels")
        n, w, h, rs, fs = self._tensor_geometry(frames, fmt, bpp)
        self._follow_torch_stream(frames)
        self._enqueue_detect(frames.data_ptr(), n, w, h, rs, fs, fmt, cap, out, keep=frames)

    def detect_batch_enqueue_ptr(self, dptr, n, w, h, row_stride, frame_stride, fmt, cap=1024, out=None, follow_torch_stream=True):
        """detect_batch_enqueue on a raw device address with any row / frame stride (as saddles_batch_enqueue_ptr); the caller
        keeps the memory alive until detect_batch_fetch."""
        if follow_torch_stream:
            self._follow_torch_stream()
        self._enqueue_detect(dptr, n, w, h, row_stride, frame_stride, fmt, cap, out, keep=None)

    def _enqueue_detect(self, dptr, n, w, h, row_stride, frame_stride, fmt, cap, out, keep):
        self._batch = None  # (one batch in flight per handle: this one replaces a saddle batch)
        self._detect = None
        self._refine = None
        self._decode = self._grow = self._find = None
        if out is None:
            self._check(self._lib.agx_detect_batch_enqueue(self._h, C.c_void_p(dptr), n, w, h, row_stride, frame_stride, fmt, cap))
        else:
            import torch
            tags, counts, status = out
            for t, shape in ((tags, (n, cap, 9)), (counts, (n,)), (status, (n,))):
                if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == torch.int32 and tuple(t.shape) == shape):
                    raise AgxError(_ffi.AGX_ERR_ARG, "out tensors must be contiguous int32 CUDA tensors [n, cap, 9], [n], [n]")
                if t.device.index != self.device:
                    raise AgxError(_ffi.AGX_ERR_ARG, "out tensor on device %s, the detector on %d" % (t.device.index, self.device))
            self._check(self._lib.agx_detect_batch_enqueue_to(self._h, C.c_void_p(dptr), n, w, h, row_stride, frame_stride, fmt,
                                                              tags.data_ptr(), cap, counts.data_ptr(), status.data_ptr()))
        self._detect = (n, cap, keep, out)  # (frames and outputs stay alive until fetched)

    def detect_batch_fetch_raw(self, n_threads=0):
        """agx_detect_batch_fetch -> (rc, out [N, cap] TAG_DTYPE, counts uint32 [N], status int32 [N]) as detect_batch_raw; after
        detect_batch_enqueue(out=...) -> (rc, tags, counts, status), the device tensors.  Nothing is raised for a frame status."""
        if self._detect is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no detect batch enqueued")
        n, cap, _, dev_out = self._detect
        self._detect = None
        if dev_out is not None:
            rc = self._lib.agx_detect_batch_fetch(self._h, None, None, None, n_threads)
            if rc not in (_ffi.AGX_OK, _ffi.AGX_ERR_CAPACITY):
                self._check(rc)
            return (rc,) + tuple(dev_out)
        out = np.zeros((n, cap), self.TAG_DTYPE)
        counts = np.zeros(n, np.uint32)
        status = np.full(n, _ffi.AGX_ERR_STATE, np.int32)
        rc = self._lib.agx_detect_batch_fetch(self._h, out.ctypes.data, counts.ctypes.data, status.ctypes.data, n_threads)
        if rc not in (_ffi.AGX_OK, _ffi.AGX_ERR_CAPACITY):
            self._check(rc)
        return rc, out, counts, status

    def detect_batch_fetch(self, n_threads=0, raise_on_overflow=True):
        """Wait for detect_batch_enqueue's batch -> what detect_batch returns (list of {tag_id: 4x2 corners}; with
        raise_on_overflow=False (results, status)).  After detect_batch_enqueue(out=...) the results stay on the device:
        -> (tags, counts, status), the tensors passed as out (raise_on_overflow as above)."""
        rc, out, counts, status = self.detect_batch_fetch_raw(n_threads)
        if rc != _ffi.AGX_OK and raise_on_overflow:
            self._check(rc)
        if not isinstance(out, np.ndarray):
            return out, counts, status
        res = [None if status[i] != 0 else {int(t["id"]): t["xy"].reshape(4, 2).copy() for t in out[i, : counts[i]]}
               for i in range(len(counts))]
        return res if raise_on_overflow else (res, status)

    def detect_batch_device(self, frames, n_threads=0, cap=1024, raise_on_overflow=True, format=None):
        """detect_batch for frames resident on the GPU only (a torch tensor): detect_batch_enqueue + detect_batch_fetch."""
        self.detect_batch_enqueue(frames, cap, format=format)
        return self.detect_batch_fetch(n_threads, raise_on_overflow)

    @staticmethod
    def split_device_tags(tags):
        """tags int32 [..., cap, 9] of detect_batch_enqueue(out=...) -> (ids int32 [..., cap], corners float32 [..., cap, 4, 2])."""
        import torch
        return tags[..., 0], tags[..., 1:].contiguous().view(torch.float32).reshape(*tags.shape[:-1], 4, 2)

    # ---- rochade_refine of caller-given points (src/detector.rs:194-361) ------------------
    _REFINE_IMAGE = {"blurred": _ffi.AGX_REFINE_BLURRED, "plane": _ffi.AGX_REFINE_PLANE}

    def _refine_image(self, image):
        if image not in self._REFINE_IMAGE:
            raise AgxError(_ffi.AGX_ERR_ARG, "image must be 'blurred' or 'plane', got %r" % (image,))
        return self._REFINE_IMAGE[image]

    def rochade_refine(self, img, points, image="blurred", format=None, half_size_patch=2):
        """detector::rochade_refine(image_input, initial_corners, half_size_patch) on a host image: points = n (x, y) pairs;
        half_size_patch in 1 .. 4 (2: what the detector itself passes).
        image="blurred": img is an image of any format and is refined on its blur at the handle's sigma, as refined_saddle_points does;
        image="plane": img is an HxW float32 plane and IS image_input.  -> (records [n] SADDLE_DTYPE, status [n] uint32
        AGX_POINT_*), in input order; a rejected point's record is zero.  The reference's Vec<Saddle> is
        records[status == AGX_POINT_REFINED]."""
        a, fmt, stride = _image_args(img, format)
        h, w = _image_hw(a, fmt)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = np.zeros(n, SADDLE_DTYPE)
        status = np.zeros(n, np.uint32)
        n_refined = C.c_uint32(0)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_rochade_refine_h(self._h, a.ctypes.data, w, h, stride, fmt, self._refine_image(image), pts.ctypes.data, n,
                                                   out.ctypes.data, status.ctypes.data, C.byref(n_refined), int(half_size_patch)))
        assert n_refined.value == int((status == _ffi.AGX_POINT_REFINED).sum())
        return out, status

    def refine_points_enqueue(self, frames, points, counts=None, out=None, status=None, image="blurred", format=None, half_size_patch=2):
        """rochade_refine over a batch on this detector's GPU, stream-ordered behind torch's current stream; returns immediately.
        frames and format= as saddles_batch_enqueue (image="plane": [N,H,W] float32, refined as it is); points: float32 [N,P,2]
        (x, y); counts: optional int32 [N], the points of frame f (at most P; slots beyond are not written); out float32 [N,P,5]
        and status int32 [N,P]: device-resident results (both or neither) -- without them refine_points_fetch returns arrays.
        half_size_patch: rochade_refine's third argument, 1 .. 4 (a 3x3 .. 9x9 fit in a 5x5 .. 17x17 window)."""
        import torch
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, rs, fs = self._tensor_geometry(frames, fmt, bpp)
        dev = frames.device

        def tensor(t, dtype, shape, what):
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the frames' device" % (what, dtype, shape))
            return t.data_ptr()

        if not (getattr(points, "is_cuda", False) and points.dim() == 3 and points.shape[0] == n and points.shape[2] == 2):
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be a device tensor [N, P, 2]")
        ppf = int(points.shape[1])
        p_points = tensor(points, torch.float32, (n, ppf, 2), "points")
        p_counts = tensor(counts, torch.int32, (n,), "counts") if counts is not None else None
        if (out is None) != (status is None):
            raise AgxError(_ffi.AGX_ERR_ARG, "out and status: both or neither")
        p_out = tensor(out, torch.float32, (n, ppf, 5), "out") if out is not None else None
        p_status = tensor(status, torch.int32, (n, ppf), "status") if status is not None else None
        self._follow_torch_stream(frames)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_refine_points_enqueue_h(self._h, frames.data_ptr(), n, w, h, rs, fs, fmt, self._refine_image(image), p_points,
                                                          ppf, p_counts, p_out, p_status, int(half_size_patch)))
        self._refine = (n, ppf, (frames, points, counts), (out, status) if out is not None else None)

    def refine_points_fetch(self):
        """Wait for refine_points_enqueue's batch -> (records [N,P] SADDLE_DTYPE, status [N,P] uint32); slots beyond a frame's
        count read zero records and status 0xFFFFFFFF.  After refine_points_enqueue(out=, status=): the two device tensors."""
        if self._refine is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no refine batch enqueued")
        n, ppf, _, dev_out = self._refine
        self._refine = None
        self._decode = self._grow = self._find = None
        if dev_out is not None:
            self._check(self._lib.agx_refine_points_fetch(self._h, None, None))
            return dev_out
        out = np.zeros((n, ppf), SADDLE_DTYPE)
        status = np.full((n, ppf), 0xFFFFFFFF, np.uint32)
        self._check(self._lib.agx_refine_points_fetch(self._h, out.ctypes.data, status.ctypes.data))
        return out, status

    def refine_windows_enqueue(self, frames, points, out, status, counts=None, status_in=None, factor=1, half_size_patch=2, format=None):
        """refine_points_enqueue(.., image="blurred") without its blur plane (agx_refine_windows_enqueue): every point's blur window
        is computed from the input pixels around it, so the cost follows the points, not the pixels, and the records and status
        words are the same bytes.  Stream-ordered behind torch's current stream; nothing to fetch.  frames: [N,H,W] uint8 / 16-bit /
        float32 on this detector's GPU, rows and frames may be padded (a view).  points: a float32 device tensor [N,P,K], K >= 2,
        whose rows start with (x, y) -- [N,P,2] points and [N,P,5] records are both read in place.  out float32 [N,P,5] and
        status int32 [N,P]: the results, required.  counts: optional int32 [N].  status_in: optional int32 [N,P]; a slot whose word
        is non-zero is not refined: zero record, the word handed on.  factor 1 .. 4: the points are those of decimate_enqueue(frames,
        factor) and go to full resolution as x * factor + (factor - 1) / 2 in float32 first."""
        import torch
        fmt, n, w, h, rs, fs = self._strided_frames(frames, format)
        dev = frames.device

        def tensor(t, dtype, shape, what):
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the frames' device" % (what, dtype, shape))
            return t.data_ptr()

        if not (getattr(points, "is_cuda", False) and points.dtype == torch.float32 and points.dim() == 3 and points.shape[0] == n
                and points.shape[1] > 0 and points.shape[2] >= 2 and points.stride(2) == 1 and points.stride(1) >= 2
                and (n == 1 or points.stride(0) == points.shape[1] * points.stride(1)) and points.device == dev):
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be a float32 device tensor [N, P, K >= 2] whose rows are evenly spaced")
        ppf = int(points.shape[1])
        p_counts = tensor(counts, torch.int32, (n,), "counts") if counts is not None else None
        p_in = tensor(status_in, torch.int32, (n, ppf), "status_in") if status_in is not None else None
        p_out, p_status = tensor(out, torch.float32, (n, ppf, 5), "out"), tensor(status, torch.int32, (n, ppf), "status")
        self._follow_torch_stream(frames)
        self._enqueued(self._lib.agx_refine_windows_enqueue(self._h, frames.data_ptr(), n, w, h, rs, fs, fmt, points.data_ptr(),
                                                            points.stride(1) * 4, ppf, p_counts, p_in, p_out, p_status, int(factor),
                                                            int(half_size_patch)))

    # ---- try_decode_quad of caller-given quads (src/detector.rs:448-476) --------------------
    def decode_quads(self, image, quads, format=None, with_bits=False):
        """try_decode_quad of every quad of `quads` (n x 4 corners (x, y), any array that reshapes to [n, 8]) on a host image
        of any format but a float32 plane; the saddle chain is not run.  -> (tags [n] TAG_DTYPE, status [n] uint32 AGX_QUAD_*),
        in input order; with_bits: also bit_code's values [n] uint64.  tags[i] is zero unless status[i] == AGX_QUAD_DECODED:
        id = the index into the family's code list, xy = the corners after rotate_left(rotation); reverse() (:467-470)."""
        a, fmt, stride = _image_args(image, format)
        h, w = _image_hw(a, fmt)
        q = np.ascontiguousarray(quads, np.float32).reshape(-1, 8)
        n = q.shape[0]
        out = np.zeros(n, self.TAG_DTYPE)
        status = np.zeros(n, np.uint32)
        bits = np.zeros(n, np.uint64)
        n_decoded = C.c_uint32(0)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_decode_quads(self._h, a.ctypes.data, w, h, stride, fmt, q.ctypes.data, n, out.ctypes.data,
                                               status.ctypes.data, bits.ctypes.data if with_bits else None, C.byref(n_decoded)))
        assert n_decoded.value == int((status == _ffi.AGX_QUAD_DECODED).sum())
        return (out, status, bits) if with_bits else (out, status)

    def decode_quads_enqueue(self, frames, quads=None, counts=None, out=None, status=None, bits=None, refined=None, format=None):
        """try_decode_quad over a batch on this detector's GPU, stream-ordered behind torch's current stream; returns immediately.
        frames and format= as saddles_batch_enqueue (float32 planes are refused).  quads: float32 [N,Q,4,2] (or [N,Q,8]) device
        tensor.  refined=(records, point_status) instead of quads: refine_points_enqueue's out [N,4Q,5] and status [N,4Q] device
        tensors as they are -- that batch need not be fetched first; a quad with a corner that was not refined is
        AGX_QUAD_SKIPPED.  counts: optional int32 [N], the quads of frame f (at most Q; slots beyond are not written).
        out int32 [N,Q,9] (split_device_tags reads it) and status int32 [N,Q]: device-resident results (both or neither),
        bits int64 [N,Q] optionally with them -- without them decode_quads_fetch returns arrays."""
        import torch
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, rs, fs = self._tensor_geometry(frames, fmt, bpp)
        dev = frames.device

        def tensor(t, dtype, shape, what):
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the frames' device" % (what, dtype, shape))
            return t.data_ptr()

        if (quads is None) == (refined is None):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads or refined=(records, point_status): one of them")
        p_point_status = None
        if refined is not None:
            records, point_status = refined
            if not (getattr(records, "is_cuda", False) and records.dim() == 3 and records.shape[0] == n and records.shape[1] % 4 == 0
                    and records.shape[1] > 0 and records.shape[2] == 5):
                raise AgxError(_ffi.AGX_ERR_ARG, "refined records must be a device tensor [N, 4 Q, 5]")
            qpf, stride = int(records.shape[1]) // 4, 20
            p_quads = tensor(records, torch.float32, (n, 4 * qpf, 5), "refined records")
            p_point_status = tensor(point_status, torch.int32, (n, 4 * qpf), "refined point status")
        else:
            if not (getattr(quads, "is_cuda", False) and quads.dim() in (3, 4) and quads.shape[0] == n and quads.shape[1] > 0
                    and tuple(quads.shape[2:]) in ((8,), (4, 2))):
                raise AgxError(_ffi.AGX_ERR_ARG, "quads must be a device tensor [N, Q, 4, 2] or [N, Q, 8]")
            qpf, stride = int(quads.shape[1]), 8
            p_quads = tensor(quads, torch.float32, tuple(quads.shape), "quads")
        p_counts = tensor(counts, torch.int32, (n,), "counts") if counts is not None else None
        if (out is None) != (status is None):
            raise AgxError(_ffi.AGX_ERR_ARG, "out and status: both or neither")
        if bits is not None and out is None:
            raise AgxError(_ffi.AGX_ERR_ARG, "bits goes with out and status (without them decode_quads_fetch returns the bits)")
        p_out = tensor(out, torch.int32, (n, qpf, 9), "out") if out is not None else None
        p_status = tensor(status, torch.int32, (n, qpf), "status") if status is not None else None
        p_bits = tensor(bits, torch.int64, (n, qpf), "bits") if bits is not None else None
        self._follow_torch_stream(frames)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_decode_quads_enqueue(self._h, frames.data_ptr(), n, w, h, rs, fs, fmt, p_quads, stride, qpf, p_counts,
                                                       p_point_status, p_out, p_status, p_bits))
        self._decode = (n, qpf, (frames, quads, refined, counts), (out, status, bits) if out is not None else None)

    def decode_quads_fetch(self):
        """Wait for decode_quads_enqueue's batch -> (tags [N,Q] TAG_DTYPE, status [N,Q] uint32, bits [N,Q] uint64); slots beyond a
        frame's count read zero tags, status 0xFFFFFFFF and bits 0.  After decode_quads_enqueue(out=, status=): those device
        tensors (out, status, bits or None)."""
        if self._decode is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no decode batch enqueued")
        n, qpf, _, dev_out = self._decode
        self._decode = self._grow = self._find = None
        if dev_out is not None:
            self._check(self._lib.agx_decode_quads_fetch(self._h, None, None, None))
            return dev_out
        out = np.zeros((n, qpf), self.TAG_DTYPE)
        status = np.full((n, qpf), 0xFFFFFFFF, np.uint32)
        bits = np.zeros((n, qpf), np.uint64)
        self._check(self._lib.agx_decode_quads_fetch(self._h, out.ctypes.data, status.ctypes.data, bits.ctypes.data))
        return out, status, bits

    # ---- the decode in three stages: decode_positions, bit_code, best_tag (src/detector.rs:42-72, :74-122, :142-169) --------
    def _family_info(self):
        """-> (edge_bits, border_bits, hamming_distance, n_codes) of the handle's family (src/detector.rs:369-405)."""
        e, b, hd, n = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.agx_detector_family_info(self._h, C.byref(e), C.byref(b), C.byref(hd), None, C.byref(n)))
        return e.value, b.value, hd.value, n.value

    @staticmethod
    def _stage_tensor(t, dtype, shape, what, dev, optional=False, where="device tensor %s on the batch's device"):
        if t is None and optional:
            return None
        if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and (shape is None or tuple(t.shape) == shape)
                and t.device == dev):
            raise AgxError(_ffi.AGX_ERR_ARG, ("%s must be a contiguous %s " + where) % (what, dtype, shape))
        return t.data_ptr()

    def _stage_lists(self, saddles, counts, frame_table, point_status):
        """The saddle lists of find_boards_enqueue, grow_boards_enqueue and init_quads_enqueue -> (n, spf, stride, tensor, p_counts,
        p_table, p_point_status): frames, slots per frame, bytes per slot, and `tensor(t, dtype, shape, what)`, the pointer of an
        optional tensor on the saddles' device (None: None)."""
        import torch
        if not (getattr(saddles, "is_cuda", False) and saddles.is_contiguous() and saddles.dtype == torch.float32 and saddles.shape[-1] >= 5):
            raise AgxError(_ffi.AGX_ERR_ARG, "saddles must be a contiguous float32 device tensor [N, S, K >= 5] (or [capacity, K] with frame_table)")
        dev = saddles.device

        def tensor(t, dtype, shape, what):
            return self._stage_tensor(t, dtype, shape, what, dev, optional=True, where="tensor %s on the saddles' device")

        if frame_table is not None:
            if saddles.dim() != 2 or frame_table.dim() != 2 or frame_table.shape[1] != 4:
                raise AgxError(_ffi.AGX_ERR_ARG, "with frame_table [N, 4]: saddles [capacity, K]")
            n, spf, n_slots = int(frame_table.shape[0]), int(saddles.shape[0]), int(saddles.shape[0])
        else:
            if saddles.dim() != 3 or saddles.shape[1] == 0:
                raise AgxError(_ffi.AGX_ERR_ARG, "saddles must be [N, S, K]")
            n, spf = int(saddles.shape[0]), int(saddles.shape[1])
            n_slots = n * spf
        p_table = tensor(frame_table, torch.int32, (n, 4), "frame_table")
        p_counts = tensor(counts, torch.int32, (n,), "counts")
        p_ps = tensor(point_status, torch.int32, None, "point_status")
        if point_status is not None and point_status.numel() != n_slots:
            raise AgxError(_ffi.AGX_ERR_ARG, "point_status: one word per slot")
        return n, spf, 4 * int(saddles.shape[-1]), tensor, p_counts, p_table, p_ps

    def _stage_quads(self, quads, refined):
        """quads [N,Q,4,2] / [N,Q,8], or refined=(records [N,4Q,5], point_status [N,4Q]) -> (n, qpf, stride, p_quads, p_point_status, dev)"""
        import torch
        if (quads is None) == (refined is None):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads or refined=(records, point_status): one of them")
        if refined is not None:
            records, point_status = refined
            if not (getattr(records, "is_cuda", False) and records.dim() == 3 and records.shape[1] % 4 == 0 and records.shape[1] > 0
                    and records.shape[2] == 5):
                raise AgxError(_ffi.AGX_ERR_ARG, "refined records must be a device tensor [N, 4 Q, 5]")
            n, qpf, dev = int(records.shape[0]), int(records.shape[1]) // 4, records.device
            return (n, qpf, 20, self._stage_tensor(records, torch.float32, (n, 4 * qpf, 5), "refined records", dev),
                    self._stage_tensor(point_status, torch.int32, (n, 4 * qpf), "refined point status", dev), dev)
        if not (getattr(quads, "is_cuda", False) and quads.dim() in (3, 4) and quads.shape[1] > 0 and tuple(quads.shape[2:]) in ((8,), (4, 2))):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads must be a device tensor [N, Q, 4, 2] or [N, Q, 8]")
        n, qpf, dev = int(quads.shape[0]), int(quads.shape[1]), quads.device
        return n, qpf, 8, self._stage_tensor(quads, torch.float32, tuple(quads.shape), "quads", dev), None, dev

    def _replaces_batch(self):
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = self._clusters = self._init = None

    def decode_positions_enqueue(self, quads=None, points=None, status=None, img_size=None, border_bits=None, edge_bits=None, margin=0.5,
                                 counts=None, refined=None, model="affine"):
        """decode_positions (src/detector.rs:42-72) of every quad slot, stream-ordered behind torch's current stream; nothing to
        fetch.  quads / refined= / counts as decode_quads_enqueue; img_size=(width, height) the corners are tested against (no
        pixel is read); border_bits, edge_bits default to the family's.  points float32 [N,Q,edge_bits^2,2]: the samples of the
        slots whose status is AGX_QUAD_DECODED, x outer and y inner; status int32 [N,Q]: AGX_QUAD_DECODED / _OUTSIDE / _SKIPPED.
        model: "affine" (tag_affine, src/image_util.rs:39-70: the reference's decode) or "homography" (tag_homography,
        src/image_util.rs:5-37: the projective map through the corners; also AGX_QUAD_DEGENERATE)."""
        import torch
        model = tag_map_model(model)
        n, qpf, stride, p_quads, p_ps, dev = self._stage_quads(quads, refined)
        fam = self._family_info()
        edge = fam[0] if edge_bits is None else int(edge_bits)
        border = fam[1] if border_bits is None else int(border_bits)
        if img_size is None:
            raise AgxError(_ffi.AGX_ERR_ARG, "img_size=(width, height) must be given")
        w, h = int(img_size[0]), int(img_size[1])
        if not (0 <= w < 2 ** 32 and 0 <= h < 2 ** 32) or not 1 <= edge <= 8:
            raise AgxError(_ffi.AGX_ERR_ARG, "img_size within uint32, edge_bits 1 .. 8")
        p_points = self._stage_tensor(points, torch.float32, (n, qpf, edge * edge, 2), "points", dev)
        p_status = self._stage_tensor(status, torch.int32, (n, qpf), "status", dev)
        p_counts = self._stage_tensor(counts, torch.int32, (n,), "counts", dev) if counts is not None else None
        self._follow_torch_stream(points)
        self._replaces_batch()
        if model == _ffi.AGX_TAG_MAP_AFFINE:
            self._check(self._lib.agx_decode_positions_enqueue(self._h, p_quads, stride, n, qpf, p_counts, p_ps, w, h, border, edge, float(margin),
                                                               p_points, p_status))
        else:
            self._check(self._lib.agx_decode_positions_enqueue_m(self._h, p_quads, stride, n, qpf, p_counts, p_ps, w, h, border, edge, float(margin),
                                                                 p_points, p_status, model))

    def tag_maps_enqueue(self, quads=None, maps=None, status=None, side_bits=None, margin=0.5, model="homography", counts=None, refined=None):
        """tag_affine (src/image_util.rs:39-70) or tag_homography (src/image_util.rs:5-37) of every quad slot, stream-ordered behind
        torch's current stream; nothing to fetch.  quads / refined= / counts as decode_positions_enqueue; side_bits in 1 .. 40
        (None: the family's 2 border_bits + edge_bits).  maps float32 [N,Q,3,3] (or [N,Q,9]): the row-major matrix from the source
        square to the image of the slots whose status is AGX_QUAD_DECODED (affine: last row 0, 0, 1; homography: w = 1 at the
        square's centre); status int32 [N,Q]: AGX_QUAD_DECODED / _OUTSIDE / _SKIPPED / _DEGENERATE."""
        import torch
        model = tag_map_model(model)
        n, qpf, stride, p_quads, p_ps, dev = self._stage_quads(quads, refined)
        if side_bits is None:
            fam = self._family_info()
            side_bits = 2 * fam[1] + fam[0]
        if maps is None or tuple(maps.shape) not in ((n, qpf, 3, 3), (n, qpf, 9)):
            raise AgxError(_ffi.AGX_ERR_ARG, "maps must be a device tensor [N, Q, 3, 3] or [N, Q, 9]")
        p_maps = self._stage_tensor(maps, torch.float32, tuple(maps.shape), "maps", dev)
        p_status = self._stage_tensor(status, torch.int32, (n, qpf), "status", dev)
        p_counts = self._stage_tensor(counts, torch.int32, (n,), "counts", dev) if counts is not None else None
        self._follow_torch_stream(maps)
        self._replaces_batch()
        self._check(self._lib.agx_tag_maps_enqueue(self._h, p_quads, stride, n, qpf, p_counts, p_ps, int(side_bits), float(margin), model, p_maps,
                                                   p_status))

    def bit_code_enqueue(self, frames, points, bits, status, counts=None, status_in=None, valid_brightness_threshold=10, max_invalid_bit=3,
                         format=None):
        """bit_code (src/detector.rs:74-122) of ANY sample points, stream-ordered behind torch's current stream; nothing to fetch.
        frames and format= as decode_quads_enqueue; points float32 [N,Q,P,2] with P in 1 .. 64 (decode_positions_enqueue's, or a
        grid of the caller's own).  status_in int32 [N,Q] (optional; may be `status` itself): a slot whose word is non-zero reads
        no pixel and keeps its word.  bits int64 [N,Q]: the first point is the most significant of the P bits, 0 unless
        AGX_QUAD_DECODED; status int32 [N,Q]: AGX_QUAD_DECODED / _OUTSIDE / _LOW_CONTRAST / _AMBIGUOUS."""
        import torch
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, rs, fs = self._tensor_geometry(frames, fmt, bpp)
        dev = frames.device
        if not (getattr(points, "is_cuda", False) and points.dim() == 4 and points.shape[0] == n and points.shape[1] > 0 and points.shape[3] == 2):
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be a device tensor [N, Q, P, 2]")
        qpf, pps = int(points.shape[1]), int(points.shape[2])
        p_points = self._stage_tensor(points, torch.float32, (n, qpf, pps, 2), "points", dev)
        p_bits = self._stage_tensor(bits, torch.int64, (n, qpf), "bits", dev)
        p_status = self._stage_tensor(status, torch.int32, (n, qpf), "status", dev)
        p_counts = self._stage_tensor(counts, torch.int32, (n,), "counts", dev) if counts is not None else None
        p_in = self._stage_tensor(status_in, torch.int32, (n, qpf), "status_in", dev) if status_in is not None else None
        if not 0 <= int(max_invalid_bit) < 2 ** 32:
            raise AgxError(_ffi.AGX_ERR_ARG, "max_invalid_bit is a uint32")
        self._follow_torch_stream(frames)
        self._replaces_batch()
        self._check(self._lib.agx_bit_code_enqueue(self._h, frames.data_ptr(), n, w, h, rs, fs, fmt, p_points, pps, qpf, p_counts, p_in,
                                                   int(valid_brightness_threshold), int(max_invalid_bit), p_bits, p_status))

    def best_tag_enqueue(self, bits, ids, rotations, status, thres=None, codes=None, edge_bits=None, counts=None, status_in=None,
                         quads=None, refined=None, tags=None):
        """best_tag (src/detector.rs:142-169) against ANY code list, stream-ordered behind torch's current stream; nothing to
        fetch.  bits int64 [N,Q]; codes: an int64 device tensor of 1 .. 65535 codes, or None: the family's list; thres (None: the
        family's Hamming distance): a rotation matches at a distance below it; edge_bits (None: the family's).  counts and
        status_in as bit_code_enqueue.  ids, rotations, status int32 [N,Q]: the code's index, the rotation (0 unless
        AGX_QUAD_DECODED) and AGX_QUAD_DECODED / _NO_MATCH.  With quads (or refined=, decode_positions_enqueue's input) and tags
        int32 [N,Q,9]: decode_quads_enqueue's records, {id, corners after rotate_left(rotation); reverse()}."""
        import torch
        if not (getattr(bits, "is_cuda", False) and bits.dim() == 2 and bits.shape[1] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "bits must be a device tensor [N, Q]")
        n, qpf, dev = int(bits.shape[0]), int(bits.shape[1]), bits.device
        fam = self._family_info()
        p_bits = self._stage_tensor(bits, torch.int64, (n, qpf), "bits", dev)
        p_out = [self._stage_tensor(t, torch.int32, (n, qpf), what, dev) for t, what in ((ids, "ids"), (rotations, "rotations"), (status, "status"))]
        p_counts = self._stage_tensor(counts, torch.int32, (n,), "counts", dev) if counts is not None else None
        p_in = self._stage_tensor(status_in, torch.int32, (n, qpf), "status_in", dev) if status_in is not None else None
        p_codes, n_codes = None, 0
        if codes is not None:
            if not (getattr(codes, "is_cuda", False) and codes.dim() == 1):
                raise AgxError(_ffi.AGX_ERR_ARG, "codes must be a one-dimensional int64 device tensor")
            n_codes = int(codes.shape[0])
            p_codes = self._stage_tensor(codes, torch.int64, (n_codes,), "codes", dev)
        p_quads, stride, p_tags = None, 0, None
        if (quads is not None or refined is not None) != (tags is not None):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads (or refined=) and tags: both or neither")
        if tags is not None:
            qn, qq, stride, p_quads, _, _ = self._stage_quads(quads, refined)
            if (qn, qq) != (n, qpf):
                raise AgxError(_ffi.AGX_ERR_ARG, "quads must have the bits' [N, Q]")
            p_tags = self._stage_tensor(tags, torch.int32, (n, qpf, 9), "tags", dev)
        self._follow_torch_stream(bits)
        self._replaces_batch()
        self._check(self._lib.agx_best_tag_enqueue(self._h, p_bits, n * qpf, qpf, p_counts, p_in, fam[2] if thres is None else int(thres),
                                                   p_codes, n_codes, fam[0] if edge_bits is None else int(edge_bits), p_quads, stride,
                                                   *p_out, p_tags))

    def decode_quads_staged(self, frames, quads, *, margin=0.5, valid_brightness_threshold=10, max_invalid_bit=3, thres=None, codes=None,
                            counts=None, format=None, model="affine"):
        """try_decode_quad (src/detector.rs:448-476) as its three stages chained on device tensors with no sync in between --
        decode_positions_enqueue -> bit_code_enqueue -> best_tag_enqueue, one status array handed on in place -- with the crate's
        arguments open: margin, the brightness rules, thres (None: the family's Hamming distance) and codes (None: the family's
        list; else 1 .. 65535 codes, a host array or an int64 device tensor) and model ("affine", or "homography":
        decode_positions_enqueue's).  frames, quads [N,Q,4,2] and counts as decode_quads_enqueue.  At the defaults the result is
        decode_quads_enqueue's, byte for byte.
        -> (tags [N,Q] TAG_DTYPE, status [N,Q] uint32, bits [N,Q] uint64, points [N,Q,edge_bits^2,2] float32) as decode_quads_fetch
        returns them: slots beyond a frame's count read zero tags, status 0xFFFFFFFF, bits 0; the points of a slot whose quad
        gave none are 0."""
        import torch
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, _, _ = self._tensor_geometry(frames, fmt, bpp)
        n, qpf, _, _, _, dev = self._stage_quads(quads, None)
        edge = self._family_info()[0]
        i32 = dict(dtype=torch.int32, device=dev)
        points = torch.zeros((n, qpf, edge * edge, 2), dtype=torch.float32, device=dev)
        status = torch.full((n, qpf), -1, **i32)
        bits = torch.zeros((n, qpf), dtype=torch.int64, device=dev)
        ids, rotations = torch.zeros((n, qpf), **i32), torch.zeros((n, qpf), **i32)
        tags = torch.zeros((n, qpf, 9), **i32)
        if codes is not None and not getattr(codes, "is_cuda", False):
            codes = torch.from_numpy(np.ascontiguousarray(codes, np.uint64).view(np.int64).reshape(-1)).to(dev)
        self.decode_positions_enqueue(quads, points, status, img_size=(int(w), int(h)), margin=margin, counts=counts, model=model)
        self.bit_code_enqueue(frames, points, bits, status, counts=counts, status_in=status, valid_brightness_threshold=valid_brightness_threshold,
                              max_invalid_bit=max_invalid_bit, format=format)
        self.best_tag_enqueue(bits, ids, rotations, status, thres=thres, codes=codes, counts=counts, status_in=status, quads=quads, tags=tags)
        self.sync()
        out = np.ascontiguousarray(tags.cpu().numpy()).view(np.uint32).reshape(n, qpf, 9).copy().view(self.TAG_DTYPE).reshape(n, qpf)
        return out, status.cpu().numpy().view(np.uint32), bits.cpu().numpy().view(np.uint64), points.cpu().numpy()

    # ---- try_find_best_board of caller-given saddle lists (src/detector.rs:588-639) --------
    def find_board(self, saddles, cap=128):
        """try_find_best_board of one host list (SADDLE_DTYPE array, or anything that reshapes to [n, 5] float32: x, y, k, theta,
        phi) on this detector's GPU -> (quads [n_quads, 4] uint32 indices into the list, status AGX_BOARD_*, n_quads).  More than `cap`
        quads: AGX_BOARD_CAPACITY and no rows."""
        return _find_board_call(lambda *a: self._check(self._lib.agx_find_board(self._h, *a)), saddles, cap, self)

    def find_boards_enqueue(self, saddles, counts=None, frame_table=None, point_status=None, quads_per_frame=128, quads=None,
                            quad_points=None, n_quads=None, status=None):
        """try_find_best_board once per frame over saddle lists on this detector's GPU, stream-ordered behind torch's current
        stream; returns immediately.  saddles: float32 device tensor [N, S, K] with K >= 5 (x, y, k, theta, phi first: K = 5 is
        refine_points_enqueue's out), frame f owning counts[f] (int32 [N], optional) of its S slots; or, with frame_table (int32
        [N, 4], saddles_batch_enqueue_to's), the flat [capacity, K] list that call wrote.  point_status: int32, one word per
        slot (refine_points_enqueue's status): only slots whose word is 0 are listed.  quads int32 [N, Q, 4], n_quads int32 [N]
        and status int32 [N]: device-resident results (all or none; Q = quads_per_frame without them); quad_points float32
        [N, Q, 4, 2] optionally -- with n_quads as counts it is decode_quads_enqueue's quads.  Indices are slot numbers
        within the frame."""
        import torch
        n, spf, stride, tensor, p_counts, p_table, p_ps = self._stage_lists(saddles, counts, frame_table, point_status)
        given = [t is not None for t in (quads, n_quads, status)]
        if any(given) != all(given):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads, n_quads and status: all or none")
        qpf = int(quads.shape[1]) if quads is not None and quads.dim() == 3 else int(quads_per_frame)
        p_quads = tensor(quads, torch.int32, (n, qpf, 4), "quads")
        p_n = tensor(n_quads, torch.int32, (n,), "n_quads")
        p_st = tensor(status, torch.int32, (n,), "status")
        p_pts = tensor(quad_points, torch.float32, (n, qpf, 4, 2), "quad_points")
        self._follow_torch_stream(saddles)
        self._replaces_batch()
        self._check(self._lib.agx_find_boards_enqueue(self._h, saddles.data_ptr(), stride, n, spf, p_counts, p_table, p_ps, qpf, p_quads, p_pts,
                                                      p_n, p_st))
        self._find = (n, qpf, (saddles, counts, frame_table, point_status, quad_points),
                      (quads, quad_points, n_quads, status) if quads is not None else None)

    def find_boards_fetch(self, n_threads=0):
        """Wait for find_boards_enqueue's batch and let the host form answer the frames the kernel handed back ->
        (quads [N, Q, 4] uint32, quad_points [N, Q, 4, 2] float32, n_quads [N] uint32, status [N] uint32 AGX_BOARD_*); rows at
        or beyond a frame's count read 0xFFFFFFFF / NaN.  After find_boards_enqueue(quads=, n_quads=, status=): those device
        tensors (quads, quad_points or None, n_quads, status), complete."""
        if self._find is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no find-boards batch enqueued")
        n, qpf, keep, dev_out = self._find
        self._replaces_batch()
        if dev_out is not None:
            self._check(self._lib.agx_find_boards_fetch(self._h, None, None, None, None, n_threads))
            return dev_out
        quads = np.full((n, qpf, 4), 0xFFFFFFFF, np.uint32)
        pts = np.full((n, qpf, 4, 2), np.nan, np.float32)
        n_quads = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint32)
        self._check(self._lib.agx_find_boards_fetch(self._h, quads.ctypes.data, pts.ctypes.data, n_quads.ctypes.data, status.ctypes.data,
                                                    n_threads))
        return quads, pts, n_quads, status

    # ---- boards from the caller's seed quads (src/board.rs:26-112) --------------------------
    def grow_boards_enqueue(self, saddles, seed_quads, quads, n_quads, status, counts=None, frame_table=None, point_status=None,
                            seed_counts=None, spacing_ratio=0.3, stop_score=0, fix_missing=True, quad_points=None, seed_scores=None,
                            best_seed=None):
        """Board::new from every seed quad of every frame at spacing_ratio, the first seed with the highest score out as
        find_boards_enqueue writes its board; stream-ordered behind torch's current stream, returns immediately.  saddles, counts,
        frame_table and point_status as find_boards_enqueue's.  seed_quads int32 [N, S, 4]: slot numbers within the frame (a row of
        find_boards_enqueue's quads is one); seed_counts int32 [N] optionally.  quads int32 [N, Q, 4], n_quads and status int32 [N]:
        the device-resident results (required); quad_points float32 [N, Q, 4, 2], seed_scores int32 [N, S] and best_seed int32 [N]
        optionally.  stop_score > 0: no seed is grown behind the first one that leaves the best score at or above it."""
        import torch
        n, spf, stride, tensor, p_counts, p_table, p_ps = self._stage_lists(saddles, counts, frame_table, point_status)
        if seed_quads is None or seed_quads.dim() != 3 or quads is None or quads.dim() != 3:
            raise AgxError(_ffi.AGX_ERR_ARG, "seed_quads [N, S, 4] and quads [N, Q, 4]")
        seeds, qpf = int(seed_quads.shape[1]), int(quads.shape[1])
        p_seeds, p_seed_counts = tensor(seed_quads, torch.int32, (n, seeds, 4), "seed_quads"), tensor(seed_counts, torch.int32, (n,), "seed_counts")
        outs = (tensor(quads, torch.int32, (n, qpf, 4), "quads"), tensor(quad_points, torch.float32, (n, qpf, 4, 2), "quad_points"),
                tensor(n_quads, torch.int32, (n,), "n_quads"), tensor(status, torch.int32, (n,), "status"),
                tensor(seed_scores, torch.int32, (n, seeds), "seed_scores"), tensor(best_seed, torch.int32, (n,), "best_seed"))
        self._follow_torch_stream(saddles)
        rc = self._lib.agx_grow_boards_enqueue(self._h, saddles.data_ptr(), stride, n, spf, p_counts, p_table, p_ps, p_seeds, seeds, p_seed_counts,
                                               float(spacing_ratio), int(stop_score), _ffi.AGX_GROW_FIX_MISSING if fix_missing else 0, qpf, *outs)
        if rc == _ffi.AGX_OK:  # (a refused argument leaves the batch in flight where it is)
            self._replaces_batch()
            self._grow = (saddles, counts, frame_table, point_status, seed_quads, seed_counts, quads, quad_points, n_quads, status, seed_scores,
                          best_seed)
        self._check(rc)

    def grow_boards_fetch(self, n_threads=0):
        """Wait for grow_boards_enqueue's batch and let the host form answer the frames the kernel handed back: the device tensors
        that call was given are complete when this returns."""
        if self._grow is not None:  # in flight: the library resolves it whatever it returns
            self._replaces_batch()
        self._check(self._lib.agx_grow_boards_fetch(self._h, n_threads))

    # ---- candidate quads of caller-given seed saddles (src/detector.rs:543-586) -------------------
    def init_quads_enqueue(self, saddles, quads, n_quads, status, seed_saddles=None, seed_counts=None, seeds_per_frame=None, n_nearest=50,
                           counts=None, frame_table=None, point_status=None, quad_points=None, seed_quad_counts=None, seeds_out=None,
                           n_seeds_out=None):
        """init_quads of every seed saddle of every frame, seed i's quads behind seed i - 1's; stream-ordered behind torch's current
        stream, returns immediately.  saddles, counts, frame_table and point_status as find_boards_enqueue's.  seed_saddles int32
        [N, S]: slot numbers within the frame (seed_counts int32 [N] optionally), or None: the reference's own seeds, at most
        seeds_per_frame of them (default 30, the reference's bound).  quads int32 [N, Q, 4], n_quads and status int32 [N]: the
        device-resident results (required) -- quads with n_quads are grow_boards_enqueue's seed_quads with seed_counts as they
        stand; quad_points float32 [N, Q, 4, 2], seed_quad_counts and seeds_out int32 [N, S], n_seeds_out int32 [N] optionally."""
        import torch
        n, spf, stride, tensor, p_counts, p_table, p_ps = self._stage_lists(saddles, counts, frame_table, point_status)
        if quads is None or quads.dim() != 3 or (seed_saddles is not None and seed_saddles.dim() != 2):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads [N, Q, 4] and seed_saddles [N, S]")
        if seed_saddles is not None:
            seeds = int(seed_saddles.shape[1])
        else:
            seeds = 30 if seeds_per_frame is None else int(seeds_per_frame)
        qpf = int(quads.shape[1])
        p_seeds, p_seed_counts = tensor(seed_saddles, torch.int32, (n, seeds), "seed_saddles"), tensor(seed_counts, torch.int32, (n,), "seed_counts")
        outs = (tensor(quads, torch.int32, (n, qpf, 4), "quads"), tensor(quad_points, torch.float32, (n, qpf, 4, 2), "quad_points"),
                tensor(n_quads, torch.int32, (n,), "n_quads"), tensor(status, torch.int32, (n,), "status"),
                tensor(seed_quad_counts, torch.int32, (n, seeds), "seed_quad_counts"), tensor(seeds_out, torch.int32, (n, seeds), "seeds_out"),
                tensor(n_seeds_out, torch.int32, (n,), "n_seeds_out"))
        self._follow_torch_stream(saddles)
        rc = self._lib.agx_init_quads_enqueue(self._h, saddles.data_ptr(), stride, n, spf, p_counts, p_table, p_ps, p_seeds, seeds, p_seed_counts,
                                              int(n_nearest), qpf, *outs)
        if rc == _ffi.AGX_OK:  # (a refused argument leaves the batch in flight where it is)
            self._replaces_batch()
            self._init = (saddles, counts, frame_table, point_status, seed_saddles, seed_counts, quads, quad_points, n_quads, status,
                          seed_quad_counts, seeds_out, n_seeds_out)
        self._check(rc)

    def init_quads_fetch(self, n_threads=0):
        """Wait for init_quads_enqueue's batch and let the host form answer the frames the kernel handed back: the device tensors
        that call was given are complete when this returns."""
        if self._init is not None:  # in flight: the library resolves it whatever it returns
            self._replaces_batch()
        self._check(self._lib.agx_init_quads_fetch(self._h, n_threads))

    # ---- caller points snapped to the nearest listed saddle (agx_snap_points_enqueue) -----------
    def snap_points_enqueue(self, saddles, points, slots, rows, n_rows, status, max_dist_sq, counts=None, frame_table=None, point_status=None,
                            row_counts=None, reverse=False, dist_sq=None, row_index=None):
        """Every caller point to the nearest listed saddle of its frame (squared distance in binary32, the lowest slot at equal
        distance, taken if it is <= max_dist_sq), stream-ordered behind torch's current stream; nothing to fetch.  saddles, counts,
        frame_table and point_status as find_boards_enqueue's.  points: float32 [N, R, P, 2] with P in 1 .. 4 -- or a tag table,
        int32 [N, R, 9] as collect_tags_enqueue and detect_batch_enqueue(out=...) leave it, whose corners are read in place (P = 4;
        with reverse=True they are a quad in init_quads' winding); row_counts int32 [N] optionally.  slots int32 [N, R, P]: the
        slot within the frame or -1 (AGX_SNAP_NONE), in the order read; rows int32 [N, R, P] with n_rows int32 [N]: the rows whose
        points all snapped to distinct slots, compacted -- grow_boards_enqueue's seed_quads / seed_counts (P = 4) or
        init_quads_enqueue's seed_saddles / seed_counts (P = 1; pass rows.view(N, R)) as they stand; status int32 [N]: AGX_SNAP_*.
        dist_sq float32 [N, R, P] and row_index int32 [N, R] optionally."""
        import torch
        n, spf, stride, tensor, p_counts, p_table, p_ps = self._stage_lists(saddles, counts, frame_table, point_status)
        ok = getattr(points, "is_cuda", False) and points.is_contiguous() and points.device == saddles.device and points.shape[0] == n
        if ok and points.dtype == torch.int32 and points.dim() == 3 and points.shape[2] == 9 and points.shape[1] > 0:
            rpf, ppr, p_points, row_stride = int(points.shape[1]), 4, points.data_ptr() + 4, 36
        elif ok and points.dtype == torch.float32 and points.dim() == 4 and points.shape[3] == 2 and points.shape[1] > 0 and 1 <= points.shape[2] <= 4:
            rpf, ppr, p_points = int(points.shape[1]), int(points.shape[2]), points.data_ptr()
            row_stride = 8 * ppr
        else:
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be a contiguous device tensor on the saddles' device: float32 [N, R, 1..4, 2] or a tag table int32 [N, R, 9]")
        if slots is None or rows is None or n_rows is None or status is None:
            raise AgxError(_ffi.AGX_ERR_ARG, "slots, rows, n_rows and status must be given")
        outs = (tensor(slots, torch.int32, (n, rpf, ppr), "slots"), tensor(dist_sq, torch.float32, (n, rpf, ppr), "dist_sq"),
                tensor(rows, torch.int32, (n, rpf, ppr), "rows"), tensor(n_rows, torch.int32, (n,), "n_rows"),
                tensor(row_index, torch.int32, (n, rpf), "row_index"), tensor(status, torch.int32, (n,), "status"))
        p_row_counts = tensor(row_counts, torch.int32, (n,), "row_counts")
        self._follow_torch_stream(saddles)
        rc = self._lib.agx_snap_points_enqueue(self._h, saddles.data_ptr(), stride, n, spf, p_counts, p_table, p_ps, p_points, row_stride, 8, rpf, ppr,
                                               p_row_counts, float(max_dist_sq), _ffi.AGX_SNAP_REVERSE if reverse else 0, *outs)
        if rc == _ffi.AGX_OK:  # (a refused argument leaves the batch in flight where it is)
            self._replaces_batch()
        self._check(rc)

    # ---- the board's homography from the tag table (agx_board_fit_enqueue) -----------------------
    @staticmethod
    def board_fit(tags, cols, rows, img_size, **kw):
        """The host form for one frame, no device needed: the module's board_fit."""
        return board_fit(tags, cols, rows, img_size, **kw)

    def board_fit_enqueue(self, tags, n_tags, cols, rows, img_size, h, err_sq, row_status, n_inliers, rms, pred, n_pred, status, first_id=0,
                          spacing_ratio=0.3, max_err_sq=4.0, max_drop=0, min_tags=1, predict_missing=False, tag_status=None):
        """Per frame the homography from the printed board to the image through every corner of the frame's tag table, its
        outlier rounds and the predicted corners of the layout's tags (board_fit, the host form, says what is computed), in
        device tensors and stream-ordered behind torch's current stream; nothing to fetch.  tags int32 [N, T, 9], n_tags and
        tag_status (optional) int32 [N]: the tables of collect_tags_enqueue / detect_batch_enqueue(out=...), read in place.
        h float64 [N, 9]; err_sq float32 and row_status int32 [N, T]; n_inliers int32, rms float32, n_pred, status int32 [N];
        pred int32 [N, rows*cols, 9]: tag rows as snap_points_enqueue reads them in place (row_counts = n_pred)."""
        import torch
        if not (getattr(tags, "is_cuda", False) and tags.dtype == torch.int32 and tags.is_contiguous() and tags.dim() == 3 and tags.shape[2] == 9
                and tags.shape[1] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "tags must be a contiguous int32 device tensor [N, T, 9]")
        n, tpf, dev = int(tags.shape[0]), int(tags.shape[1]), tags.device
        n_board = int(cols) * int(rows)

        def tensor(t, dtype, shape, what, optional=False):
            if t is None and optional:
                return None
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the tags' device" % (what, dtype, shape))
            return t.data_ptr()

        ins = (tensor(n_tags, torch.int32, (n,), "n_tags"), tensor(tag_status, torch.int32, (n,), "tag_status", optional=True))
        outs = (tensor(h, torch.float64, (n, 9), "h"), tensor(err_sq, torch.float32, (n, tpf), "err_sq"),
                tensor(row_status, torch.int32, (n, tpf), "row_status"), tensor(n_inliers, torch.int32, (n,), "n_inliers"),
                tensor(rms, torch.float32, (n,), "rms"), tensor(pred, torch.int32, (n, n_board, 9), "pred"),
                tensor(n_pred, torch.int32, (n,), "n_pred"), tensor(status, torch.int32, (n,), "status"))
        self._follow_torch_stream(tags)
        rc = self._lib.agx_board_fit_enqueue(self._h, n, tags.data_ptr(), tpf, *ins, int(cols), int(rows), int(first_id), float(spacing_ratio),
                                             int(img_size[0]), int(img_size[1]), float(max_err_sq), int(max_drop), int(min_tags),
                                             _ffi.AGX_FIT_PREDICT_MISSING if predict_missing else 0, *outs)
        if rc == _ffi.AGX_OK:  # (a refused argument leaves the batch in flight where it is)
            self._replaces_batch()
        self._check(rc)

    # ---- the board's pose under a lens model (agx_board_pose_enqueue) --------------------------------
    @staticmethod
    def board_pose(tags, cols, rows, camera, **kw):
        """The host form for one frame, no device needed: the module's board_pose."""
        return board_pose(tags, cols, rows, camera, **kw)

    def board_pose_enqueue(self, tags, n_tags, cols, rows, camera, pose, err_sq, row_status, n_inliers, rms, best_iter, pred, n_pred, status,
                           tag_size=1.0, first_id=0, spacing_ratio=0.3, max_err_sq=4.0, max_drop=0, min_tags=1, iterations=10,
                           predict_missing=False, tag_status=None):
        """Per frame the pose of the printed board in the camera frame under `camera` (a Camera: pinhole + radial-tangential, or
        Camera.equidistant's fisheye or Camera.double_sphere's model -- the camera's model attribute picks the kernel)
        through every corner of the frame's tag table, its outlier rounds and the predicted corners of the layout's tags through
        the lens model (board_pose, the host form, says what is computed), in device tensors and stream-ordered behind torch's
        current stream; nothing to fetch.  tags, n_tags, tag_status and err_sq, row_status, n_inliers, rms, pred, n_pred, status
        as board_fit_enqueue's; pose float64 [N, 12] (R row major, then t); best_iter int32 [N]."""
        import torch
        if not (getattr(tags, "is_cuda", False) and tags.dtype == torch.int32 and tags.is_contiguous() and tags.dim() == 3 and tags.shape[2] == 9
                and tags.shape[1] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "tags must be a contiguous int32 device tensor [N, T, 9]")
        n, tpf, dev = int(tags.shape[0]), int(tags.shape[1]), tags.device
        n_board = int(cols) * int(rows)

        def tensor(t, dtype, shape, what, optional=False):
            if t is None and optional:
                return None
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the tags' device" % (what, dtype, shape))
            return t.data_ptr()

        ins = (tensor(n_tags, torch.int32, (n,), "n_tags"), tensor(tag_status, torch.int32, (n,), "tag_status", optional=True))
        outs = (tensor(pose, torch.float64, (n, 12), "pose"), tensor(err_sq, torch.float32, (n, tpf), "err_sq"),
                tensor(row_status, torch.int32, (n, tpf), "row_status"), tensor(n_inliers, torch.int32, (n,), "n_inliers"),
                tensor(rms, torch.float32, (n,), "rms"), tensor(best_iter, torch.int32, (n,), "best_iter"),
                tensor(pred, torch.int32, (n, n_board, 9), "pred"), tensor(n_pred, torch.int32, (n,), "n_pred"),
                tensor(status, torch.int32, (n,), "status"))
        model, cam = _camera(camera)
        self._follow_torch_stream(tags)
        head = (self._h, n, tags.data_ptr(), tpf, *ins, int(cols), int(rows), int(first_id), float(spacing_ratio), float(tag_size))
        rest = (cam, float(max_err_sq), int(max_drop), int(min_tags), int(iterations), _ffi.AGX_FIT_PREDICT_MISSING if predict_missing else 0, *outs)
        if model == _ffi.AGX_LENS_RADTAN:  # (the call of a radial-tangential camera is the one it was)
            rc = self._lib.agx_board_pose_enqueue(*head, *rest)
        else:
            rc = self._lib.agx_board_pose_enqueue_m(*head, model, *rest)
        if rc == _ffi.AGX_OK:  # (a refused argument leaves the batch in flight where it is)
            self._replaces_batch()
        self._check(rc)

    # ---- the camera from the batch (agx_calibrate_enqueue) ---------------------------------------------------------------------
    @staticmethod
    def calibrate(tags, n_tags, cols, rows, camera, poses, row_status, fit_status, **kw):
        """The host form, no device needed: the module's calibrate."""
        return calibrate(tags, n_tags, cols, rows, camera, poses, row_status, fit_status, **kw)

    @staticmethod
    def calibrate_seed(h, fit_status, img_size):
        """The closed-form seed, host only: the module's calibrate_seed."""
        return calibrate_seed(h, fit_status, img_size)

    def calibrate_enqueue(self, tags, n_tags, cols, rows, camera, pose_in, row_status, fit_status, camera_out, pose, frame_cost, frame_n, report,
                          tag_size=1.0, first_id=0, spacing_ratio=0.3, fixed=0, damping=0.0, iterations=10, min_tags=1, min_frames=1,
                          accept_loose=False, tag_status=None):
        """The camera's nine doubles and every usable frame's pose from a batch of tag tables (calibrate, the host form, says what
        is computed), in device tensors and stream-ordered behind torch's current stream; nothing to fetch.  tags, n_tags,
        tag_status as board_pose_enqueue's; pose_in float64 [N, 12], row_status int32 [N, T] and fit_status int32 [N] are its pose,
        row_status and status, read in place.  camera: the seed (host).  camera_out float64 [9]; pose float64 [N, 12] (may be
        pose_in); frame_cost float32 [N]; frame_n int32 [N]; report float64 [69], read with calib_report()."""
        import torch
        if not (getattr(tags, "is_cuda", False) and tags.dtype == torch.int32 and tags.is_contiguous() and tags.dim() == 3 and tags.shape[2] == 9
                and tags.shape[1] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "tags must be a contiguous int32 device tensor [N, T, 9]")
        n, tpf, dev = int(tags.shape[0]), int(tags.shape[1]), tags.device

        def tensor(t, dtype, shape, what, optional=False):
            if t is None and optional:
                return None
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the tags' device" % (what, dtype, shape))
            return t.data_ptr()

        ins = (tensor(n_tags, torch.int32, (n,), "n_tags"), tensor(tag_status, torch.int32, (n,), "tag_status", optional=True))
        state = (tensor(pose_in, torch.float64, (n, 12), "pose_in"), tensor(row_status, torch.int32, (n, tpf), "row_status"),
                 tensor(fit_status, torch.int32, (n,), "fit_status"))
        outs = (tensor(camera_out, torch.float64, (9,), "camera_out"), tensor(pose, torch.float64, (n, 12), "pose"),
                tensor(frame_cost, torch.float32, (n,), "frame_cost"), tensor(frame_n, torch.int32, (n,), "frame_n"),
                tensor(report, torch.float64, (69,), "report"))
        model, cam = _camera(camera)
        self._follow_torch_stream(tags)
        rc = self._lib.agx_calibrate_enqueue(self._h, n, tags.data_ptr(), tpf, *ins, int(cols), int(rows), int(first_id), float(spacing_ratio),
                                             float(tag_size), model, cam, _fixed_mask(fixed), float(damping), int(iterations), int(min_tags),
                                             int(min_frames), _ffi.AGX_CALIB_ACCEPT_LOOSE if accept_loose else 0, *state, *outs)
        self._enqueued(rc)

    def calibrate_batch(self, frames, cols, rows, tag_size=1.0, lens="radtan", camera=None, fixed=0, rounds=3, iterations=10, damping=None,
                        first_id=0, spacing_ratio=0.3, cap=None, max_err_sq=4.0, max_drop=0, min_tags=1, min_frames=1, accept_loose=True,
                        pose_iterations=10, format=None):
        """A camera from a batch of frames resident on this detector's GPU, every stage on the device: detect_batch_enqueue(out=)
        -> board_fit_enqueue -> calibrate_seed -> `rounds` x (board_pose_enqueue with its outlier rounds -> calibrate_enqueue).
        camera: the seed; None: calibrate_seed's pinhole under the model `lens` names ("radtan", "equidistant" or "double_sphere";
        a double-sphere seed is that pinhole at xi = 0, alpha = 0.5).  With a camera given, its own model counts and `lens` is
        not read.  damping: None is 0, and 1e-6 under the double-sphere model (_seed_damping says why).
        The frames' tables, poses and masks stay on the device.  Read back between the stages: the seed's homographies and status
        words once; per round the nine doubles and the 552-byte report; at the end the pose call's status words and the frames'
        corner counts for the report.
        -> (Camera, poses float64 [N, 12] on the device (frames that were not usable keep the pose call's rows), report: the last
        round's calib_report() with pose_status, the pose call's status words, and frame_n)."""
        import torch
        n, h, w = int(frames.shape[0]), int(frames.shape[-2] if frames.dim() == 3 else frames.shape[1]), int(frames.shape[-1] if frames.dim() == 3 else frames.shape[2])
        n_board = int(cols) * int(rows)
        cap = n_board if cap is None else int(cap)
        dev = frames.device
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        tags, counts, status = i32(n, cap, 9), i32(n), i32(n)
        self.detect_batch_enqueue(frames, cap, out=(tags, counts, status), format=format)
        self.detect_batch_fetch(raise_on_overflow=False)
        err, rst, n_inl, rms, pred, n_pred, fst = f32(n, cap), i32(n, cap), i32(n), f32(n), i32(n, n_board, 9), i32(n), i32(n)
        layout = dict(first_id=first_id, spacing_ratio=spacing_ratio)
        if camera is None:
            hs = f64(n, 9)
            self.board_fit_enqueue(tags, counts, cols, rows, (w, h), hs, err, rst, n_inl, rms, pred, n_pred, fst, max_err_sq=max_err_sq,
                                   max_drop=max_drop, min_tags=min_tags, tag_status=status, **layout)
            torch.cuda.current_stream(dev).synchronize()
            seed = calibrate_seed(hs.cpu().numpy(), fst.cpu().numpy().astype(np.uint32), (w, h))
            if seed["status"] != _ffi.AGX_CALIB_OK:
                raise AgxError(_ffi.AGX_ERR_STATE, "calibrate_batch: the seed is AGX_CALIB_%s" % ("FEW" if seed["status"] == _ffi.AGX_CALIB_FEW else "SINGULAR"))
            camera = _lens_seed(lens, seed["camera"])
        pose, best, cam_out, fcost, fn, rep = f64(n, 12), i32(n), f64(9), f32(n), i32(n), f64(69)
        report, damping = None, _seed_damping(camera, damping)
        for _ in range(int(rounds)):
            self.board_pose_enqueue(tags, counts, cols, rows, camera, pose, err, rst, n_inl, rms, best, pred, n_pred, fst, tag_size=tag_size,
                                    max_err_sq=max_err_sq, max_drop=max_drop, min_tags=min_tags, iterations=pose_iterations, tag_status=status,
                                    **layout)
            self.calibrate_enqueue(tags, counts, cols, rows, camera, pose, rst, fst, cam_out, pose, fcost, fn, rep, tag_size=tag_size, fixed=fixed,
                                   damping=damping, iterations=iterations, min_tags=min_tags, min_frames=min_frames, accept_loose=accept_loose,
                                   tag_status=status, **layout)
            torch.cuda.current_stream(dev).synchronize()
            report = calib_report(rep.cpu().numpy())
            if report["status"] != _ffi.AGX_CALIB_OK:
                break
            camera = type(camera)(*cam_out.cpu().numpy().tolist()) if isinstance(camera, Camera) else Camera(*cam_out.cpu().numpy().tolist())
        if report is not None:
            report["pose_status"] = fst.cpu().numpy()
            report["frame_n"] = fn.cpu().numpy()
        return camera, pose, report

    # ---- the rig from the batch (agx_rig_calibrate_enqueue) -------------------------------------------------------------------
    @staticmethod
    def rig_calibrate(tags, n_tags, cols, rows, cameras, poses, row_status, fit_status, extrinsics, **kw):
        """The host form, no device needed: the module's rig_calibrate."""
        return rig_calibrate(tags, n_tags, cols, rows, cameras, poses, row_status, fit_status, extrinsics, **kw)

    @staticmethod
    def rig_seed(poses, fit_status, frame_n=None):
        """The closed-form seed, host only: the module's rig_seed."""
        return rig_seed(poses, fit_status, frame_n)

    def rig_calibrate_enqueue(self, tags, n_tags, cols, rows, cameras, pose_in, row_status, fit_status, extrinsics_in, extrinsics, rig_pose,
                              frame_cost, frame_n, cam_n, report, tag_size=1.0, first_id=0, spacing_ratio=0.3, damping=0.0, iterations=10,
                              min_tags=1, min_cams=2, min_instants=1, accept_loose=False, tag_status=None):
        """The extrinsics of a rig's cameras and the board's pose at every usable instant from synchronised tag tables
        (rig_calibrate, the host form, says what is computed), in device tensors and stream-ordered behind torch's current stream;
        nothing to fetch.  tags int32 [C, S, T, 9] (camera c at instant s), n_tags and fit_status int32 [C, S], row_status int32
        [C, S, T], pose_in float64 [C, S, 12]: the pose call's tables and answers per camera, read in place (tag_status int32
        [C, S] or None).  cameras: C Cameras (host), held.  extrinsics_in float64 [C, 12]: the seed (rig_seed), may be
        extrinsics itself.  extrinsics float64 [C, 12]; rig_pose float64 [S, 12]; frame_cost float32 [C, S]; frame_n int32
        [C, S]; cam_n int32 [C]; report float64 [70], read with rig_report()."""
        import torch
        if not (getattr(tags, "is_cuda", False) and tags.dtype == torch.int32 and tags.is_contiguous() and tags.dim() == 4 and tags.shape[3] == 9
                and tags.shape[2] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "tags must be a contiguous int32 device tensor [C, S, T, 9]")
        nc, ns, tpf, dev = int(tags.shape[0]), int(tags.shape[1]), int(tags.shape[2]), tags.device

        def tensor(t, dtype, shape, what, optional=False):
            if t is None and optional:
                return None
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the tags' device" % (what, dtype, shape))
            return t.data_ptr()

        ins = (tensor(n_tags, torch.int32, (nc, ns), "n_tags"), tensor(tag_status, torch.int32, (nc, ns), "tag_status", optional=True))
        state = (tensor(pose_in, torch.float64, (nc, ns, 12), "pose_in"), tensor(row_status, torch.int32, (nc, ns, tpf), "row_status"),
                 tensor(fit_status, torch.int32, (nc, ns), "fit_status"), tensor(extrinsics_in, torch.float64, (nc, 12), "extrinsics_in"))
        outs = (tensor(extrinsics, torch.float64, (nc, 12), "extrinsics"), tensor(rig_pose, torch.float64, (ns, 12), "rig_pose"),
                tensor(frame_cost, torch.float32, (nc, ns), "frame_cost"), tensor(frame_n, torch.int32, (nc, ns), "frame_n"),
                tensor(cam_n, torch.int32, (nc,), "cam_n"), tensor(report, torch.float64, (70,), "report"))
        models, cams = _rig_cameras(cameras, nc)
        self._follow_torch_stream(tags)
        rc = self._lib.agx_rig_calibrate_enqueue(self._h, nc, ns, tags.data_ptr(), tpf, *ins, int(cols), int(rows), int(first_id), float(spacing_ratio),
                                                 float(tag_size), models, cams, float(damping), int(iterations), int(min_tags), int(min_cams),
                                                 int(min_instants), _ffi.AGX_CALIB_ACCEPT_LOOSE if accept_loose else 0, *state, *outs)
        self._enqueued(rc)

    def rig_calibrate_batch(self, frames, cols, rows, cameras, tag_size=1.0, rounds=2, iterations=10, damping=0.0, first_id=0, spacing_ratio=0.3,
                            cap=None, max_err_sq=4.0, max_drop=0, min_tags=1, min_cams=2, min_instants=1, accept_loose=True, pose_iterations=10,
                            format=None):
        """A rig's extrinsics from frames [C, S, H, W] resident on this detector's GPU (camera c at instant s), every stage on the
        device: detect_batch_enqueue(out=) on the stacked batch -> `rounds` x (one board_pose_enqueue per camera on its slice, whose
        rounds mark the outliers -> rig_calibrate_enqueue).  cameras: C calibrated Cameras, held.  Read back: the poses and status
        words for rig_seed in the first round only, and the 560-byte report per round.  Each round's extrinsics seed the next.
        -> (extrinsics float64 [C, 12] and rig poses float64 [S, 12] on the device, report: the last round's rig_report() with
        cam_status (rig_seed's), cam_n, frame_n and pose_status)."""
        import torch
        if frames.dim() != 4:
            raise AgxError(_ffi.AGX_ERR_ARG, "frames must be [C, S, H, W]")
        nc, ns = int(frames.shape[0]), int(frames.shape[1])
        n, n_board = nc * ns, int(cols) * int(rows)
        cap = n_board if cap is None else int(cap)
        dev = frames.device
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        tags, counts, status = i32(n, cap, 9), i32(n), i32(n)
        self.detect_batch_enqueue(frames.reshape(n, int(frames.shape[2]), int(frames.shape[3])), cap, out=(tags, counts, status), format=format)
        self.detect_batch_fetch(raise_on_overflow=False)
        err, rst, n_inl, rms, best, pred, n_pred, fst = f32(n, cap), i32(n, cap), i32(n), f32(n), i32(n), i32(n, n_board, 9), i32(n), i32(n)
        pose, ext, rig_pose, fcost, fn, cam_n, rep = f64(n, 12), f64(nc, 12), f64(ns, 12), f32(nc, ns), i32(nc, ns), i32(nc), f64(70)
        layout = dict(first_id=first_id, spacing_ratio=spacing_ratio)
        report, cam_status = None, None
        for rnd in range(int(rounds)):
            for c in range(nc):
                k = slice(c * ns, (c + 1) * ns)
                self.board_pose_enqueue(tags[k], counts[k], cols, rows, cameras[c], pose[k], err[k], rst[k], n_inl[k], rms[k], best[k], pred[k],
                                        n_pred[k], fst[k], tag_size=tag_size, max_err_sq=max_err_sq, max_drop=max_drop, min_tags=min_tags,
                                        iterations=pose_iterations, tag_status=status[k], **layout)
            if rnd == 0:
                torch.cuda.current_stream(dev).synchronize()
                seed = rig_seed(pose.cpu().numpy().reshape(nc, ns, 12), fst.cpu().numpy().astype(np.uint32).reshape(nc, ns),
                                n_inl.cpu().numpy().astype(np.uint32).reshape(nc, ns))
                cam_status = seed["cam_status"]
                ext.copy_(torch.from_numpy(seed["extrinsics"]))
            self.rig_calibrate_enqueue(tags.view(nc, ns, cap, 9), counts.view(nc, ns), cols, rows, cameras, pose.view(nc, ns, 12), rst.view(nc, ns, cap),
                                       fst.view(nc, ns), ext, ext, rig_pose, fcost, fn, cam_n, rep, tag_size=tag_size, damping=damping,
                                       iterations=iterations, min_tags=min_tags, min_cams=min_cams, min_instants=min_instants,
                                       accept_loose=accept_loose, tag_status=status.view(nc, ns), **layout)
            torch.cuda.current_stream(dev).synchronize()
            report = rig_report(rep.cpu().numpy())
            if report["status"] != _ffi.AGX_RIG_OK:
                break
        if report is not None:
            report.update(cam_status=cam_status, cam_n=cam_n.cpu().numpy(), frame_n=fn.cpu().numpy(), pose_status=fst.cpu().numpy().reshape(nc, ns))
        return ext, rig_pose, report

    # ---- rectified batches: the lens model applied to the pixels (csrc/rectify.hip) ------------------------------------------
    def _enqueued(self, rc):
        if rc == _ffi.AGX_OK:  # (a refused argument leaves the batch in flight where it is)
            self._replaces_batch()
        self._check(rc)

    def rectify_map_enqueue(self, camera, src_size, dst_size=None, new_camera=None, rotation=None, out=None):
        """rectify_map (the host form says what is computed) on the device, stream-ordered behind torch's current stream; nothing
        to fetch.  -> the map, an int32 device tensor [dst_h, dst_w, 2]; out: the caller's (rows may be padded: stride(0) even,
        stride(1) = 2, stride(2) = 1)."""
        import torch
        model, cam, ncam, rot, (sw, sh), (dw, dh) = _rectify_args(camera, src_size, dst_size, new_camera, rotation)
        if out is None:
            if not (1 <= dw <= 16384 and 1 <= dh <= 16384):
                raise AgxError(_ffi.AGX_ERR_ARG, "dst_size must be in 1 .. 16384")
            out = torch.empty((dh, dw, 2), dtype=torch.int32, device="cuda:%d" % self.device)
        elif not (getattr(out, "is_cuda", False) and out.dtype == torch.int32 and tuple(out.shape) == (dh, dw, 2) and out.stride(2) == 1
                  and out.stride(1) == 2 and out.device.index == self.device):
            raise AgxError(_ffi.AGX_ERR_ARG, "out must be an int32 tensor [dst_h, dst_w, 2] on the detector's device whose rows are packed")
        self._follow_torch_stream(out)
        self._enqueued(self._lib.agx_rectify_map_enqueue(self._h, model, cam, ncam, rot, sw, sh, dw, dh, out.data_ptr(),
                                                         (out.stride(0) if dh > 1 else 2 * dw) * 4))
        return out

    @staticmethod
    def _gray_batch(t, what):
        """-> (agx_format, pixel bytes) of a device tensor [N, H, W] uint8 / int16 / uint16 whose pixels of a row are adjacent."""
        import torch
        if not (getattr(t, "is_cuda", False) and t.dim() == 3 and t.stride(2) == 1 and min(t.shape) > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a device tensor [N, H, W] with adjacent pixels in a row" % what)
        if t.dtype == torch.uint8:
            return _ffi.AGX_L8, 1
        if t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
            return _ffi.AGX_L16, 2
        raise AgxError(_ffi.AGX_ERR_ARG, "%s must be uint8 (AGX_L8) or 16-bit (AGX_L16)" % what)

    def remap_enqueue(self, frames, map, out=None, border=0):
        """remap (the host form says what is computed) of a device batch [N, H, W] uint8 / 16-bit through `map` (an int32 device
        tensor [dst_h, dst_w, 2]: rectify_map_enqueue's, or the caller's own) into out [N, dst_h, dst_w] of the same dtype (made if
        None), stream-ordered behind torch's current stream; nothing to fetch.  frames, map and out may be views with padded rows
        and frames.  -> out."""
        import torch
        fmt, px = self._gray_batch(frames, "frames")
        if not (getattr(map, "is_cuda", False) and map.dtype == torch.int32 and map.dim() == 3 and map.shape[2] == 2 and map.stride(2) == 1
                and map.stride(1) == 2 and map.device == frames.device):
            raise AgxError(_ffi.AGX_ERR_ARG, "map must be an int32 tensor [dst_h, dst_w, 2] on the frames' device whose rows are packed")
        n, dh, dw = int(frames.shape[0]), int(map.shape[0]), int(map.shape[1])
        if out is None:
            out = torch.empty((n, dh, dw), dtype=frames.dtype, device=frames.device)
        elif self._gray_batch(out, "out")[0] != fmt or tuple(out.shape) != (n, dh, dw) or out.device != frames.device:
            raise AgxError(_ffi.AGX_ERR_ARG, "out must be a tensor [N, dst_h, dst_w] of the frames' dtype on their device")
        self._follow_torch_stream(frames)
        rs = lambda t: (t.stride(1) if t.shape[1] > 1 else t.shape[2]) * px  # (a lone row or frame has no stride of its own)
        fs = lambda t: (t.stride(0) * px if t.shape[0] > 1 else rs(t) * t.shape[1])
        self._enqueued(self._lib.agx_remap_enqueue(self._h, frames.data_ptr(), n, int(frames.shape[2]), int(frames.shape[1]), rs(frames), fs(frames), fmt,
                                                   map.data_ptr(), (map.stride(0) if dh > 1 else 2 * dw) * 4, dw, dh, out.data_ptr(), rs(out), fs(out),
                                                   int(border)))
        return out

    def decimate_enqueue(self, frames, factor, out=None):
        """decimate (the host form says what is computed) of a device batch [N, H, W] uint8 / 16-bit by `factor` in 2 .. 4 into out
        [N, H // factor, W // factor] of the same dtype (made if None), stream-ordered behind torch's current stream; nothing to
        fetch.  frames and out may be views with padded rows and frames.  -> out."""
        import torch
        fmt, px = self._gray_batch(frames, "frames")
        f = int(factor)
        n, dh, dw = int(frames.shape[0]), int(frames.shape[1]) // max(f, 1), int(frames.shape[2]) // max(f, 1)
        if out is None:
            out = torch.empty((n, max(dh, 1), max(dw, 1)), dtype=frames.dtype, device=frames.device)  # (a side of 0: the library refuses)
        elif self._gray_batch(out, "out")[0] != fmt or tuple(out.shape) != (n, dh, dw) or out.device != frames.device:
            raise AgxError(_ffi.AGX_ERR_ARG, "out must be a tensor [N, H // factor, W // factor] of the frames' dtype on their device")
        self._follow_torch_stream(frames)
        rs = lambda t: (t.stride(1) if t.shape[1] > 1 else t.shape[2]) * px  # (a lone row or frame has no stride of its own)
        fs = lambda t: (t.stride(0) * px if t.shape[0] > 1 else rs(t) * t.shape[1])
        self._enqueued(self._lib.agx_decimate_enqueue(self._h, frames.data_ptr(), n, int(frames.shape[2]), int(frames.shape[1]), rs(frames), fs(frames),
                                                      fmt, f, out.data_ptr(), rs(out), fs(out)))
        return out

    def rectified_points_enqueue(self, points, camera, new_camera, rotation=None, out=None):
        """rectified_points (the host form says what is computed) on the device, stream-ordered behind torch's current stream;
        nothing to fetch.  points: a contiguous float32 device tensor [..., 2] -> out of the same shape (made if None; out = points
        is in place); or an int32 tag table [..., 9] of detect_batch_enqueue(out=) / collect_tags_enqueue, whose corners are
        replaced in place (four launches, one per corner; the ids stay).  -> the tensor written."""
        import torch
        model, cam, ncam, rot, _, _ = _rectify_args(camera, (1, 1), None, new_camera, rotation)
        if not (getattr(points, "is_cuda", False) and points.is_contiguous() and points.dim() >= 1):
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be a contiguous device tensor")
        self._follow_torch_stream(points)
        if points.dtype == torch.int32 and points.shape[-1] == 9:
            if out is not None and out is not points:
                raise AgxError(_ffi.AGX_ERR_ARG, "a tag table is converted in place")
            rows = points.numel() // 9
            for j in range(4 if rows else 0):
                p = points.data_ptr() + 4 + 8 * j
                self._enqueued(self._lib.agx_rectified_points_enqueue(self._h, model, cam, ncam, rot, p, 36, rows, p, 36))
            return points
        if points.dtype != torch.float32 or points.shape[-1] != 2:
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be float32 [..., 2] or an int32 tag table [..., 9]")
        if out is None:
            out = torch.empty_like(points)
        elif not (getattr(out, "is_cuda", False) and out.is_contiguous() and out.dtype == torch.float32 and out.shape == points.shape
                  and out.device == points.device):
            raise AgxError(_ffi.AGX_ERR_ARG, "out must be a contiguous float32 tensor of the points' shape on their device")
        self._enqueued(self._lib.agx_rectified_points_enqueue(self._h, model, cam, ncam, rot, points.data_ptr(), 8, points.numel() // 2,
                                                              out.data_ptr(), 8))
        return out

    def render_boards_enqueue(self, frames, cols, rows, camera, poses, truth, n_truth, status, family=None, first_id=0, spacing_ratio=0.3,
                              tag_size=1.0, black=0, white=None, background=None, page_margin=0.5, supersample=3, keep_background=False):
        """render_boards (the host form says what is drawn) into a device batch, stream-ordered behind torch's current stream;
        nothing to fetch.  frames: a device tensor [N, H, W] uint8 / 16-bit whose pixels of a row are adjacent (rows and frames may
        be padded views); poses: float64 [N, 12] on the frames' device, R row major then t -- board_pose_enqueue's `pose`, read
        in place; truth int32 [N, rows * cols, 9], n_truth and status int32 [N] take the projected corners of every tag (the
        rows board_pose_enqueue's `pred` would hold), their count and AGX_RENDER_*.  family: a TagFamily (default: the
        detector's).  white defaults to the format's largest value, background to half of it.  -> frames."""
        import torch
        fmt, px = self._gray_batch(frames, "frames")
        n, h, w, dev = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]), frames.device
        n_board = int(cols) * int(rows)

        def tensor(t, dtype, shape, what):
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the frames' device" % (what, dtype, shape))
            return t.data_ptr()

        ptrs = (tensor(truth, torch.int32, (n, n_board, 9), "truth"), tensor(n_truth, torch.int32, (n,), "n_truth"),
                tensor(status, torch.int32, (n,), "status"))
        d_poses = tensor(poses, torch.float64, (n, 12), "poses")
        model, cam = _camera(camera)
        params = _render_params(fmt, black, white, background, page_margin, supersample, keep_background)
        fam = int(self.tag_family if family is None else (TagFamily.from_str(family) if isinstance(family, str) else family))
        self._follow_torch_stream(frames)
        rs = (frames.stride(1) if h > 1 else w) * px  # (a lone row or frame has no stride of its own)
        fs = frames.stride(0) * px if n > 1 else rs * h
        self._enqueued(self._lib.agx_render_boards_enqueue(self._h, n, w, h, rs, fs, fmt, fam, int(cols), int(rows), int(first_id), float(spacing_ratio),
                                                           float(tag_size), model, cam, d_poses, C.addressof(params), frames.data_ptr(), *ptrs))
        return frames

    def detect_rectified(self, frames, camera, new_camera=None, dst_size=None, rotation=None, to_source=False, border=0, **detect_kw):
        """detect_batch on the frames as the ideal pinhole `new_camera` (default: the camera's own fx fy cx cy) would have seen
        them: frames, a device tensor [N, H, W] uint8 / 16-bit of `camera` (a Camera of any lens model), go through remap_enqueue
        into a batch of dst_size (w, h; default the frames' size) on the device and detect_batch_device runs on that batch
        (detect_kw: its keywords).  The map is computed on the device once and kept on the detector, keyed by the arguments.
        -> detect_batch's structure, the corners in rectified pixels or, with to_source=True, in the sensor's (rectified_points of
        every corner)."""
        src_size = (int(frames.shape[2]), int(frames.shape[1]))
        model, cam, ncam, rot, _, dst = _rectify_args(camera, src_size, dst_size, new_camera, rotation)
        key = (model, tuple(cam), tuple(ncam), None if rot is None else tuple(rot), src_size, dst, frames.device.index)
        cache = self.__dict__.setdefault("_rectify_maps", {})
        if key not in cache:
            cache[key] = self.rectify_map_enqueue(camera, src_size, dst, new_camera, rotation)
        rect = self.remap_enqueue(frames, cache[key], border=border)
        res = self.detect_batch_device(rect, **detect_kw)
        if to_source:
            for frame in (res[0] if isinstance(res, tuple) else res):
                for t in (frame or ()):
                    frame[t] = rectified_points(frame[t], camera, ncam, rotation)
        return res

    def find_boards_staged(self, saddles, spacing_ratio=0.3, counts=None, point_status=None, quads_per_frame=128, candidates_per_frame=1024,
                           n_nearest=50):
        """try_find_best_board (src/detector.rs:588-639) as its stages on device tensors, at ANY spacing_ratio: the reference's seeds
        and their candidate quads (init_quads_enqueue), a board from every candidate (grow_boards_enqueue), then the reference's
        stop rule per seed SADDLE (:626) on the host from the seeds' scores and the quads per seed: the board is the first
        candidate that strictly beats all before it among those of the seeds up to and including the first seed after which the
        best score is >= 36.  Where that is not the first maximum over all candidates, a second grow launch restricted to that
        prefix gives the board.  saddles / counts / point_status as find_boards_enqueue's.  -> (quads, quad_points, n_quads,
        status) as find_boards_fetch returns them: at 0.3 what find_boards_enqueue + find_boards_fetch answer."""
        import torch
        n, dev = int(saddles.shape[0]), saddles.device
        qpf, cpf = int(quads_per_frame), int(candidates_per_frame)
        i32 = dict(dtype=torch.int32, device=dev)
        cand, ncand, cst = torch.zeros((n, cpf, 4), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        per_seed = torch.zeros((n, 30), **i32)
        self.init_quads_enqueue(saddles, cand, ncand, cst, seeds_per_frame=30, n_nearest=n_nearest, counts=counts, point_status=point_status,
                                seed_quad_counts=per_seed)
        self.init_quads_fetch()
        quads, qpts = torch.zeros((n, qpf, 4), **i32), torch.zeros((n, qpf, 4, 2), dtype=torch.float32, device=dev)
        nq, bst, best = torch.zeros(n, **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        scores = torch.zeros((n, cpf), **i32)

        def grow(seed_counts):
            self.grow_boards_enqueue(saddles, cand, quads, nq, bst, counts=counts, point_status=point_status, seed_counts=seed_counts,
                                     spacing_ratio=spacing_ratio, stop_score=0, fix_missing=True, quad_points=qpts, seed_scores=scores,
                                     best_seed=best)
            self.grow_boards_fetch()

        grow(ncand)
        h_cst, h_ncand, h_per = cst.cpu().numpy(), ncand.cpu().numpy(), per_seed.cpu().numpy()
        h_bst, h_best, h_scores = bst.cpu().numpy(), best.cpu().numpy(), scores.cpu().numpy()
        prefix = h_ncand.copy()
        again = False
        for f in range(n):
            if h_cst[f] != _ffi.AGX_BOARD_FOUND or h_bst[f] not in (_ffi.AGX_BOARD_FOUND, _ffi.AGX_BOARD_CAPACITY):
                continue
            best_score, best_at, done = 0, -1, 0
            for per in h_per[f]:  # the reference's loop over the seed saddles (:613-629)
                for i in range(done, done + int(per)):
                    if int(h_scores[f, i]) > best_score:
                        best_score, best_at = int(h_scores[f, i]), i
                done += int(per)
                if best_score >= 36:
                    break
            prefix[f] = done
            again = again or best_at != int(h_best[f])
        if again:
            grow(torch.from_numpy(prefix.astype(np.int32)).to(dev))
        out_q = np.full((n, qpf, 4), 0xFFFFFFFF, np.uint32)
        out_p = np.full((n, qpf, 4, 2), np.nan, np.float32)
        h_q, h_p = quads.cpu().numpy().view(np.uint32), qpts.cpu().numpy()
        out_n, out_s = nq.cpu().numpy().view(np.uint32).copy(), bst.cpu().numpy().view(np.uint32).copy()
        for f in range(n):
            if h_cst[f] == _ffi.AGX_BOARD_CAPACITY:
                raise AgxError(_ffi.AGX_ERR_CAPACITY, "find_boards_staged: frame %d has %d candidate quads (candidates_per_frame = %d)"
                               % (f, int(h_ncand[f]), cpf))
            if out_s[f] == _ffi.AGX_BOARD_FOUND:
                k = int(out_n[f])
                out_q[f, :k], out_p[f, :k] = h_q[f, :k], h_p[f, :k]
        return out_q, out_p, out_n, out_s

    # ---- gaussian_blur_f32 / hessian_response as planes (src/image_util.rs:110-206, :72-109) ----
    @staticmethod
    def _strided_frames(frames, format=None):
        """-> (agx_format, n, w, h, row stride, frame stride in bytes) of a device tensor of frames whose rows (and, for the
        planar layout, planes) may be padded: a view cut out of a larger tensor."""
        fmt, bpp = TagDetector._tensor_format(frames, format, strided=True)
        planes = _ffi.FORMAT_LAYOUT[fmt][1]
        el, st = frames.element_size(), frames.stride()
        n = int(frames.shape[0])
        h, w = (int(frames.shape[2]), int(frames.shape[3])) if planes == 3 else (int(frames.shape[1]), int(frames.shape[2]))
        row = st[2] if planes == 3 else st[1]
        inner = tuple(st[3:]) if planes == 3 else tuple(st[2:])
        dense = (1,) if frames.dim() == 3 or planes == 3 else (int(frames.shape[3]), 1)
        if inner != dense or (planes == 3 and st[1] != h * row):
            raise AgxError(_ffi.AGX_ERR_ARG, "frames: the pixels of a row must be contiguous (rows and frames may be padded)")
        return fmt, n, w, h, row * el, st[0] * el

    def planes_enqueue(self, frames, sigma, blur=None, response=None, format=None):
        """gaussian_blur_f32(to_luma32f(frame), sigma) into `blur` and hessian_response of it into `response` (either may be
        None, not both), over a batch on this detector's GPU, stream-ordered behind torch's current stream; returns immediately
        and there is nothing to fetch: the planes are complete in stream order.  frames and format= as saddles_batch_enqueue,
        but rows and frames may be padded (a view); blur, response: float32 device tensors [N,H,W] with contiguous rows and the
        same strides.  sigma 0: no blur -- blur must be None and response is hessian_response(to_luma32f(frame)).
        The handle keeps no reference to frames, blur or response: the caller keeps the outputs alive to use them, and frames may
        be dropped at once, because the kernels run on torch's current stream and torch's allocator hands freed memory out
        again only to work queued behind them on that stream (a tensor used on another stream needs record_stream, as ever)."""
        import torch
        fmt, n, w, h, rs, fs = self._strided_frames(frames, format)
        strides = None
        for t, what in ((blur, "blur"), (response, "response")):
            if t is None:
                continue
            if not (getattr(t, "is_cuda", False) and t.dtype == torch.float32 and tuple(t.shape) == (n, h, w) and t.stride(2) == 1
                    and t.device == frames.device):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a float32 tensor %s with contiguous rows on the frames' device" % (what, (n, h, w)))
            if strides is not None and strides != (t.stride(0), t.stride(1)):
                raise AgxError(_ffi.AGX_ERR_ARG, "blur and response must have the same strides")
            strides = (t.stride(0), t.stride(1))
        ors, ofs = (4 * strides[1], 4 * strides[0]) if strides else (4 * w, 4 * w * h)
        self._follow_torch_stream(frames)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_planes_enqueue(self._h, frames.data_ptr(), n, w, h, rs, fs, fmt, float(sigma),
                                                 blur.data_ptr() if blur is not None else None,
                                                 response.data_ptr() if response is not None else None, ors, ofs))

    def gaussian_blur_f32(self, img, sigma=1.5, format=None):
        """image_util::gaussian_blur_f32(img.to_luma32f(), sigma) of a host image (any format; an HxW float32 plane is taken
        as it is) -> HxW float32 array."""
        a, fmt, stride = _image_args(img, format)
        h, w = _image_hw(a, fmt)
        out = np.empty((h, w), np.float32)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_gaussian_blur_f32(self._h, a.ctypes.data, w, h, stride, fmt, float(sigma), out.ctypes.data))
        return out

    def hessian_response(self, img, format=None):
        """image_util::hessian_response(img.to_luma32f()) of a host image, no blur -> HxW float32 array."""
        a, fmt, stride = _image_args(img, format)
        h, w = _image_hw(a, fmt)
        out = np.empty((h, w), np.float32)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = None
        self._check(self._lib.agx_hessian_response(self._h, a.ctypes.data, w, h, stride, fmt, out.ctypes.data))
        return out

    # ---- cluster centres of caller-given response planes, the k / phi filter (src/detector.rs:414-429, :432-445) ----
    def cluster_centers(self, resp, cap=16384):
        """src/detector.rs:414-429 on an HxW float32 response plane in host memory: the frame minimum, thr = 0.05 * min,
        init_saddle_clusters and the centroid map -> (rows CLUSTER_DTYPE (first_index, size, cx, cy) in the reference's order,
        status AGX_CLUSTERS_*, count).  A plane with a pixel of its outermost ring below thr is refused (AGX_CLUSTERS_BORDER, no
        rows); more than `cap` clusters is AGX_CLUSTERS_CAPACITY with the true count and no rows."""
        a = np.asarray(resp)
        if a.dtype != np.float32 or a.ndim != 2 or a.strides[1] != 4 or a.strides[0] < 4 * a.shape[1]:
            a = np.ascontiguousarray(resp, np.float32)
        if a.ndim != 2:
            raise AgxError(_ffi.AGX_ERR_ARG, "resp must be an HxW float32 plane")
        h, w = a.shape
        out = np.zeros(int(cap), _CLUSTER_DTYPE)
        n, status = C.c_uint32(0), C.c_uint32(0)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = self._clusters = None
        self._check(self._lib.agx_cluster_centers(self._h, a.ctypes.data, w, h, a.strides[0], out.ctypes.data, int(cap), C.byref(n), C.byref(status)))
        ok = (status.value & 0xFF) == _ffi.AGX_CLUSTERS_OK
        return out[:n.value if ok else 0].copy(), status.value, n.value

    def clusters_enqueue(self, response, clusters_per_frame=4096, clusters=None, points=None, counts=None, status=None):
        """src/detector.rs:414-429 over a batch of response planes on this detector's GPU, stream-ordered behind torch's current
        stream; returns immediately.  response: float32 device tensor [N,H,W] with contiguous rows (rows and frames may be padded:
        planes_enqueue's `response`, or any plane of the caller's).  clusters int32 [N,C,4] (first_index, size and the float
        bits of cx, cy: view it as CLUSTER_DTYPE on the host), counts int32 [N] and status int32 [N]: device-resident results
        (all or none; C = clusters_per_frame without them); points float32 [N,C,2] optionally -- with counts it is
        refine_points_enqueue's points / counts as it stands."""
        import torch
        if not (getattr(response, "is_cuda", False) and response.dtype == torch.float32 and response.dim() == 3 and response.stride(2) == 1):
            raise AgxError(_ffi.AGX_ERR_ARG, "response must be a float32 device tensor [N, H, W] with contiguous rows")
        n, h, w = (int(v) for v in response.shape)
        dev = response.device

        def tensor(t, dtype, shape, what):
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous %s tensor %s on the planes' device" % (what, dtype, shape))
            return t.data_ptr()

        given = [t is not None for t in (clusters, counts, status)]
        if any(given) != all(given):
            raise AgxError(_ffi.AGX_ERR_ARG, "clusters, counts and status: all or none")
        cpf = int(clusters.shape[1]) if clusters is not None and clusters.dim() == 3 else int(clusters_per_frame)
        p_rows = tensor(clusters, torch.int32, (n, cpf, 4), "clusters") if clusters is not None else None
        p_counts = tensor(counts, torch.int32, (n,), "counts") if counts is not None else None
        p_status = tensor(status, torch.int32, (n,), "status") if status is not None else None
        p_points = tensor(points, torch.float32, (n, cpf, 2), "points") if points is not None else None
        self._follow_torch_stream(response)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = self._clusters = None
        self._check(self._lib.agx_clusters_enqueue(self._h, response.data_ptr(), n, w, h, 4 * response.stride(1), 4 * response.stride(0), cpf,
                                                   p_rows, p_points, p_counts, p_status))
        self._clusters = (n, cpf, (response, points), (clusters, points, counts, status) if clusters is not None else None)

    def clusters_fetch(self):
        """Wait for clusters_enqueue's batch -> (rows [N,C] CLUSTER_DTYPE, points [N,C,2] float32, counts [N] uint32, status [N]
        uint32 AGX_CLUSTERS_*); slots at or beyond a frame's count read 0xFFFFFFFF / NaN (points given to the enqueue stay on the
        device: None here).  After clusters_enqueue(clusters=, counts=, status=): those device tensors (clusters, points or None,
        counts, status), complete."""
        if getattr(self, "_clusters", None) is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no clusters batch enqueued")
        n, cpf, keep, dev_out = self._clusters
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = self._clusters = None
        if dev_out is not None:
            self._check(self._lib.agx_clusters_fetch(self._h, None, None, None, None))
            return dev_out
        rows = np.full((n, cpf, 4), 0xFFFFFFFF, np.uint32).view(_CLUSTER_DTYPE).reshape(n, cpf)
        pts = np.full((n, cpf, 2), np.nan, np.float32) if keep[1] is None else None
        counts = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint32)
        self._check(self._lib.agx_clusters_fetch(self._h, rows.ctypes.data, pts.ctypes.data if pts is not None else None, counts.ctypes.data,
                                                 status.ctypes.data))
        return rows, pts, counts, status

    def filter_saddles_enqueue(self, records, status, counts=None):
        """The k / phi filter of refined_saddle_points (src/detector.rs:432-445) on refine_points_enqueue's device tensors, in
        place and stream-ordered behind torch's current stream: records float32 [N,P,5], status int32 [N,P], counts int32 [N]
        (optional).  Refined slots (status 0) that fail k >= max_k / 10 or min_saddle_angle <= phi <= max_saddle_angle get
        AGX_POINT_FILTERED; status then serves as find_boards_enqueue's point_status.  Nothing to fetch."""
        import torch
        if not (getattr(records, "is_cuda", False) and records.is_contiguous() and records.dtype == torch.float32 and records.dim() == 3
                and records.shape[2] == 5):
            raise AgxError(_ffi.AGX_ERR_ARG, "records must be a contiguous float32 device tensor [N, P, 5]")
        n, ppf = int(records.shape[0]), int(records.shape[1])
        for t, shape, what in ((status, (n, ppf), "status"), (counts, (n,), "counts")):
            if t is not None and not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == torch.int32 and tuple(t.shape) == shape
                                      and t.device == records.device):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous int32 tensor %s on the records' device" % (what, shape))
        if status is None:
            raise AgxError(_ffi.AGX_ERR_ARG, "status must be given")
        self._follow_torch_stream(records)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = self._clusters = None
        self._check(self._lib.agx_filter_saddles_enqueue(self._h, records.data_ptr(), status.data_ptr(), n, ppf,
                                                         counts.data_ptr() if counts is not None else None))

    # ---- the rounds of max_num_of_boards on the device (src/detector.rs:510-539) ----------------
    def collect_tags_enqueue(self, quads, n_quads, board_status, quad_tags, quad_status, point_status, tags, n_tags, tag_status,
                             reset=False, frame_table=None, saddles_per_frame=None):
        """One round of detect's loop behind its board search and decode (src/detector.rs:510-539), per frame, in place and
        stream-ordered behind torch's current stream; nothing to fetch.  quads int32 [N,Q,4], n_quads and board_status int32 [N]:
        find_boards_enqueue's quads, n_quads and status; quad_tags int32 [N,Q,9] and quad_status int32 [N,Q]:
        decode_quads_enqueue's out and status.  tags int32 [N,T,9] (split_device_tags reads it), n_tags and tag_status int32 [N]:
        the frames' tag tables, in and out -- every decoded quad inserts (id, corners): a new id takes the next row, a known one
        keeps its row and takes the new corners; tag_status is AGX_TAGS_*, and a frame that is not AGX_TAGS_OK stays as it is.
        reset=True takes every table as empty (the first round).  point_status int32 [N,S] (or, with frame_table int32 [N,4],
        the flat words that table indexes): find_boards_enqueue's point_status; the saddles of decoded quads get
        AGX_POINT_USED.  None: nothing is marked (the last round) and saddles_per_frame= names S, the bound of a slot number."""
        import torch
        if not (getattr(quads, "is_cuda", False) and quads.dim() == 3 and quads.shape[2] == 4 and quads.shape[1] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "quads must be a device tensor [N, Q, 4]")
        if not (getattr(tags, "is_cuda", False) and tags.dim() == 3 and tags.shape[2] == 9 and tags.shape[1] > 0):
            raise AgxError(_ffi.AGX_ERR_ARG, "tags must be a device tensor [N, T, 9]")
        n, qpf, tpf = int(quads.shape[0]), int(quads.shape[1]), int(tags.shape[1])
        dev = quads.device

        def tensor(t, shape, what):
            if not (getattr(t, "is_cuda", False) and t.is_contiguous() and t.dtype == torch.int32 and (shape is None or tuple(t.shape) == shape)
                    and t.device == dev):
                raise AgxError(_ffi.AGX_ERR_ARG, "%s must be a contiguous int32 tensor %s on the quads' device" % (what, shape))
            return t.data_ptr()

        p = [tensor(quads, (n, qpf, 4), "quads"), tensor(n_quads, (n,), "n_quads"), tensor(board_status, (n,), "board_status"),
             tensor(quad_tags, (n, qpf, 9), "quad_tags"), tensor(quad_status, (n, qpf), "quad_status")]
        p_table = tensor(frame_table, (n, 4), "frame_table") if frame_table is not None else None
        p_ps = None
        if point_status is not None:
            p_ps = tensor(point_status, None, "point_status")
            if frame_table is None:
                if point_status.dim() != 2 or point_status.shape[0] != n or point_status.shape[1] == 0:
                    raise AgxError(_ffi.AGX_ERR_ARG, "point_status must be [N, S] (or the flat words of frame_table)")
                if saddles_per_frame is not None and int(saddles_per_frame) != int(point_status.shape[1]):
                    raise AgxError(_ffi.AGX_ERR_ARG, "saddles_per_frame is point_status' second dimension")
                saddles_per_frame = int(point_status.shape[1])
        if frame_table is None and not saddles_per_frame:
            raise AgxError(_ffi.AGX_ERR_ARG, "without point_status and frame_table: saddles_per_frame= bounds the slot numbers")
        out = [tensor(tags, (n, tpf, 9), "tags"), tensor(n_tags, (n,), "n_tags"), tensor(tag_status, (n,), "tag_status")]
        self._follow_torch_stream(quads)
        self._batch = self._detect = self._refine = self._decode = self._grow = self._find = self._clusters = None
        self._check(self._lib.agx_collect_tags_enqueue(self._h, n, qpf, *p, int(saddles_per_frame or 0), p_table, p_ps, tpf, *out,
                                                       1 if reset else 0))

    _TAGS_STATUS = {_ffi.AGX_TAGS_CAPACITY: "AGX_TAGS_CAPACITY (more tags than tags_per_frame)",
                    _ffi.AGX_TAGS_INPUT: "AGX_TAGS_INPUT (a board beyond quads_per_frame, or a refused saddle list)",
                    _ffi.AGX_TAGS_PENDING: "AGX_TAGS_PENDING"}

    def detect_staged(self, frames, clusters_per_frame=4096, quads_per_frame=128, tags_per_frame=None, format=None, decode_model="affine"):
        """detect (src/detector.rs:505-540) as the staged chain on device tensors, every stage handing its arrays to the next in
        place: planes at the handle's sigma, clusters, refine on the blur plane at the handle's half_size_patch, the k / phi
        filter, then max_num_of_boards rounds of find boards -> find_boards_fetch (which lets the host form answer a frame the
        kernel hands back) -> decode -> collect (src/detector.rs:510-539).  frames and format= as detect_batch_enqueue.
        decode_model: "affine" -- the fused decode, the reference's -- or "homography": the decode as its three stages with
        tag_homography (src/image_util.rs:5-37) as the sampling model, for tags seen under strong perspective.
        tags_per_frame: rows of a frame's tag table (None: one per code of the family, which always holds).
        -> one {tag_id: 4x2 corners} per frame in row order, as detect_batch.  A frame whose clusters or tags could not be held
        raises AgxError naming the frame and its status."""
        _lists, cstatus, tags, ntags, tst = self._staged_tables(frames, clusters_per_frame, quads_per_frame, tags_per_frame, format, decode_model)
        self.sync()
        return self._staged_result("detect_staged", cstatus, int(clusters_per_frame), tags, ntags, tst)

    def detect_decimated(self, frames, factor=2, fine_half_size_patch=None, clusters_per_frame=4096, quads_per_frame=128, tags_per_frame=None,
                         format=None, decode_model="affine", return_saddles=False):
        """detect, coarse to fine (AprilTag's quad_decimate with a refine at full resolution): the frames -- a device tensor [N,H,W]
        uint8 / 16-bit -- are averaged down by `factor` in 2 .. 4 (decimate_enqueue); detect_staged's planes, clusters and refine
        run on that coarse batch, 1 / factor^2 of the pixels and of the workspace; refine_windows_enqueue then refines every coarse
        saddle on the FULL frames at fine_half_size_patch (None: the handle's half_size_patch), reading the coarse records in place
        with the coarse point status handed on and the points taken to full resolution by its factor=; the k / phi filter and
        detect_staged's rounds -- find boards, decode on the full-resolution frames, collect -- follow.  No plane of the full size
        is made.  The remaining keywords are detect_staged's.  factor=1 is detect_staged itself.
        -> detect_staged's structure, the corners in full-resolution pixels; with return_saddles also (records, counts, status),
        the fine saddle lists as device tensors."""
        import torch
        if int(factor) == 1:
            if return_saddles:
                raise AgxError(_ffi.AGX_ERR_ARG, "factor=1 is detect_staged, which returns no saddle lists")
            return self.detect_staged(frames, clusters_per_frame, quads_per_frame, tags_per_frame, format, decode_model)
        if format is not None and format != self._gray_batch(frames, "frames")[0]:
            raise AgxError(_ffi.AGX_ERR_FORMAT, "detect_decimated at factor > 1 takes AGX_L8 / AGX_L16 frames [N, H, W]")
        self._gray_batch(frames, "frames")
        if not frames.is_contiguous():
            raise AgxError(_ffi.AGX_ERR_ARG, "frames must be a contiguous device tensor")
        n, h, w = (int(v) for v in frames.shape)
        cpf, qpf = int(clusters_per_frame), int(quads_per_frame)
        if tags_per_frame is None:
            n_codes = C.c_int(0)
            self._check(self._lib.agx_detector_family_info(self._h, None, None, None, None, C.byref(n_codes)))
            tags_per_frame = n_codes.value
        half = self.half_size_patch if fine_half_size_patch is None else int(fine_half_size_patch)
        coarse = self.decimate_enqueue(frames, factor)
        crec, counts, cpst, cstatus = self._staged_saddles(coarse, n, int(coarse.shape[2]), int(coarse.shape[1]), cpf, None, filtered=False)
        records, pstatus = torch.zeros_like(crec), torch.zeros_like(cpst)
        self.refine_windows_enqueue(frames, crec, records, pstatus, counts=counts, status_in=cpst, factor=factor, half_size_patch=half)
        self.filter_saddles_enqueue(records, pstatus, counts=counts)
        listed = pstatus.clone() if return_saddles else None
        tags, ntags, tst = self._staged_rounds(frames, n, w, h, records, counts, pstatus, cpf, qpf, int(tags_per_frame), None, decode_model)
        self.sync()
        out = self._staged_result("detect_decimated", cstatus, cpf, tags, ntags, tst)
        return (out, (records, counts, listed)) if return_saddles else out

    def _staged_tables(self, frames, clusters_per_frame, quads_per_frame, tags_per_frame, format, decode_model, keep_listed=False):
        """detect_staged's chain and rounds, enqueued -> ((records, counts, listed point status), cluster status, tags, n_tags,
        tag_status): device tensors, complete in stream order.  keep_listed: the point status words as the k / phi filter left
        them, before any round marked a saddle used (a copy; else None)."""
        import torch
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, _, _ = self._tensor_geometry(frames, fmt, bpp)
        n, w, h = int(n), int(w), int(h)
        cpf, qpf = int(clusters_per_frame), int(quads_per_frame)
        if tags_per_frame is None:
            n_codes = C.c_int(0)
            self._check(self._lib.agx_detector_family_info(self._h, None, None, None, None, C.byref(n_codes)))
            tags_per_frame = n_codes.value
        tpf = int(tags_per_frame)
        dev = frames.device
        i32 = dict(dtype=torch.int32, device=dev)
        records, counts, pstatus, cstatus = self._staged_saddles(frames, n, w, h, cpf, format)
        listed = pstatus.clone() if keep_listed else None
        tags, ntags, tst = self._staged_rounds(frames, n, w, h, records, counts, pstatus, cpf, qpf, tpf, format, decode_model)
        return (records, counts, listed), cstatus, tags, ntags, tst

    def _staged_rounds(self, frames, n, w, h, records, counts, pstatus, cpf, qpf, tpf, format, decode_model):
        """max_num_of_boards rounds of find boards -> decode on `frames` -> collect over the saddle lists (records, counts, pstatus:
        _staged_saddles'), enqueued -> (tags, n_tags, tag_status), device tensors."""
        import torch
        dev = frames.device
        i32 = dict(dtype=torch.int32, device=dev)
        quads, qpts = torch.zeros((n, qpf, 4), **i32), torch.zeros((n, qpf, 4, 2), dtype=torch.float32, device=dev)
        nq, bst = torch.zeros(n, **i32), torch.zeros(n, **i32)
        qtags, qst = torch.zeros((n, qpf, 9), **i32), torch.zeros((n, qpf), **i32)
        tags, ntags, tst = torch.zeros((n, tpf, 9), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        rounds = int(self.detector_params.max_num_of_boards)
        decode_model = tag_map_model(decode_model)
        if decode_model != _ffi.AGX_TAG_MAP_AFFINE:
            edge = self._family_info()[0]
            spts = torch.zeros((n, qpf, edge * edge, 2), dtype=torch.float32, device=dev)
            sbits = torch.zeros((n, qpf), dtype=torch.int64, device=dev)
            sids, srots = torch.zeros((n, qpf), **i32), torch.zeros((n, qpf), **i32)
        for r in range(rounds):
            self.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
            self.find_boards_fetch()
            if decode_model == _ffi.AGX_TAG_MAP_AFFINE:
                self.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst, format=format)
            else:
                self.decode_positions_enqueue(qpts, spts, qst, img_size=(w, h), counts=nq, model=decode_model)
                self.bit_code_enqueue(frames, spts, sbits, qst, counts=nq, status_in=qst, format=format)
                self.best_tag_enqueue(sbits, sids, srots, qst, counts=nq, status_in=qst, quads=qpts, tags=qtags)
            self.collect_tags_enqueue(quads, nq, bst, qtags, qst, pstatus if r + 1 < rounds else None, tags, ntags, tst, reset=r == 0,
                                      saddles_per_frame=cpf)
        return tags, ntags, tst

    def recover_tags_enqueue(self, frames, saddles, counts, point_status, tags, n_tags, tag_status, cols, rows, first_id=0, spacing_ratio=0.3,
                             max_dist=3.0, max_err=2.0, max_drop=4, min_tags=2, format=None, camera=None, tag_size=1.0, iterations=10):
        """The tags of a printed board that a frame's table lacks, recovered in place on device tensors, stream-ordered behind
        torch's current stream, with no host step: board_fit_enqueue over the tables with only the missing tags predicted (the
        layout cols x rows from first_id at spacing_ratio; a row more than max_err px off goes, at most max_drop of them) ->
        snap_points_enqueue on the predicted rows in place, back to front, within max_dist px of a listed saddle -> the snapped
        slots' (x, y) gathered from the records -> decode_quads_enqueue -> a quad counts only if it decoded TO THE ID PREDICTED
        FOR IT (every other one gets AGX_QUAD_NO_MATCH) -> collect_tags_enqueue into the frame's table.  frames and format= as
        decode_quads_enqueue; saddles float32 [N, S, 5], counts int32 [N] and point_status int32 [N, S] (or None) as
        find_boards_enqueue reads them; tags int32 [N, T, 9], n_tags and tag_status int32 [N]: the tables, in and out.  A frame
        whose fit is not AGX_FIT_OK or AGX_FIT_LOOSE predicts nothing and keeps its table; a recovered id that an outlier row
        already holds takes that row (collect's rule), and the fit returned says which rows those were.
        With camera= (a Camera) the first step is board_pose_enqueue at tag_size and iterations instead: the predictions go
        through the lens model, everything behind them is unchanged.
        -> the fit's device tensors: dict(h, err_sq, row_status, n_inliers, rms, pred, n_pred, status) of board_fit_enqueue -- with
        a camera pose and best_iter of board_pose_enqueue in place of h --, and recovered int32 [N], the quads accepted per frame."""
        import torch
        if not (getattr(saddles, "is_cuda", False) and saddles.dim() == 3 and saddles.shape[2] >= 2):
            raise AgxError(_ffi.AGX_ERR_ARG, "saddles must be a device tensor [N, S, K >= 5]")
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, _, _ = self._tensor_geometry(frames, fmt, bpp)
        n, w, h, spf, tpf, nb = int(n), int(w), int(h), int(saddles.shape[1]), int(tags.shape[1]), int(cols) * int(rows)
        dev = frames.device
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        fit = dict(err_sq=torch.zeros((n, tpf), **f32),
                   row_status=torch.zeros((n, tpf), **i32), n_inliers=torch.zeros(n, **i32), rms=torch.zeros(n, **f32),
                   pred=torch.zeros((n, max(nb, 1), 9), **i32), n_pred=torch.zeros(n, **i32), status=torch.zeros(n, **i32))
        if camera is None:
            fit["h"] = torch.zeros((n, 9), dtype=torch.float64, device=dev)
            self.board_fit_enqueue(tags, n_tags, cols, rows, (w, h), first_id=first_id, spacing_ratio=spacing_ratio,
                                   max_err_sq=float(max_err) * float(max_err), max_drop=max_drop, min_tags=min_tags, predict_missing=True,
                                   tag_status=tag_status, **fit)
        else:
            fit["pose"] = torch.zeros((n, 12), dtype=torch.float64, device=dev)
            fit["best_iter"] = torch.zeros(n, **i32)
            self.board_pose_enqueue(tags, n_tags, cols, rows, camera, tag_size=tag_size, first_id=first_id, spacing_ratio=spacing_ratio,
                                    max_err_sq=float(max_err) * float(max_err), max_drop=max_drop, min_tags=min_tags, iterations=iterations,
                                    predict_missing=True, tag_status=tag_status, **fit)
        slots, quads = torch.zeros((n, nb, 4), **i32), torch.zeros((n, nb, 4), **i32)
        nq, sst, index = torch.zeros(n, **i32), torch.zeros(n, **i32), torch.zeros((n, nb), **i32)
        self.snap_points_enqueue(saddles, fit["pred"], slots, quads, nq, sst, float(max_dist) * float(max_dist), counts=counts,
                                 point_status=point_status, row_counts=fit["n_pred"], reverse=True, row_index=index)
        at = quads.long().clamp_(0, spf - 1).view(n, nb * 4, 1).expand(-1, -1, 2)  # (rows beyond a frame's count hold zeros)
        qpts = torch.gather(saddles[:, :, :2], 1, at).view(n, nb, 4, 2).contiguous()
        qtags, qst = torch.zeros((n, nb, 9), **i32), torch.zeros((n, nb), **i32)
        self.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst, format=format)
        want = torch.gather(fit["pred"][:, :, 0], 1, index.long().clamp_(0, nb - 1))
        below = torch.arange(nb, device=dev)[None, :] < nq[:, None]
        ok = below & (qst == _ffi.AGX_QUAD_DECODED) & (qtags[:, :, 0] == want)
        qst = torch.where(ok, qst, torch.full_like(qst, _ffi.AGX_QUAD_NO_MATCH))
        found = torch.full((n,), _ffi.AGX_BOARD_FOUND, **i32)
        self.collect_tags_enqueue(quads, nq, found, qtags, qst, None, tags, n_tags, tag_status, reset=False, saddles_per_frame=spf)
        fit["recovered"] = ok.sum(dim=1).to(torch.int32)
        return fit

    def detect_recovered(self, frames, cols, rows, first_id=0, spacing_ratio=0.3, max_dist=3.0, max_err=2.0, max_drop=4, min_tags=2,
                         clusters_per_frame=4096, quads_per_frame=128, tags_per_frame=None, format=None, return_fit=False, camera=None,
                         tag_size=1.0, iterations=10):
        """detect (src/detector.rs:505-540) of frames that show ONE printed board whose layout is known (Kalibr's AprilGrid:
        cols x rows tags from first_id, spacing_ratio), with the tags the board search dropped recovered: detect_staged's chain
        and rounds, then recover_tags_enqueue on its arrays as they stand -- fit, predict the missing tags, snap, decode, accept
        what decoded to the predicted id, collect.  Frames whose fit is neither AGX_FIT_OK nor AGX_FIT_LOOSE keep
        detect_staged's result.  Outlier rows are reported, never removed.
        -> one {tag_id: 4x2 corners} per frame in row order (detect_staged's rows first, bit for bit); with return_fit also a
        list of dict(status, H, rms, n_inliers, row_status, err_sq, recovered) per frame, row_status / err_sq over detect_staged's
        rows (AGX_FIT_ROW_*); H, rms, row_status and err_sq are None where the fit was refused.  With camera= (a Camera) the
        predictions go through the lens model (recover_tags_enqueue's camera=), and the dicts carry pose (float64 [12]: R row major,
        then t, at tag_size) and best_iter in place of H."""
        (records, counts, listed), cstatus, tags, ntags, tst = self._staged_tables(frames, clusters_per_frame, quads_per_frame, tags_per_frame,
                                                                                   format, "affine", keep_listed=True)
        before = ntags.clone()
        fit = self.recover_tags_enqueue(frames, records, counts, listed, tags, ntags, tst, cols, rows, first_id=first_id,
                                        spacing_ratio=spacing_ratio, max_dist=max_dist, max_err=max_err, max_drop=max_drop, min_tags=min_tags,
                                        format=format, camera=camera, tag_size=tag_size, iterations=iterations)
        self.sync()
        out = self._staged_result("detect_recovered", cstatus, int(clusters_per_frame), tags, ntags, tst)
        if not return_fit:
            return out
        host = {k: v.cpu().numpy() for k, v in fit.items() if k != "pred"}
        before = before.cpu().numpy()
        fits = []
        for f in range(len(out)):
            st, k = int(host["status"][f]), int(before[f])
            good = st in (_ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE)
            model = ({"H": host["h"][f].reshape(3, 3).copy() if good else None} if camera is None else
                     {"pose": host["pose"][f].copy() if good else None, "best_iter": int(host["best_iter"][f]) if good else None})
            fits.append({"status": st, "n_inliers": int(host["n_inliers"][f]), "recovered": int(host["recovered"][f]), **model,
                         "rms": float(host["rms"][f]) if good else None,
                         "row_status": host["row_status"][f, :k].view(np.uint32).copy() if good else None,
                         "err_sq": host["err_sq"][f, :k].copy() if good else None})
        return out, fits

    def _staged_saddles(self, frames, n, w, h, cpf, format, filtered=True):
        """The staged chain up to the saddle lists: planes at the handle's sigma, clusters, refine on the blur plane at the
        handle's half_size_patch, the k / phi filter (filtered=False: not that) -> (records float32 [N, cpf, 5], counts int32 [N], point status int32 [N, cpf],
        cluster status int32 [N]), device tensors as find_boards_enqueue reads them."""
        import torch
        dev = frames.device
        i32 = dict(dtype=torch.int32, device=dev)
        blur = torch.empty((n, h, w), dtype=torch.float32, device=dev)
        resp = torch.empty_like(blur)
        rows, pts = torch.zeros((n, cpf, 4), **i32), torch.zeros((n, cpf, 2), dtype=torch.float32, device=dev)
        counts, cstatus = torch.zeros(n, **i32), torch.zeros(n, **i32)
        records, pstatus = torch.zeros((n, cpf, 5), dtype=torch.float32, device=dev), torch.zeros((n, cpf), **i32)
        self.planes_enqueue(frames, self.blur_sigma, blur=blur, response=resp, format=format)
        self.clusters_enqueue(resp, clusters=rows, points=pts, counts=counts, status=cstatus)
        self.refine_points_enqueue(blur, pts, counts=counts, out=records, status=pstatus, image="plane", half_size_patch=self.half_size_patch)
        if filtered:
            self.filter_saddles_enqueue(records, pstatus, counts=counts)
        return records, counts, pstatus, cstatus

    def _staged_result(self, who, cstatus, cpf, tags, ntags, tst, skip=None):
        """The frames' tag tables (device tensors of collect_tags_enqueue) -> one {tag_id: 4x2 corners} per frame in row order; a
        frame whose clusters or tags could not be held raises.  skip: a bool per frame, True = not looked at (its entry is None)."""
        n, tpf = int(tags.shape[0]), int(tags.shape[1])
        cstatus, tst, ntags = cstatus.cpu().numpy(), tst.cpu().numpy(), ntags.cpu().numpy()
        table = tags.cpu().numpy().view(np.uint32).reshape(n, tpf, 9)
        out = []
        for f in range(n):
            if skip is not None and skip[f]:
                out.append(None)
                continue
            if (int(cstatus[f]) & 0xFF) != _ffi.AGX_CLUSTERS_OK:
                raise AgxError(_ffi.AGX_ERR_CAPACITY, "%s: frame %d: cluster status %d (AGX_CLUSTERS_*; clusters_per_frame = %d)"
                               % (who, f, int(cstatus[f]), cpf))
            if int(tst[f]) != _ffi.AGX_TAGS_OK:
                raise AgxError(_ffi.AGX_ERR_CAPACITY if int(tst[f]) != _ffi.AGX_TAGS_PENDING else _ffi.AGX_ERR_STATE,
                               "%s: frame %d: tag status %s" % (who, f, self._TAGS_STATUS.get(int(tst[f]), str(int(tst[f])))))
            t = table[f, :int(ntags[f])]
            out.append({int(row[0]): row[1:].view(np.float32).reshape(4, 2).copy() for row in t})
        return out

    def detect_tracked(self, frames, prior, max_dist=5.0, spacing_ratio=0.3, seeds_per_frame=None, clusters_per_frame=4096, quads_per_frame=128,
                       tags_per_frame=None, format=None):
        """detect (src/detector.rs:505-540) of a batch whose boards are known from the last call: instead of the board search, the
        prior tags' corners are snapped to this frame's saddles (snap_points_enqueue, within max_dist px) and the boards grown from
        them as seed quads.  frames and format= as detect_batch_enqueue.  prior: last call's tags per frame -- a list of
        {tag_id: 4x2 corners} (what detect_batch returns), or (tags int32 [N, T, 9], counts int32 [N]), the device tag table of
        detect_batch_enqueue(out=...) / collect_tags_enqueue and its counts.  The staged chain up to the saddle lists, then
        max_num_of_boards rounds of snap (corners back to front, listed slots only) -> grow boards at spacing_ratio with
        try_fix_missing -> grow_boards_fetch -> decode -> collect.  seeds_per_frame: only the first that many prior tags of a frame
        are seeds (None: all of them).  A frame with no snapped row, or whose first round's board status is not AGX_BOARD_FOUND, is
        not tracked: those frames, and only those, are run through detect_staged.
        -> (one {tag_id: 4x2 corners} per frame as detect_batch, tracked bool [N])."""
        import torch
        fmt, bpp = self._tensor_format(frames, format)
        n, w, h, _, _ = self._tensor_geometry(frames, fmt, bpp)
        n, w, h = int(n), int(w), int(h)
        cpf, qpf = int(clusters_per_frame), int(quads_per_frame)
        if tags_per_frame is None:
            n_codes = C.c_int(0)
            self._check(self._lib.agx_detector_family_info(self._h, None, None, None, None, C.byref(n_codes)))
            tags_per_frame = n_codes.value
        tpf = int(tags_per_frame)
        dev = frames.device
        i32 = dict(dtype=torch.int32, device=dev)
        if isinstance(prior, (list, tuple)) and len(prior) == 2 and getattr(prior[0], "is_cuda", False):
            ptags, pcounts = prior
            if ptags.dim() != 3 or ptags.shape[0] != n or pcounts.shape != (n,):
                raise AgxError(_ffi.AGX_ERR_ARG, "prior tags int32 [N, T, 9] and counts int32 [N]")
        else:
            if len(prior) != n:
                raise AgxError(_ffi.AGX_ERR_ARG, "prior: one {tag_id: corners} per frame")
            table = np.zeros((n, max([len(d) for d in prior] + [1]), 9), np.uint32)
            for f, d in enumerate(prior):
                for r, (tag_id, xy) in enumerate(d.items()):
                    table[f, r, 0] = int(tag_id)
                    table[f, r, 1:] = np.ascontiguousarray(xy, np.float32).reshape(8).view(np.uint32)
            ptags = torch.from_numpy(table.view(np.int32)).to(dev)
            pcounts = torch.tensor([len(d) for d in prior], **i32)
        if seeds_per_frame is not None:
            pcounts = torch.clamp(pcounts, max=int(seeds_per_frame))
        rpf = int(ptags.shape[1])
        records, counts, pstatus, cstatus = self._staged_saddles(frames, n, w, h, cpf, format)
        slots, seeds = torch.zeros((n, rpf, 4), **i32), torch.zeros((n, rpf, 4), **i32)
        nseeds, sst = torch.zeros(n, **i32), torch.zeros(n, **i32)
        quads, qpts = torch.zeros((n, qpf, 4), **i32), torch.zeros((n, qpf, 4, 2), dtype=torch.float32, device=dev)
        nq, bst = torch.zeros(n, **i32), torch.zeros(n, **i32)
        qtags, qst = torch.zeros((n, qpf, 9), **i32), torch.zeros((n, qpf), **i32)
        tags, ntags, tst = torch.zeros((n, tpf, 9), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        rounds = int(self.detector_params.max_num_of_boards)
        tracked = None
        for r in range(rounds):
            self.snap_points_enqueue(records, ptags, slots, seeds, nseeds, sst, float(max_dist) * float(max_dist), counts=counts,
                                     point_status=pstatus, row_counts=pcounts, reverse=True)
            self.grow_boards_enqueue(records, seeds, quads, nq, bst, counts=counts, point_status=pstatus, seed_counts=nseeds,
                                     spacing_ratio=spacing_ratio, fix_missing=True, quad_points=qpts)
            self.grow_boards_fetch()
            if r == 0:
                tracked = (nseeds > 0) & (bst == _ffi.AGX_BOARD_FOUND)
            self.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst, format=format)
            self.collect_tags_enqueue(quads, nq, bst, qtags, qst, pstatus if r + 1 < rounds else None, tags, ntags, tst, reset=r == 0,
                                      saddles_per_frame=cpf)
        self.sync()
        tracked = tracked.cpu().numpy().astype(bool) if tracked is not None else np.zeros(n, bool)
        out = self._staged_result("detect_tracked", cstatus, cpf, tags, ntags, tst, skip=~tracked)
        lost = np.flatnonzero(~tracked)
        if lost.size:
            again = self.detect_staged(frames[torch.from_numpy(lost).to(dev)].contiguous(), clusters_per_frame=cpf, quads_per_frame=qpf,
                                       tags_per_frame=tpf, format=format)
            for f, res in zip(lost, again):
                out[int(f)] = res
        return out, tracked

    # ---- measurement / parity hooks ------------------------------------------------------
    def profile_enable(self, level=2):
        """0/False off, 1 = time the blur kernel only, 2/True = time every kernel."""
        level = 2 if level is True else (0 if level is False else int(level))
        self._check(self._lib.agx_profile_enable(self._h, level))

    def profile_reset(self):
        self._check(self._lib.agx_profile_reset(self._h))

    def profile_read(self):
        names = (C.c_char_p * _ffi.AGX_N_KERNELS)()
        ms = (C.c_double * _ffi.AGX_N_KERNELS)()
        cnt = (C.c_uint64 * _ffi.AGX_N_KERNELS)()
        self._check(self._lib.agx_profile_read(self._h, names, ms, cnt))
        return {names[i].decode(): (ms[i], int(cnt[i])) for i in range(_ffi.AGX_N_KERNELS) if names[i]}

    def constants(self):
        w = np.zeros(7, np.float32)
        cone = np.zeros(25, np.float32)
        pmat = np.zeros((25, 6), np.float32)
        self._check(self._lib.agx_detector_constants(self._h, w.ctypes.data, cone.ctypes.data, pmat.ctypes.data))
        return w, cone, pmat

    def debug_fetch(self, frame, what, shape=None):
        """Intermediate product of the last batch: 'blur', 'resp' (HxW f32; K1's in-register response,
        needs set_option("store_response", 1) before the batch), 'resp_recomputed', 'min' (f32),
        'centers' (cluster table sorted by first pixel), 'refined' (unfiltered saddles)."""
        code = {"blur": 0, "resp": 1, "min": 2, "centers": 3, "refined": 4, "counters": 5, "resp_recomputed": 6, "verify_stats": 7, "redzones": 8, "luma8": 9, "wave_times": 10}[what]
        n = C.c_size_t(0)
        if code in (0, 1, 6):
            assert shape is not None
            buf = np.empty(shape, np.float32)
        elif code == 2:
            buf = np.empty(1, np.float32)
        elif code == 5:
            buf = np.empty(8, np.uint32)
        elif code == 7:
            buf = np.empty(20, np.uint32)
        elif code == 8:
            buf = np.empty(6, np.uint32)
        elif code == 9:
            assert shape is not None
            buf = np.empty(shape, np.uint8)
        elif code == 10:  # `frame` selects the kernel (1 verify, 2 flood, 3 refine); shape = number of workgroups
            buf = np.zeros((int(shape), 2), np.uint64)
        elif code == 3:
            buf = np.empty(1 << 20, _CLUSTER_DTYPE)
        else:
            buf = np.empty(1 << 20, SADDLE_DTYPE)
        self._check(self._lib.agx_debug_fetch(self._h, frame, code, buf.ctypes.data, buf.nbytes, C.byref(n)))
        if code == 2:
            return buf[0]
        if code == 5:
            return dict(zip(["flags", "seeds", "big_seeds", "clusters", "generic_candidates", "generic_roots",
                             "refined", "saddles"], [int(v) for v in buf]))
        if code == 7:
            return buf
        if code == 8:  # AGX_REDZONE_BYTES set when the handle was created: guard bytes around the workspace buffers
            return {"buffers": int(buf[0]), "damaged_bytes": int(buf[1]), "first_buffer": int(np.int32(buf[2])),
                    "first_offset": int(buf[3:4].view(np.int32)[0]), "buffer0_address": int(buf[4]) | (int(buf[5]) << 32)}
        if code in (3, 4):
            return buf[: n.value].copy()
        return buf


def blur_weights(sigma):
    """The taps of gaussian_blur_f32 at sigma (src/image_util.rs:111-124): 2 * ceil(2 sigma) + 1 float32 weights; no device."""
    w = np.zeros(2 * 16 + 1, np.float32)
    radius = C.c_int(0)
    st = _ffi.lib().agx_debug_blur_weights(float(sigma), w.ctypes.data, len(w), C.byref(radius))
    if st != _ffi.AGX_OK:
        raise AgxError(st, "sigma %r" % (sigma,))
    return w[: 2 * radius.value + 1].copy()


def refine_constants(half_size_patch):
    """rochade_refine's constants at half_size_patch in 1 .. 4 (src/detector.rs:208-254), ks = 2 * half_size_patch + 1:
    -> (cone [ks*ks] float32, pmat [ks*ks, 6] float32); no device."""
    cone = np.zeros(81, np.float32)
    pmat = np.zeros(81 * 6, np.float32)
    n = C.c_int(0)
    st = _ffi.lib().agx_debug_refine_constants(int(half_size_patch), cone.ctypes.data, pmat.ctypes.data, 81, C.byref(n))
    if st != _ffi.AGX_OK:
        raise AgxError(st, "half_size_patch %r" % (half_size_patch,))
    return cone[: n.value].copy(), pmat[: n.value * 6].reshape(n.value, 6).copy()


def filter_saddles(records, status, optional_detector_params=None):
    """The host's k / phi filter (src/detector.rs:432-445) without a device: records a SADDLE_DTYPE array (or [n, 5] float32) and
    their status words [n] (AGX_POINT_*) -> a copy of status in which the refined records that refined_saddle_points drops read
    AGX_POINT_FILTERED -- what TagDetector.filter_saddles_enqueue leaves on the device."""
    a = np.asarray(records)
    if a.dtype == SADDLE_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 5)
    st = np.array(status, np.uint32).reshape(-1)
    if st.shape[0] != a.shape[0]:
        raise AgxError(_ffi.AGX_ERR_ARG, "one status word per record")
    prm = optional_detector_params._c() if optional_detector_params is not None else None
    rc = _ffi.lib().agx_filter_saddles_tail(C.byref(prm) if prm is not None else None, a.ctypes.data if len(a) else None,
                                            st.ctypes.data if len(a) else None, a.shape[0])
    if rc != _ffi.AGX_OK:
        raise AgxError(rc)
    return st


def collect_tags(tag_family, quads, board_status, quad_tags, quad_status, n_slots, point_status=None, tags=None, n_tags=0, tag_status=0,
                 tag_cap=None):
    """One round of detect's loop behind its board search and decode (src/detector.rs:510-539) for one frame on the host, without
    a device -- what TagDetector.collect_tags_enqueue leaves on the device.  quads [n, 4] saddle indices and board_status as
    find_board_tail answered, quad_tags [n] TagDetector.TAG_DTYPE and quad_status [n] as decode_quads_tail did; n_slots bounds
    the indices; point_status: n_slots words or None (nothing is marked).  tags (TAG_DTYPE rows), n_tags and tag_status: the
    table so far (nothing for the first round); tag_cap: its rows (None: len(tags), or one per code of the family).
    -> (tags [tag_cap], n_tags, tag_status AGX_TAGS_*, point_status): copies; rows below n_tags are the table."""
    fam = TagFamily.from_str(tag_family) if isinstance(tag_family, str) else TagFamily(tag_family)
    q = np.ascontiguousarray(quads, np.uint32).reshape(-1, 4)
    qt = np.ascontiguousarray(quad_tags, TagDetector.TAG_DTYPE).reshape(-1)
    qs = np.ascontiguousarray(quad_status, np.uint32).reshape(-1)
    if not (len(q) == len(qt) == len(qs)):
        raise AgxError(_ffi.AGX_ERR_ARG, "one tag and one status per quad")
    if tag_cap is None:
        tag_cap = len(tags) if tags is not None and len(tags) else 587
    rows = np.zeros(int(tag_cap), TagDetector.TAG_DTYPE)
    if tags is not None:
        t = np.asarray(tags, TagDetector.TAG_DTYPE).reshape(-1)[:int(tag_cap)]
        rows[:len(t)] = t
    ps = np.array(point_status, np.uint32).reshape(-1) if point_status is not None else None
    if ps is not None and len(ps) != int(n_slots):
        raise AgxError(_ffi.AGX_ERR_ARG, "point_status: n_slots words")
    n, st = C.c_uint32(int(n_tags)), C.c_uint32(int(tag_status))
    rc = _ffi.lib().agx_collect_tags_tail(int(fam), len(q), q.ctypes.data if len(q) else None,
                                          int(board_status), qt.ctypes.data if len(q) else None, qs.ctypes.data if len(q) else None,
                                          int(n_slots), ps.ctypes.data if ps is not None and len(ps) else None, int(tag_cap),
                                          rows.ctypes.data if len(rows) else None, C.byref(n), C.byref(st))
    if rc != _ffi.AGX_OK:
        raise AgxError(rc)
    return rows, n.value, st.value, ps


def decode_quads_tail(tag_family, luma8, quads, with_bits=False):
    """The host's try_decode_quad (src/detector.rs:448-476) without a device: luma8 an HxW uint8 plane (to_luma8; rows may be
    strided), quads n x 4 corners (x, y).  -> (tags [n] TagDetector.TAG_DTYPE, status [n] uint32 AGX_QUAD_*) and, with_bits,
    bit_code's values [n] uint64 -- what TagDetector.decode_quads returns."""
    fam = TagFamily.from_str(tag_family) if isinstance(tag_family, str) else TagFamily(tag_family)
    g = np.asarray(luma8)
    if g.dtype != np.uint8 or g.ndim != 2 or g.strides[1] != 1 or g.strides[0] < g.shape[1]:
        g = np.ascontiguousarray(luma8, np.uint8)
    h, w = g.shape
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 8)
    n = q.shape[0]
    out = np.zeros(n, TagDetector.TAG_DTYPE)
    status = np.zeros(n, np.uint32)
    bits = np.zeros(n, np.uint64)
    n_decoded = C.c_uint32(0)
    st = _ffi.lib().agx_decode_quads_tail(int(fam), g.ctypes.data, w, h, g.strides[0], q.ctypes.data, n, out.ctypes.data, status.ctypes.data,
                                          bits.ctypes.data if with_bits else None, C.byref(n_decoded))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    assert n_decoded.value == int((status == _ffi.AGX_QUAD_DECODED).sum())
    return (out, status, bits) if with_bits else (out, status)


def tag_map_model(model):
    """"affine" / "homography" (or an AGX_TAG_MAP_* value) -> the value the library takes"""
    if isinstance(model, str):
        try:
            return {"affine": _ffi.AGX_TAG_MAP_AFFINE, "homography": _ffi.AGX_TAG_MAP_HOMOGRAPHY}[model]
        except KeyError:
            raise AgxError(_ffi.AGX_ERR_ARG, 'model must be "affine" or "homography"')
    return int(model)


def decode_positions(quads, img_w, img_h, border_bits, edge_bits, margin=0.5, model="affine"):
    """The host's decode_positions (src/detector.rs:42-72) without a device -- the first stage of decode_quads_tail, the same
    code: quads n x 4 corners (x, y).  -> (points [n, edge_bits^2, 2] float32, x outer and y inner, zero where the quad gave none;
    status [n] uint32: AGX_QUAD_DECODED or AGX_QUAD_OUTSIDE).  model="homography": tag_homography (src/image_util.rs:5-37) in
    tag_affine's place; the status may be AGX_QUAD_DEGENERATE too."""
    model = tag_map_model(model)
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 8)
    n, e = q.shape[0], int(edge_bits)
    points = np.zeros((n, max(e * e, 1) if 1 <= e <= 8 else 1, 2), np.float32)
    status = np.zeros(n, np.uint32)
    if model == _ffi.AGX_TAG_MAP_AFFINE:
        st = _ffi.lib().agx_decode_positions_tail(q.ctypes.data, n, int(img_w), int(img_h), int(border_bits), e, float(margin), points.ctypes.data,
                                                  status.ctypes.data)
    else:
        st = _ffi.lib().agx_decode_positions_tail_m(q.ctypes.data, n, int(img_w), int(img_h), int(border_bits), e, float(margin),
                                                    points.ctypes.data, status.ctypes.data, model)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return points, status


def tag_maps(quads, side_bits, margin=0.5, model="homography"):
    """The host's tag_affine (src/image_util.rs:39-70) / tag_homography (src/image_util.rs:5-37) without a device: quads n x 4
    corners (x, y), side_bits in 1 .. 40.  -> (maps [n, 3, 3] float32, row-major from the source square (-margin, -margin) ..
    (side_bits - 1 + margin, side_bits - 1 + margin) to the image, zero where the quad gave none; status [n] uint32:
    AGX_QUAD_DECODED, AGX_QUAD_OUTSIDE (a corner that is not finite) or AGX_QUAD_DEGENERATE)."""
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 8)
    n = q.shape[0]
    maps = np.zeros((n, 3, 3), np.float32)
    status = np.zeros(n, np.uint32)
    st = _ffi.lib().agx_tag_maps_tail(q.ctypes.data, n, int(side_bits), float(margin), tag_map_model(model), maps.ctypes.data, status.ctypes.data)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return maps, status


def bit_code(luma8, points, valid_brightness_threshold=10, max_invalid_bit=3, status_in=None):
    """The host's bit_code (src/detector.rs:74-122) without a device -- the second stage of decode_quads_tail, the same code:
    luma8 an HxW uint8 plane (rows may be strided), points [n, P, 2] with P in 1 .. 64, status_in [n] optional (a non-zero word
    is passed through, and the slot reads nothing).  -> (bits [n] uint64, the first point the most significant of the P bits and
    0 unless AGX_QUAD_DECODED; status [n] uint32: AGX_QUAD_DECODED / _OUTSIDE / _LOW_CONTRAST / _AMBIGUOUS)."""
    g = np.asarray(luma8)
    if g.dtype != np.uint8 or g.ndim != 2 or g.strides[1] != 1 or g.strides[0] < g.shape[1]:
        g = np.ascontiguousarray(luma8, np.uint8)
    h, w = g.shape
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 3 or p.shape[2] != 2:
        raise AgxError(_ffi.AGX_ERR_ARG, "points must be [n, P, 2]")
    n, pps = p.shape[0], p.shape[1]
    bits = np.zeros(n, np.uint64)
    status = np.zeros(n, np.uint32)
    s_in = np.ascontiguousarray(status_in, np.uint32).reshape(n) if status_in is not None else None
    st = _ffi.lib().agx_bit_code_tail(g.ctypes.data, w, h, g.strides[0], p.ctypes.data, pps, n, s_in.ctypes.data if s_in is not None else None,
                                      int(valid_brightness_threshold), int(max_invalid_bit), bits.ctypes.data, status.ctypes.data)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return bits, status


def best_tag(bits, thres, codes=None, edge_bits=None, tag_family=None, status_in=None, quads=None):
    """The host's best_tag (src/detector.rs:142-169) without a device -- the third stage of decode_quads_tail, the same code:
    bits [n] uint64, thres 0 .. 255 (a rotation matches at a distance below it), codes 1 .. 65535 uint64 codes, or None: the
    list of tag_family; edge_bits (None: tag_family's).  status_in as bit_code's.  -> (ids [n], rotations [n], status [n]
    uint32: AGX_QUAD_DECODED or AGX_QUAD_NO_MATCH) and, with quads (n x 4 corners), the tags [n] TagDetector.TAG_DTYPE that
    decode_quads_tail gives."""
    b = np.ascontiguousarray(bits, np.uint64).reshape(-1)
    n = b.shape[0]
    fam = 0
    if tag_family is not None:
        fam = int(TagFamily.from_str(tag_family) if isinstance(tag_family, str) else TagFamily(tag_family))
    if edge_bits is None:
        if tag_family is None:
            raise AgxError(_ffi.AGX_ERR_ARG, "edge_bits or tag_family must be given")
        edge_bits = {TagFamily.T16H5: 4, TagFamily.T25H7: 5, TagFamily.T25H9: 5, TagFamily.T36H11: 6, TagFamily.T36H11B1: 6}[TagFamily(fam)]
    if codes is None and tag_family is None:
        raise AgxError(_ffi.AGX_ERR_ARG, "codes or tag_family must be given")
    c = np.ascontiguousarray(codes, np.uint64).reshape(-1) if codes is not None else None
    ids, rotations, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    s_in = np.ascontiguousarray(status_in, np.uint32).reshape(n) if status_in is not None else None
    q = np.ascontiguousarray(quads, np.float32).reshape(n, 8) if quads is not None else None
    tags = np.zeros(n, TagDetector.TAG_DTYPE) if quads is not None else None
    st = _ffi.lib().agx_best_tag_tail(b.ctypes.data, n, s_in.ctypes.data if s_in is not None else None, int(thres), fam,
                                      c.ctypes.data if c is not None else None, len(c) if c is not None else 0, int(edge_bits),
                                      q.ctypes.data if q is not None else None, ids.ctypes.data, rotations.ctypes.data, status.ctypes.data,
                                      tags.ctypes.data if tags is not None else None)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return (ids, rotations, status, tags) if tags is not None else (ids, rotations, status)


def snap_points(saddles, points, max_dist_sq, reverse=False, point_status=None):
    """The host form of snap_points_enqueue for one list (agx_snap_points_tail) without a device: saddles a SADDLE_DTYPE array (or
    [n, 5] float32); points float32 [R, P, 2] with P in 1 .. 4, or R rows of TagDetector.TAG_DTYPE, whose corners are read in
    place (P = 4) -> (slots [R, P] uint32, AGX_SNAP_NONE where a point did not snap; dist_sq [R, P] float32; rows [K, P] uint32,
    the rows that snapped whole, compacted; row_index [K] uint32; status AGX_SNAP_*)."""
    a = np.asarray(saddles)
    if a.dtype == SADDLE_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 5)
    pts = np.asarray(points)
    if pts.dtype == TagDetector.TAG_DTYPE:
        pts = np.ascontiguousarray(pts).reshape(-1)
        n_rows, ppr, row_stride, p_points = pts.shape[0], 4, 36, pts.ctypes.data + 4
    else:
        pts = np.ascontiguousarray(pts, np.float32)
        if pts.ndim != 3 or pts.shape[2] != 2:
            raise AgxError(_ffi.AGX_ERR_ARG, "points must be [R, P, 2] or rows of TAG_DTYPE")
        n_rows, ppr, p_points = pts.shape[0], pts.shape[1], pts.ctypes.data
        row_stride = 8 * ppr
    ps = None if point_status is None else np.ascontiguousarray(point_status, np.uint32).reshape(a.shape[0])
    room = (max(n_rows, 1), max(ppr, 1))
    slots, dist, rows, index = np.zeros(room, np.uint32), np.zeros(room, np.float32), np.zeros(room, np.uint32), np.zeros(room[0], np.uint32)
    kept, status = C.c_uint32(0), C.c_uint32(0)
    st = _ffi.lib().agx_snap_points_tail(a.ctypes.data if a.shape[0] else None, a.shape[0], ps.ctypes.data if ps is not None and ps.size else None,
                                         p_points, row_stride, 8, n_rows, ppr, float(max_dist_sq), _ffi.AGX_SNAP_REVERSE if reverse else 0,
                                         slots.ctypes.data, dist.ctypes.data, rows.ctypes.data, C.byref(kept), index.ctypes.data, C.byref(status))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return slots[:n_rows], dist[:n_rows], rows[:kept.value].copy(), index[:kept.value].copy(), status.value


def _tag_rows(tags):
    """{tag_id: 4x2 corners} (rows in the dict's order) or rows of TagDetector.TAG_DTYPE -> contiguous rows of TAG_DTYPE"""
    if isinstance(tags, dict):
        rows = np.zeros(len(tags), TagDetector.TAG_DTYPE)
        for r, (tag_id, xy) in enumerate(tags.items()):
            rows[r]["id"] = int(tag_id)
            rows[r]["xy"] = np.asarray(xy, np.float32).reshape(8)
        return rows
    rows = np.ascontiguousarray(tags)
    if rows.dtype != TagDetector.TAG_DTYPE:
        raise AgxError(_ffi.AGX_ERR_ARG, "tags must be {tag_id: 4x2 corners} or rows of TAG_DTYPE")
    return rows.reshape(-1)


def board_fit(tags, cols, rows, img_size, first_id=0, spacing_ratio=0.3, max_err_sq=4.0, max_drop=0, min_tags=1, predict_missing=False,
              tag_status=0, tags_per_frame=None):
    """The host form of board_fit_enqueue for one frame (agx_board_fit_tail) without a device: the homography from the printed
    board (Kalibr's AprilGrid layout: tag first_id + r*cols + c at column c, row r; corner j at (c*(1+s) + (0,1,1,0)[j],
    r*(1+s) + (0,0,1,1)[j]) in tag sides) to the image through every corner of `tags` -- {tag_id: 4x2 corners} or rows of
    TagDetector.TAG_DTYPE -- with rounds that drop the row of the largest residual while that is above max_err_sq (px^2) and
    fewer than max_drop rows went, and the predicted corners of the layout's tags (predict_missing: only of those that are not
    inlier rows).  img_size (w, h) only centres and scales the image coordinates.
    -> dict: status AGX_FIT_*; for AGX_FIT_OK and AGX_FIT_LOOSE also H [3, 3] float64 (board units -> pixels), err_sq float32 and
    row_status uint32 per row (AGX_FIT_ROW_*; err_sq is NaN for an off-board row), n_inliers, rms, pred (rows of TAG_DTYPE)."""
    t = _tag_rows(tags)
    n = int(t.shape[0])
    cap = n if tags_per_frame is None else int(tags_per_frame)
    n_board = max(int(cols) * int(rows), 1) if 0 < int(cols) * int(rows) <= 4096 else 1
    h = np.zeros(9, np.float64)
    err, rst = np.full(max(n, 1), np.nan, np.float32), np.zeros(max(n, 1), np.uint32)
    pred = np.zeros(n_board, TagDetector.TAG_DTYPE)
    n_inl, n_pred, status, rms = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_float(0)
    st = _ffi.lib().agx_board_fit_tail(t.ctypes.data if n else None, cap, n, int(tag_status), int(cols), int(rows), int(first_id),
                                       float(spacing_ratio), int(img_size[0]), int(img_size[1]), float(max_err_sq), int(max_drop), int(min_tags),
                                       _ffi.AGX_FIT_PREDICT_MISSING if predict_missing else 0, h.ctypes.data, err.ctypes.data, rst.ctypes.data,
                                       C.byref(n_inl), C.byref(rms), pred.ctypes.data, C.byref(n_pred), C.byref(status))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    out = {"status": status.value, "n_inliers": n_inl.value, "n_pred": n_pred.value}
    if status.value in (_ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE):
        out.update(H=h.reshape(3, 3), err_sq=err[:n], row_status=rst[:n], rms=rms.value, pred=pred[:n_pred.value].copy())
    return out


class Camera(namedtuple("Camera", "fx fy cx cy k1 k2 p1 p2 k3", defaults=(0.0, 0.0, 0.0, 0.0, 0.0))):
    """agx_camera: the pinhole + radial-tangential model (OpenCV's; Kalibr's pinhole-radtan with k3 = 0).  Camera(fx, fy, cx, cy)
    is a pinhole.  model is the lens model the nine numbers are read under (AGX_LENS_*): AGX_LENS_RADTAN here,
    AGX_LENS_EQUIDISTANT for a camera made by Camera.equidistant, AGX_LENS_DOUBLE_SPHERE for one made by Camera.double_sphere."""
    __slots__ = ()
    model = _ffi.AGX_LENS_RADTAN

    def as_doubles(self):
        """The nine doubles agx_board_pose_enqueue / _tail read."""
        return (C.c_double * 9)(*[float(v) for v in self])

    @staticmethod
    def equidistant(fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0):
        """The pinhole-equidistant model (Kalibr's pinhole-equi, OpenCV's fisheye, Kannala-Brandt with four coefficients):
        theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), (u, v) = (fx, fy) theta_d (x, y) / r
        + (cx, cy).  A Camera whose model is AGX_LENS_EQUIDISTANT and whose nine numbers are fx, fy, cx, cy, k1, k2, k3, k4, 0."""
        return _EquidistantCamera(fx, fy, cx, cy, k1, k2, k3, k4, 0.0)

    @staticmethod
    def double_sphere(fx, fy, cx, cy, xi, alpha):
        """The double-sphere model (Usenko, Demmel, Cremers 2018; Kalibr's ds, Basalt's default): d1 = |(X, Y, Z)|, k = xi d1 + Z,
        d2 = |(X, Y, k)|, (u, v) = (fx X, fy Y) / (alpha d2 + (1 - alpha) k) + (cx, cy), for every point inside the model's valid
        cone, points with Z <= 0 among them.  -1 < xi <= 1, 0 <= alpha <= 1.  A Camera whose model is AGX_LENS_DOUBLE_SPHERE and
        whose nine numbers are fx, fy, cx, cy, xi, alpha, 0, 0, 0."""
        return _DoubleSphereCamera(fx, fy, cx, cy, xi, alpha, 0.0, 0.0, 0.0)


class _EquidistantCamera(Camera):
    """Camera.equidistant's: the same nine numbers in the order the equidistant model reads them (k3, k4 by name; p1, p2 are the
    tuple's sixth and seventh fields, which hold k3 and k4)."""
    __slots__ = ()
    model = _ffi.AGX_LENS_EQUIDISTANT
    k3 = property(lambda self: self[6])
    k4 = property(lambda self: self[7])

    def __repr__(self):
        return "Camera.equidistant(fx=%r, fy=%r, cx=%r, cy=%r, k1=%r, k2=%r, k3=%r, k4=%r)" % tuple(self[:8])


class _DoubleSphereCamera(Camera):
    """Camera.double_sphere's: xi and alpha by name (the tuple's fourth and fifth fields, k1 and k2); the last three numbers are 0."""
    __slots__ = ()
    model = _ffi.AGX_LENS_DOUBLE_SPHERE
    xi = property(lambda self: self[4])
    alpha = property(lambda self: self[5])

    def __repr__(self):
        return "Camera.double_sphere(fx=%r, fy=%r, cx=%r, cy=%r, xi=%r, alpha=%r)" % tuple(self[:6])


def _camera(camera):
    """-> (AGX_LENS_*, the nine doubles) of a Camera or of nine numbers (radial-tangential)."""
    if camera is None:
        raise AgxError(_ffi.AGX_ERR_ARG, "camera must be given")
    camera = camera if isinstance(camera, Camera) else Camera(*camera)
    return camera.model, camera.as_doubles()


def board_pose(tags, cols, rows, camera, tag_size=1.0, first_id=0, spacing_ratio=0.3, max_err_sq=4.0, max_drop=0, min_tags=1, iterations=10,
               predict_missing=False, tag_status=0, tags_per_frame=None, return_iter_sums=False):
    """The host form of board_pose_enqueue for one frame (agx_board_pose_tail) without a device: the pose of the printed board
    (board_fit's layout in the plane Z = 0, centred on the board's centre, times tag_size) in the camera frame, Xc = R X + t, under
    `camera` (a Camera, or its nine numbers) through every corner of `tags`: a homography seed on undistorted corners, then
    `iterations` Gauss-Newton steps on the pixel residual, the best iterate kept; board_fit's outlier rounds on the pose's
    residuals; the predicted corners of the layout's tags through the lens model.
    -> dict: status AGX_FIT_*; for AGX_FIT_OK and AGX_FIT_LOOSE also R [3, 3] and t [3] float64, pose (the 12 numbers as stored),
    best_iter, err_sq, row_status, n_inliers, rms, pred as board_fit's; with return_iter_sums (a debug return, a second run through
    agx_debug_board_pose_sums) also iter_sums [iterations + 1], the sum of |e|^2 of every iterate of the last round (NaN: not
    reached)."""
    t = _tag_rows(tags)
    n = int(t.shape[0])
    cap = n if tags_per_frame is None else int(tags_per_frame)
    n_board = max(int(cols) * int(rows), 1) if 0 < int(cols) * int(rows) <= 4096 else 1
    pose = np.zeros(12, np.float64)
    sums = np.full(max(int(iterations), 0) + 1 if 0 <= int(iterations) <= 64 else 1, np.nan, np.float64)
    err, rst = np.full(max(n, 1), np.nan, np.float32), np.zeros(max(n, 1), np.uint32)
    pred = np.zeros(n_board, TagDetector.TAG_DTYPE)
    n_inl, n_pred, status, rms, best = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_float(0), C.c_uint32(0)
    model, cam = _camera(camera)
    head = (t.ctypes.data if n else None, cap, n, int(tag_status), int(cols), int(rows), int(first_id), float(spacing_ratio), float(tag_size))
    rest = (cam, float(max_err_sq), int(max_drop), int(min_tags), int(iterations), _ffi.AGX_FIT_PREDICT_MISSING if predict_missing else 0)
    outs = (pose.ctypes.data, err.ctypes.data, rst.ctypes.data, C.byref(n_inl), C.byref(rms), C.byref(best), pred.ctypes.data, C.byref(n_pred),
            C.byref(status))
    if model == _ffi.AGX_LENS_RADTAN:  # (the calls of a radial-tangential camera are the ones they were)
        st = _ffi.lib().agx_board_pose_tail(*head, *rest, *outs)
        if st == _ffi.AGX_OK and return_iter_sums:
            st = _ffi.lib().agx_debug_board_pose_sums(*head, *rest, C.byref(C.c_uint32(0)), sums.ctypes.data)
    else:
        st = _ffi.lib().agx_board_pose_tail_m(*head, model, *rest, *outs)
        if st == _ffi.AGX_OK and return_iter_sums:
            st = _ffi.lib().agx_debug_board_pose_sums_m(*head, model, *rest, C.byref(C.c_uint32(0)), sums.ctypes.data)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    out = {"status": status.value, "n_inliers": n_inl.value, "n_pred": n_pred.value}
    if status.value in (_ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE):
        out.update(R=pose[:9].reshape(3, 3), t=pose[9:], pose=pose, best_iter=best.value, err_sq=err[:n], row_status=rst[:n], rms=rms.value,
                   pred=pred[:n_pred.value].copy())
        if return_iter_sums:
            out["iter_sums"] = sums
    return out


def _fixed_mask(fixed):
    """fixed: the mask itself, or the held doubles by position 0 .. 8 or by Camera's field names -> the mask"""
    if isinstance(fixed, (int, np.integer)):
        mask = int(fixed)
    else:
        mask = 0
        for f in fixed:
            i = Camera._fields.index(f) if isinstance(f, str) and f in Camera._fields else f
            if isinstance(i, str) or not 0 <= int(i) < 9:
                raise AgxError(_ffi.AGX_ERR_ARG, "fixed names one of %s or a position 0 .. 8, got %r" % (", ".join(Camera._fields), f))
            mask |= 1 << int(i)
    if not 0 <= mask < 512:
        raise AgxError(_ffi.AGX_ERR_ARG, "fixed must be a mask below 512")
    return mask


def _lens_seed(lens, pinhole):
    """calibrate_seed's pinhole as the seed of the lens model `lens`"""
    fx, fy, cx, cy = pinhole[:4]
    if lens in ("radtan", _ffi.AGX_LENS_RADTAN):
        return Camera(fx, fy, cx, cy)
    if lens in ("equidistant", _ffi.AGX_LENS_EQUIDISTANT):
        return Camera.equidistant(fx, fy, cx, cy)
    if lens in ("double_sphere", _ffi.AGX_LENS_DOUBLE_SPHERE):
        # near the axis den = (1 + xi) Z: at xi = 0 the focal length is fx itself, whatever alpha is.  At xi = 0 the undamped system
        # of iterate 0 is refused (AGX_CALIB_SINGULAR): calibrate_batch steps from this seed under _seed_damping
        return Camera.double_sphere(fx, fy, cx, cy, 0.0, 0.5)
    raise AgxError(_ffi.AGX_ERR_ARG, "lens must be 'radtan', 'equidistant' or 'double_sphere', got %r" % (lens,))


def _seed_damping(camera, damping):
    """calibrate_batch's damping: the caller's, or by default 0 -- under the double-sphere model 1e-6, which carries the first step
    off the set xi = 0 where the undamped reduced system is singular (Levenberg's factor 1 + 1e-6 on the diagonals slows the last
    steps, it does not move the minimum: tests/test_calibrate_cpu.py measures the answer against scipy's)"""
    if damping is not None:
        return float(damping)
    return 1e-6 if _camera(camera)[0] == _ffi.AGX_LENS_DOUBLE_SPHERE else 0.0


def calib_report(report):
    """agx_calib_report's 552 bytes (calibrate_enqueue's report tensor on the host) -> dict: status AGX_CALIB_*, best_iter,
    iterations_run, n_frames_used, n_corners, rms, cost float64 [65] (NaN: an iterate that was not reached)."""
    r = np.ascontiguousarray(report).view(np.uint8).reshape(-1)
    if r.size != 552:
        raise AgxError(_ffi.AGX_ERR_ARG, "a report is 552 bytes")
    r = r.view(np.dtype(_ffi.CALIB_REPORT_DTYPE))[0]
    return {"status": int(r["status"]), "best_iter": int(r["best_iter"]), "iterations_run": int(r["iterations_run"]),
            "n_frames_used": int(r["n_frames_used"]), "n_corners": int(r["n_corners"]), "rms": float(r["rms"]), "cost": r["cost"].copy()}


def calibrate(tags, n_tags, cols, rows, camera, poses, row_status, fit_status, tag_size=1.0, first_id=0, spacing_ratio=0.3, fixed=0, damping=0.0,
              iterations=10, min_tags=1, min_frames=1, accept_loose=False, tag_status=None, raw=False):
    """The host form of calibrate_enqueue (agx_calibrate_tail) without a device: the camera's nine doubles, under `camera`'s lens
    model from `camera` as the seed, and every usable frame's pose, by `iterations` damped Gauss-Newton steps on the pixel residual
    of all inlier corners with the poses eliminated frame by frame; the iterate of the lowest cost is the answer (iterate 0 is the
    inputs).  tags: rows of TagDetector.TAG_DTYPE [N, T]; n_tags [N]; poses float64 [N, 12], row_status uint32 [N, T] and
    fit_status uint32 [N]: board_pose's pose, row_status and status per frame.  A frame is usable iff its status is AGX_FIT_OK
    (accept_loose: AGX_FIT_LOOSE too) and min_tags of its rows are AGX_FIT_ROW_INLIER.  fixed: a mask (bit i holds the i-th
    double), or the held doubles by Camera's field names or positions.
    -> dict: status AGX_CALIB_* and calib_report's fields; for AGX_CALIB_OK also camera (a Camera of the seed's model), pose
    float64 [N, 12] (the input's rows where a frame was not usable), frame_cost float32 [N], frame_n uint32 [N].  raw: also the
    output arrays as the call left them over guard values (camera_raw, pose_raw, ..., report_raw), for parity tests."""
    t = np.ascontiguousarray(tags)
    if t.dtype != TagDetector.TAG_DTYPE or t.ndim != 2:
        raise AgxError(_ffi.AGX_ERR_ARG, "tags must be rows of TAG_DTYPE [N, T]")
    n, tpf = int(t.shape[0]), int(t.shape[1])
    cnt = np.ascontiguousarray(n_tags, np.uint32).reshape(-1)
    pin = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    rst = np.ascontiguousarray(row_status, np.uint32).reshape(n, -1)
    fst = np.ascontiguousarray(fit_status, np.uint32).reshape(-1)
    tst = None if tag_status is None else np.ascontiguousarray(tag_status, np.uint32).reshape(-1)
    if not (cnt.shape[0] == n and pin.shape[0] == n and rst.shape[1] == tpf and fst.shape[0] == n and (tst is None or tst.shape[0] == n)):
        raise AgxError(_ffi.AGX_ERR_ARG, "n_tags, poses, row_status, fit_status (and tag_status) must have one entry per frame of tags")
    model, cam = _camera(camera)
    cam_out = np.full(9, np.nan, np.float64)
    pose = pin.copy()
    cost, fn = np.full(max(n, 1), np.nan, np.float32), np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    rep = np.zeros(1, np.dtype(_ffi.CALIB_REPORT_DTYPE))
    st = _ffi.lib().agx_calibrate_tail(n, t.ctypes.data if t.size else None, tpf, cnt.ctypes.data, None if tst is None else tst.ctypes.data,
                                       int(cols), int(rows), int(first_id), float(spacing_ratio), float(tag_size), model, cam, _fixed_mask(fixed),
                                       float(damping), int(iterations), int(min_tags), int(min_frames),
                                       _ffi.AGX_CALIB_ACCEPT_LOOSE if accept_loose else 0, pin.ctypes.data, rst.ctypes.data, fst.ctypes.data,
                                       cam_out.ctypes.data, pose.ctypes.data, cost.ctypes.data, fn.ctypes.data, rep.ctypes.data)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    out = calib_report(rep)
    if out["status"] == _ffi.AGX_CALIB_OK:
        seed = camera if isinstance(camera, Camera) else Camera(*camera)
        out.update(camera=type(seed)(*cam_out.tolist()), pose=pose, frame_cost=cost[:n], frame_n=fn[:n])
    if raw:
        out.update(camera_raw=cam_out, pose_raw=pose, frame_cost_raw=cost[:n], frame_n_raw=fn[:n], report_raw=rep)
    return out


def calibrate_seed(h, fit_status, img_size):
    """The closed-form seed of a calibration (agx_calibrate_seed_tail; OpenCV's initCameraMatrix2D), host only: from the
    homographies h [N, 9] or [N, 3, 3] of board_fit (board units -> pixels) whose status word is AGX_FIT_OK or AGX_FIT_LOOSE, the
    principal point ((w - 1) / 2, (h - 1) / 2) and fx, fy from the two orthogonality constraints per homography (Zhang 2000);
    zero distortion.  -> dict: status AGX_CALIB_OK with camera (a pinhole Camera), or AGX_CALIB_FEW / AGX_CALIB_SINGULAR."""
    hs = np.ascontiguousarray(h, np.float64).reshape(-1, 9)
    fst = np.ascontiguousarray(fit_status, np.uint32).reshape(-1)
    if hs.shape[0] != fst.shape[0]:
        raise AgxError(_ffi.AGX_ERR_ARG, "one status word per homography")
    cam = np.zeros(9, np.float64)
    status = C.c_uint32(0)
    st = _ffi.lib().agx_calibrate_seed_tail(hs.ctypes.data if hs.size else None, fst.ctypes.data if fst.size else None, int(hs.shape[0]),
                                            int(img_size[0]), int(img_size[1]), cam.ctypes.data, C.byref(status))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    out = {"status": status.value}
    if status.value == _ffi.AGX_CALIB_OK:
        out["camera"] = Camera(*cam.tolist())
    return out


def calib_param_jacobian(camera, xyz):
    """For tests of the arithmetic (agx_debug_calib_param_jacobian): the derivative of the projected pixel by the camera's nine
    doubles at points xyz [N, 3] of the camera frame -> float64 [N, 2, 9] (NaN where the point has no projection)."""
    p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((p.shape[0], 2, 9), np.float64)
    model, cam = _camera(camera)
    st = _ffi.lib().agx_debug_calib_param_jacobian(model, cam, p.ctypes.data if p.size else None, int(p.shape[0]), out.ctypes.data if p.size else None)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return out


def _rig_cameras(cameras, n_cams):
    """-> (int [C] of AGX_LENS_*, double [C * 9]) as ctypes arrays, from C Cameras (or nine numbers each)"""
    cameras = list(cameras)
    if len(cameras) != n_cams or not 2 <= n_cams <= 8:
        raise AgxError(_ffi.AGX_ERR_ARG, "one camera per camera of the rig, 2 .. 8 of them")
    pairs = [_camera(c) for c in cameras]
    models = (C.c_int * n_cams)(*[m for m, _ in pairs])
    nine = (C.c_double * (9 * n_cams))(*[float(v) for _, d in pairs for v in d])
    return models, nine


def rig_report(report):
    """agx_rig_report's 560 bytes (rig_calibrate_enqueue's report tensor on the host) -> dict: status AGX_RIG_*, best_iter,
    iterations_run, n_instants_used, n_frames_used, n_corners, n_cams_free, rms, cost float64 [65] (NaN: an iterate that was not
    reached)."""
    r = np.ascontiguousarray(report).view(np.uint8).reshape(-1)
    if r.size != 560:
        raise AgxError(_ffi.AGX_ERR_ARG, "a report is 560 bytes")
    r = r.view(np.dtype(_ffi.RIG_REPORT_DTYPE))[0]
    out = {k: int(r[k]) for k in ("status", "best_iter", "iterations_run", "n_instants_used", "n_frames_used", "n_corners", "n_cams_free")}
    out.update(rms=float(r["rms"]), cost=r["cost"].copy())
    return out


def rig_calibrate(tags, n_tags, cols, rows, cameras, poses, row_status, fit_status, extrinsics, tag_size=1.0, first_id=0, spacing_ratio=0.3,
                  damping=0.0, iterations=10, min_tags=1, min_cams=2, min_instants=1, accept_loose=False, tag_status=None, raw=False, in_place=False):
    """The host form of rig_calibrate_enqueue (agx_rig_calibrate_tail) without a device: the extrinsics E_c (camera from rig,
    E_0 the identity) of C = 2 .. 8 cameras and the board's pose T_s (rig from board) at every usable instant, by `iterations`
    damped Gauss-Newton steps on the pixel residual of all inlier corners under E_c o T_s with the T_s eliminated instant by
    instant; the iterate of the lowest cost is the answer (iterate 0 is the inputs).  tags: rows of TagDetector.TAG_DTYPE
    [C, S, T] (camera c at instant s); n_tags [C, S]; poses float64 [C, S, 12], row_status uint32 [C, S, T] and fit_status uint32
    [C, S]: board_pose's answers per frame under cameras[c]; extrinsics float64 [C, 12]: the seed (rig_seed).  A frame is usable
    as calibrate's; an instant iff min_cams of its frames are; a camera without a counted frame keeps its seed.
    -> dict: status AGX_RIG_* and rig_report's fields; for AGX_RIG_OK also extrinsics [C, 12], rig_pose [S, 12] (NaN rows for
    unusable instants), frame_cost float32 [C, S], frame_n uint32 [C, S], cam_n uint32 [C].  raw: also the output arrays as the
    call left them over guard values (extrinsics_raw, ...).  in_place: the seed array is the output array (the aliased call)."""
    t = np.ascontiguousarray(tags)
    if t.dtype != TagDetector.TAG_DTYPE or t.ndim != 3:
        raise AgxError(_ffi.AGX_ERR_ARG, "tags must be rows of TAG_DTYPE [C, S, T]")
    nc, ns, tpf = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    n = nc * ns
    cnt = np.ascontiguousarray(n_tags, np.uint32).reshape(-1)
    pin = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    rst = np.ascontiguousarray(row_status, np.uint32).reshape(-1, max(tpf, 1))
    fst = np.ascontiguousarray(fit_status, np.uint32).reshape(-1)
    tst = None if tag_status is None else np.ascontiguousarray(tag_status, np.uint32).reshape(-1)
    ein = np.array(extrinsics, np.float64).reshape(-1, 12)
    if not (cnt.shape[0] == n and pin.shape[0] == n and rst.shape[0] == n and fst.shape[0] == n and (tst is None or tst.shape[0] == n) and ein.shape[0] == nc):
        raise AgxError(_ffi.AGX_ERR_ARG, "n_tags, poses, row_status, fit_status (and tag_status) must have one entry per frame of tags, extrinsics one per camera")
    models, cams = _rig_cameras(cameras, nc)
    ext = ein if in_place else np.full((nc, 12), np.nan, np.float64)
    rig_pose = np.full((max(ns, 1), 12), np.nan, np.float64)
    cost, fn = np.full(max(n, 1), np.nan, np.float32), np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    cam_n = np.full(nc, 0xFFFFFFFF, np.uint32)
    rep = np.zeros(1, np.dtype(_ffi.RIG_REPORT_DTYPE))
    st = _ffi.lib().agx_rig_calibrate_tail(nc, ns, t.ctypes.data if t.size else None, tpf, cnt.ctypes.data, None if tst is None else tst.ctypes.data,
                                           int(cols), int(rows), int(first_id), float(spacing_ratio), float(tag_size), models, cams, float(damping),
                                           int(iterations), int(min_tags), int(min_cams), int(min_instants),
                                           _ffi.AGX_CALIB_ACCEPT_LOOSE if accept_loose else 0, pin.ctypes.data, rst.ctypes.data, fst.ctypes.data,
                                           ein.ctypes.data, ext.ctypes.data, rig_pose.ctypes.data, cost.ctypes.data, fn.ctypes.data, cam_n.ctypes.data,
                                           rep.ctypes.data)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    out = rig_report(rep)
    if out["status"] == _ffi.AGX_RIG_OK:
        out.update(extrinsics=ext, rig_pose=rig_pose[:ns], frame_cost=cost[:n].reshape(nc, ns), frame_n=fn[:n].reshape(nc, ns), cam_n=cam_n)
    if raw:
        out.update(extrinsics_raw=ext, rig_pose_raw=rig_pose[:ns], frame_cost_raw=cost[:n], frame_n_raw=fn[:n], cam_n_raw=cam_n, report_raw=rep)
    return out


def rig_seed(poses, fit_status, frame_n=None):
    """The closed-form seed of a rig calibration (agx_rig_seed_tail), host only: poses float64 [C, S, 12] and fit_status [C, S] of
    board_pose per frame, frame_n [C, S] (correspondences per frame) or None.  Cameras attach level by level from camera 0, each
    through the lowest-numbered camera attached earlier with which it shares an instant where both poses are AGX_FIT_OK, at the
    shared instant with the most correspondences (the lowest at ties): E_c = pose[c, s] o pose[r, s]^-1 o E_r.
    -> dict: extrinsics float64 [C, 12], cam_status uint32 [C] (AGX_RIG_CAM_ATTACHED, or AGX_RIG_CAM_DETACHED with the identity)."""
    p = np.ascontiguousarray(poses, np.float64)
    if p.ndim != 3 or p.shape[2] != 12:
        raise AgxError(_ffi.AGX_ERR_ARG, "poses must be [C, S, 12]")
    nc, ns = int(p.shape[0]), int(p.shape[1])
    fst = np.ascontiguousarray(fit_status, np.uint32).reshape(-1)
    fn = None if frame_n is None else np.ascontiguousarray(frame_n, np.uint32).reshape(-1)
    if fst.shape[0] != nc * ns or (fn is not None and fn.shape[0] != nc * ns):
        raise AgxError(_ffi.AGX_ERR_ARG, "one status word (and one count) per pose")
    ext, cst = np.zeros((nc, 12), np.float64), np.zeros(nc, np.uint32)
    st = _ffi.lib().agx_rig_seed_tail(nc, ns, p.ctypes.data if p.size else None, fst.ctypes.data if fst.size else None,
                                      None if fn is None else fn.ctypes.data, ext.ctypes.data, cst.ctypes.data)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return {"extrinsics": ext, "cam_status": cst}


def rig_jacobian(camera, extrinsic, rig_pose, XY):
    """For tests of the arithmetic (agx_debug_rig_jacobian): the derivative of the projected pixel of board points XY [N, 2] under
    camera, extrinsic [12] (None: camera 0) and rig_pose [12] by the 6 + 6 update unknowns -> float64 [N, 2, 12] (NaN where the
    point has no projection)."""
    p = np.ascontiguousarray(XY, np.float64).reshape(-1, 2)
    out = np.zeros((p.shape[0], 2, 12), np.float64)
    model, cam = _camera(camera)
    e = None if extrinsic is None else np.ascontiguousarray(extrinsic, np.float64).reshape(12)
    t = np.ascontiguousarray(rig_pose, np.float64).reshape(12)
    st = _ffi.lib().agx_debug_rig_jacobian(model, cam, None if e is None else e.ctypes.data, t.ctypes.data, p.ctypes.data if p.size else None,
                                           int(p.shape[0]), out.ctypes.data if p.size else None)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return out


def _rectify_args(camera, src_size, dst_size, new_camera, rotation):
    """-> (AGX_LENS_*, camera's nine doubles, new_camera's four, rotation's nine or None, (src_w, src_h), (dst_w, dst_h)).
    Defaults: the source size, the camera's own fx fy cx cy, no rotation."""
    model, cam = _camera(camera)
    nc = [float(v) for v in (cam[:4] if new_camera is None else new_camera)][:9]
    if len(nc) not in (4, 9):
        raise AgxError(_ffi.AGX_ERR_ARG, "new_camera must be fx, fy, cx, cy (or a Camera, whose first four numbers are read)")
    rot = None
    if rotation is not None:
        r = np.asarray(rotation, np.float64)
        if r.size != 9:
            raise AgxError(_ffi.AGX_ERR_ARG, "rotation must be a 3 x 3 matrix")
        rot = (C.c_double * 9)(*r.ravel())
    src = (int(src_size[0]), int(src_size[1]))
    dst = src if dst_size is None else (int(dst_size[0]), int(dst_size[1]))
    return model, cam, (C.c_double * 4)(*nc[:4]), rot, src, dst


def rectify_map(camera, src_size, dst_size=None, new_camera=None, rotation=None, row_stride=None):
    """The rectification map of `camera` (a Camera of any lens model) without a device (agx_rectify_map_tail): for every pixel
    (i, j) of the ideal pinhole new_camera = (fx', fy', cx', cy') of dst_size = (w, h) the sensor pixel it comes from -- the ray
    ((i - cx') / fx', (j - cy') / fy', 1), turned by rotation (3 x 3, rectified frame -> camera frame), projected through the
    lens model -- in units of 1/32 px of the src_size = (w, h) sensor image, rounded to nearest.
    -> int32 [dst_h, dst_w, 2]: (mx, my), or (AGX_MAP_NONE, AGX_MAP_NONE) where the ray has no pixel in the source.  Defaults: the
    source's size, the camera's own fx fy cx cy, no rotation.  row_stride: bytes between the rows of the array the map is a view
    of (padding bytes keep 0x5a).  Choosing a new_camera inside the radius where a radial-tangential polynomial is monotone is
    the caller's job: beyond it far rays fold back into the image."""
    model, cam, ncam, rot, (sw, sh), (dw, dh) = _rectify_args(camera, src_size, dst_size, new_camera, rotation)
    stride = 8 * max(dw, 0) if row_stride is None else int(row_stride)
    buf = None
    if 1 <= dw <= 16384 and 1 <= dh <= 16384 and stride >= 8 * dw and stride % 8 == 0:
        buf = np.full((dh, stride // 4), 0x5a5a5a5a, np.int32)
    st = _ffi.lib().agx_rectify_map_tail(model, cam, ncam, rot, sw, sh, dw, dh, None if buf is None else buf.ctypes.data, stride)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return buf[:, :2 * dw].reshape(dh, dw, 2)


def _gray_host(a, what):
    """-> (array [N, H, W], agx_format, pixel bytes, had no frame axis) of a host image or batch, uint8 or uint16, rows may be padded"""
    a = np.asarray(a)
    lone = a.ndim == 2
    a = a[None] if lone else a
    if a.ndim != 3 or a.dtype not in (np.uint8, np.uint16) or 0 in a.shape or a.strides[2] != a.itemsize or a.strides[1] < 0 or a.strides[0] < 0:
        raise AgxError(_ffi.AGX_ERR_ARG, "%s must be uint8 or uint16, [H, W] or [N, H, W], with adjacent pixels in a row" % what)
    return a, (_ffi.AGX_L8 if a.dtype == np.uint8 else _ffi.AGX_L16), a.itemsize, lone


def remap(image, map, border=0, out=None):
    """image ([H, W] or [N, H, W], uint8 or uint16; rows and frames may be padded views) through a rectification map (int32
    [dst_h, dst_w, 2] in 1/32 px: rectify_map's, or the caller's own) without a device (agx_remap_tail): per destination pixel with
    entry (mx, my), x0 = mx >> 5, ax = mx & 31, x1 = min(x0 + 1, W - 1), the same in y, and
    ((32 - ax)(32 - ay) p00 + ax (32 - ay) p10 + (32 - ax) ay p01 + ax ay p11 + 512) >> 10 -- integers only; `border` where the
    entry is AGX_MAP_NONE or otherwise not inside the source.  -> [dst_h, dst_w] or [N, dst_h, dst_w] of the image's dtype (out:
    the caller's array of that shape, rows and frames may be padded)."""
    a, fmt, px, lone = _gray_host(image, "image")
    m = np.asarray(map)
    if m.dtype != np.int32 or m.ndim != 3 or m.shape[2] != 2 or 0 in m.shape or m.strides[2] != 4 or m.strides[1] != 8 or m.strides[0] < 0:
        raise AgxError(_ffi.AGX_ERR_ARG, "map must be int32 [dst_h, dst_w, 2] whose rows are packed")
    n, dh, dw = a.shape[0], m.shape[0], m.shape[1]
    if out is None:
        res = np.empty((n, dh, dw), a.dtype)
    else:
        res = _gray_host(out, "out")[0]
        if res.dtype != a.dtype or res.shape != (n, dh, dw):
            raise AgxError(_ffi.AGX_ERR_ARG, "out must have the image's dtype and the shape [N, dst_h, dst_w]")
    rs = lambda t: t.strides[1] if t.shape[1] > 1 else t.shape[2] * px  # (a lone row or frame has no stride of its own)
    fs = lambda t: t.strides[0] if t.shape[0] > 1 else rs(t) * t.shape[1]
    st = _ffi.lib().agx_remap_tail(a.ctypes.data, n, a.shape[2], a.shape[1], rs(a), fs(a), fmt, m.ctypes.data, m.strides[0] if dh > 1 else 8 * dw, dw, dh,
                                   res.ctypes.data, rs(res), fs(res), int(border))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    if out is not None:
        return out
    return res[0] if lone else res


def decimate(image, factor, out=None):
    """image ([H, W] or [N, H, W], uint8 or uint16; rows and frames may be padded views) averaged down by `factor` in 2 .. 4 without
    a device (agx_decimate_tail): out(X, Y) = (sum of the factor x factor pixels at (factor X + dx, factor Y + dy) + factor^2 // 2)
    // factor^2 -- integers only, round half up; trailing columns and rows are dropped.  The centre of out(X, Y) is the image
    position (factor X + (factor - 1) / 2, factor Y + (factor - 1) / 2): what refine_windows_enqueue's factor= undoes.
    -> [H // factor, W // factor] or [N, H // factor, W // factor] of the image's dtype (out: the caller's array of that shape, rows
    and frames may be padded)."""
    a, fmt, px, lone = _gray_host(image, "image")
    f = int(factor)
    n, dh, dw = a.shape[0], a.shape[1] // max(f, 1), a.shape[2] // max(f, 1)
    if out is None:
        res = np.empty((n, max(dh, 1), max(dw, 1)), a.dtype)  # (an output side of 0 is the library's to refuse)
    else:
        res = _gray_host(out, "out")[0]
        if res.dtype != a.dtype or res.shape != (n, dh, dw):
            raise AgxError(_ffi.AGX_ERR_ARG, "out must have the image's dtype and the shape [N, H // factor, W // factor]")
    rs = lambda t: t.strides[1] if t.shape[1] > 1 else t.shape[2] * px  # (a lone row or frame has no stride of its own)
    fs = lambda t: t.strides[0] if t.shape[0] > 1 else rs(t) * t.shape[1]
    st = _ffi.lib().agx_decimate_tail(a.ctypes.data, n, a.shape[2], a.shape[1], rs(a), fs(a), fmt, f, res.ctypes.data, rs(res), fs(res))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    if out is not None:
        return out
    return res[0] if lone else res


def rectified_points(points, camera, new_camera, rotation=None):
    """Points (x, y) of the rectified image, float32 [..., 2], to the sensor pixels they come from, without a device
    (agx_rectified_points_tail): rectify_map's ray, rotation and projection in binary64 (the map's entry is this function at integer
    positions), rounded to float32; (NaN, NaN) where the ray has no projection.  new_camera None: the camera's own fx fy cx cy."""
    model, cam, ncam, rot, _, _ = _rectify_args(camera, (1, 1), None, new_camera, rotation)
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim < 1 or p.shape[-1] != 2:
        raise AgxError(_ffi.AGX_ERR_ARG, "points must be [..., 2]")
    out = np.empty_like(p)
    st = _ffi.lib().agx_rectified_points_tail(model, cam, ncam, rot, p.ctypes.data if p.size else None, 8, p.size // 2,
                                              out.ctypes.data if p.size else None, 8)
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    return out


def _render_params(fmt, black, white, background, page_margin, supersample, keep_background):
    """-> the agx_render_params of the keywords (white None: the format's largest value; background None: half of it)"""
    top = 65535 if fmt == _ffi.AGX_L16 else 255
    white = top if white is None else white
    background = top // 2 + 1 if background is None else background
    for v in (black, white, background, supersample):
        if not 0 <= int(v) < 2 ** 32:
            raise AgxError(_ffi.AGX_ERR_ARG, "black, white, background and supersample must be unsigned 32-bit numbers")
    return _ffi.RenderParams(int(black), int(white), int(background), float(page_margin), int(supersample),
                             _ffi.AGX_RENDER_KEEP_BACKGROUND if keep_background else 0)


def board_pose_looking_at(distance, tilt_x=0.0, tilt_y=0.0, roll=0.0, offset=(0.0, 0.0)):
    """The pose (R [3, 3], t [3], float64; Xc = R X + t) of a board that faces the camera `distance` (in tag_size's unit) down the
    optical axis, its centre moved by `offset` (x, y) in the camera frame.  At zero angles the board's X is the image's right and
    its Y the image's up -- tag first_id sits at the bottom left, as Kalibr prints it -- so R = diag(1, -1, -1).  tilt_x, tilt_y and
    roll (degrees) then turn the board about the camera's x, y and z axes through the board's centre: R = Rz(roll) Ry(tilt_y)
    Rx(tilt_x) diag(1, -1, -1)."""
    ax, ay, az = (float(np.deg2rad(v)) for v in (tilt_x, tilt_y, roll))
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return rz @ ry @ rx @ np.diag([1.0, -1.0, -1.0]), np.array([float(offset[0]), float(offset[1]), float(distance)], np.float64)


def pose_rows(poses):
    """(R, t), a list of them, or an array [12] / [N, 12] -> contiguous float64 [N, 12]: R row major, then t"""
    if isinstance(poses, tuple) and len(poses) == 2 and np.ndim(poses[0]) == 2:
        poses = [poses]
    if isinstance(poses, (list, tuple)) and len(poses) and isinstance(poses[0], (list, tuple)) and len(poses[0]) == 2 and np.ndim(poses[0][0]) == 2:
        poses = [np.concatenate([np.asarray(r, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]) for r, t in poses]
    a = np.ascontiguousarray(poses, np.float64)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != 12:
        raise AgxError(_ffi.AGX_ERR_ARG, "poses must be (R, t), a list of them, or an array [N, 12]")
    return a


def render_boards(size, cols, rows, camera, poses, family="T36H11", first_id=0, spacing_ratio=0.3, tag_size=1.0, black=0, white=None,
                  background=None, page_margin=0.5, supersample=3, keep_background=False, dtype=np.uint8, out=None):
    """The printed board (Kalibr's AprilGrid layout of board_fit: tag first_id + r*cols + c at column c, row r; black squares of
    side spacing_ratio at the lattice points; the tags of `family` with their borders and code bits) as `camera` (a Camera of any
    lens model) sees it from each of `poses` ((R, t), a list of them or [N, 12]; Xc = R X + t with the board in the plane Z = 0,
    centred, in tag_size's unit: board_pose's pose) without a device (agx_render_boards_tail, once per frame).  A pixel takes
    supersample x supersample samples; each is taken back to the board through the inverse of board_pose's forward projection
    (a seed from the lens's unprojection, 4 Newton steps, accepted within 2^-20 px) and the pixel is the rounded mean of white,
    black and background over its samples, in integers.  page_margin: the white border around the board, in tag sides.
    keep_background: the frame's own pixels are the background (an overlay on `out`); a pixel with no sample on the page is not
    written.  size (w, h); dtype uint8 or uint16; out: the caller's array [N, H, W] (or [H, W] for one pose), rows and frames may
    be padded.
    -> (frames [N, H, W], truth [N, rows * cols] rows of TagDetector.TAG_DTYPE -- the projected corners of every tag in id order,
    NaN without a projection --, n_truth uint32 [N], status uint32 [N] AGX_RENDER_*)."""
    p = pose_rows(poses)
    n, (w, h) = p.shape[0], (int(size[0]), int(size[1]))
    if out is None:
        dt = np.dtype(dtype)
        if dt not in (np.uint8, np.uint16) or keep_background:
            raise AgxError(_ffi.AGX_ERR_ARG, "dtype must be uint8 or uint16; keep_background needs out")
        res = np.zeros((n, max(h, 0), max(w, 0)), dt)
        fmt, px = (_ffi.AGX_L8 if dt == np.uint8 else _ffi.AGX_L16), dt.itemsize
        if res.size == 0:
            res = np.zeros((n, 1, 1), dt)  # (the library refuses the size)
    else:
        res, fmt, px, _ = _gray_host(out, "out")
        if res.shape != (n, h, w):
            raise AgxError(_ffi.AGX_ERR_ARG, "out must have the shape [N, H, W] of the poses and size")
    model, cam = _camera(camera)
    params = _render_params(fmt, black, white, background, page_margin, supersample, keep_background)
    fam = int(TagFamily.from_str(family) if isinstance(family, str) else family)
    n_board = int(cols) * int(rows) if 0 < int(cols) * int(rows) <= 4096 else 1
    truth = np.zeros((n, n_board), TagDetector.TAG_DTYPE)
    n_truth, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rs = res.strides[1] if res.shape[1] > 1 else res.shape[2] * px
    for f in range(n):
        st = _ffi.lib().agx_render_boards_tail(w, h, rs, fmt, fam, int(cols), int(rows), int(first_id), float(spacing_ratio), float(tag_size), model, cam,
                                               p[f].ctypes.data, C.addressof(params), res[f].ctypes.data, truth[f].ctypes.data,
                                               n_truth[f:].ctypes.data, status[f:].ctypes.data)
        if st != _ffi.AGX_OK:
            raise AgxError(st)
    return (res if out is None else out), truth, n_truth, status


def _find_board_call(call, saddles, cap, keep=None):
    a = np.asarray(saddles)
    if a.dtype == SADDLE_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 5)
    quads = np.zeros((max(int(cap), 0), 4), np.uint32)
    n_quads, status = C.c_uint32(0), C.c_uint32(0)
    if keep is not None:
        keep._batch = keep._detect = keep._refine = keep._decode = keep._grow = keep._find = None
    call(a.ctypes.data if a.shape[0] else None, a.shape[0], quads.ctypes.data if quads.shape[0] else None, quads.shape[0], C.byref(n_quads),
         C.byref(status))
    found = status.value == _ffi.AGX_BOARD_FOUND
    return quads[:n_quads.value if found else 0].copy(), status.value, n_quads.value


def find_board_tail(saddles, cap=128):
    """The host's try_find_best_board (src/detector.rs:588-639) without a device: saddles a SADDLE_DTYPE array (or [n, 5] float32)
    -> (quads [n_quads, 4] uint32 indices into the list, status AGX_BOARD_*, n_quads) -- what TagDetector.find_board returns."""
    def call(*a):
        st = _ffi.lib().agx_find_board_tail(*a)
        if st != _ffi.AGX_OK:
            raise AgxError(st)
    return _find_board_call(call, saddles, cap)


def grow_board_tail(saddles, seeds, spacing_ratio=0.3, stop_score=0, fix_missing=True, cap=128, point_status=None):
    """The host form of boards from seed quads (src/board.rs:26-112; agx_grow_board_tail) without a device: saddles a SADDLE_DTYPE
    array (or [n, 5] float32), seeds [n_seeds, 4] indices into it -> (quads [n_quads, 4] uint32, status AGX_BOARD_*, n_quads,
    seed_scores [n_seeds] uint32, best_seed); seed_scores and best_seed are None unless a board was found."""
    a = np.asarray(saddles)
    if a.dtype == SADDLE_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 5)
    s = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 4)
    ps = None if point_status is None else np.ascontiguousarray(point_status, np.uint32).reshape(a.shape[0])
    quads = np.zeros((max(int(cap), 0), 4), np.uint32)
    scores = np.zeros(s.shape[0], np.uint32)
    n_quads, status, best = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = _ffi.lib().agx_grow_board_tail(a.ctypes.data if a.shape[0] else None, a.shape[0], ps.ctypes.data if ps is not None and ps.size else None,
                                        s.ctypes.data if s.shape[0] else None, s.shape[0], float(spacing_ratio), int(stop_score),
                                        _ffi.AGX_GROW_FIX_MISSING if fix_missing else 0, quads.ctypes.data if quads.shape[0] else None,
                                        quads.shape[0], C.byref(n_quads), C.byref(status), scores.ctypes.data if s.shape[0] else None, C.byref(best))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    found = status.value == _ffi.AGX_BOARD_FOUND
    some = found or status.value == _ffi.AGX_BOARD_CAPACITY
    return quads[:n_quads.value if found else 0].copy(), status.value, n_quads.value, scores if some else None, best.value if some else None


def init_quads_tail(saddles, seeds=None, max_seeds=None, n_nearest=50, cap=1024, point_status=None):
    """The host form of init_quads for a list of seeds (src/detector.rs:543-586; agx_init_quads_tail) without a device: saddles a
    SADDLE_DTYPE array (or [n, 5] float32); seeds: indices into it, or None for the reference's own seeds (:601-616), at most
    max_seeds of them (default 30; with seeds: default all of them) -> (quads [n_quads, 4] uint32, status AGX_BOARD_*, n_quads,
    seed_quad_counts [max_seeds] uint32, seeds_taken uint32); the last two are None for AGX_BOARD_INPUT."""
    a = np.asarray(saddles)
    if a.dtype == SADDLE_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 5)
    s = None if seeds is None else np.ascontiguousarray(seeds, np.uint32).reshape(-1)
    if max_seeds is None:
        max_seeds = 30 if s is None else max(1, s.shape[0])
    room = max(int(max_seeds), 0)
    ps = None if point_status is None else np.ascontiguousarray(point_status, np.uint32).reshape(a.shape[0])
    quads = np.zeros((max(int(cap), 0), 4), np.uint32)
    per_seed, taken = np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    none = np.zeros(1, np.uint32)  # (a non-null pointer for an empty seed list: null asks for the reference's seeds)
    n_quads, status, n_taken = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = _ffi.lib().agx_init_quads_tail(a.ctypes.data if a.shape[0] else None, a.shape[0], ps.ctypes.data if ps is not None and ps.size else None,
                                        None if s is None else (s.ctypes.data if s.shape[0] else none.ctypes.data), 0 if s is None else s.shape[0],
                                        room, int(n_nearest), quads.ctypes.data if quads.shape[0] else None, quads.shape[0], C.byref(n_quads),
                                        C.byref(status), per_seed.ctypes.data if room else None, taken.ctypes.data if room else None,
                                        C.byref(n_taken))
    if st != _ffi.AGX_OK:
        raise AgxError(st)
    found = status.value == _ffi.AGX_BOARD_FOUND
    bad = status.value == _ffi.AGX_BOARD_INPUT
    return (quads[:n_quads.value if found else 0].copy(), status.value, n_quads.value, None if bad else per_seed,
            None if bad else taken[:n_taken.value].copy())


class DetectorGroup:
    """Several GPUs of one node from ONE process over the C ABI's detector groups (agx_group_*):
    rank r = one TagDetector on devices[r] with its own stream; a batch shards by frame and the
    per-rank result slabs are gathered to devices[0] (transport "rccl": ncclSend / ncclRecv over
    xGMI; "peer": hipMemcpyPeerAsync -- also accepts the same device twice, for one-GPU boxes)."""

    def __init__(self, tag_family, devices, optional_detector_params=None, transport="rccl", blur_sigma=None):
        self._lib = _ffi.lib()
        self._g = C.c_void_p()
        fam = TagFamily.from_str(tag_family) if isinstance(tag_family, str) else TagFamily(tag_family)
        prm = optional_detector_params._c() if optional_detector_params is not None else None
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        tr = {"rccl": _ffi.AGX_GATHER_RCCL, "peer": _ffi.AGX_GATHER_PEER}[transport]
        st = self._lib.agx_group_create(int(fam), C.byref(prm) if prm is not None else None, devs, len(devices), tr,
                                        C.byref(self._g))
        if st != _ffi.AGX_OK:
            self._g = C.c_void_p()
            raise AgxError(st, "agx_group_create: %s" % self._lib.agx_group_last_error(None).decode())
        self.devices = list(devices)
        self._keep = None
        self._frames_per_rank = 0
        self._detect = None
        if blur_sigma is not None:
            try:
                self.set_blur_sigma(blur_sigma)
            except AgxError:
                self.close()
                raise

    def set_blur_sigma(self, sigma):
        """TagDetector.set_blur_sigma on every rank's detector."""
        for r in range(len(self.devices)):
            h = C.c_void_p(self._lib.agx_group_detector(self._g, r))
            st = self._lib.agx_detector_set_blur_sigma(h, float(sigma))
            if st != _ffi.AGX_OK:
                raise AgxError(st, "rank %d: %s" % (r, self._lib.agx_last_error(h).decode()))

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._lib.agx_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self._lib.agx_group_size(self._g)

    def _check(self, st):
        if st != _ffi.AGX_OK:
            raise AgxError(st, self._lib.agx_group_last_error(self._g).decode())

    def saddles_enqueue(self, frames_per_rank, records_per_frame=0, format=None):
        """frames_per_rank: one contiguous device tensor per rank (shapes and format= as TagDetector.saddles_batch_enqueue,
        same shape everywhere), rank r's on devices[r]; the caller has made sure they are ready
        (e.g. torch.cuda.synchronize): the ranks run on their detectors' own streams."""
        assert len(frames_per_rank) == len(self.devices)
        fmt, bpp = TagDetector._tensor_format(frames_per_rank[0], format)
        n, w, h, rs, fs = TagDetector._tensor_geometry(frames_per_rank[0], fmt, bpp)
        for t in frames_per_rank:
            assert tuple(t.shape) == tuple(frames_per_rank[0].shape) and t.is_contiguous() and t.is_cuda
        ptrs = (C.c_void_p * len(frames_per_rank))(*[t.data_ptr() for t in frames_per_rank])
        self._check(self._lib.agx_group_saddles_enqueue(self._g, ptrs, n, w, h, rs, fs, fmt,
                                                        records_per_frame))
        self._keep = list(frames_per_rank)
        self._frames_per_rank = n

    def saddles_fetch(self, cap_per_frame=2048, raise_on_overflow=True):
        """-> (list of SADDLE_DTYPE arrays, global frame r*F + f; status array)."""
        n = self._frames_per_rank * len(self.devices)
        out = np.zeros((n, cap_per_frame), SADDLE_DTYPE)
        counts = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        st = self._lib.agx_group_saddles_fetch(self._g, out.ctypes.data, cap_per_frame, counts.ctypes.data,
                                               status.ctypes.data)
        if st != _ffi.AGX_OK and (raise_on_overflow or st != _ffi.AGX_ERR_CAPACITY):
            self._check(st)
        self._keep = None
        # a frame whose list is merely longer than cap_per_frame reports its length (status -3): fetch again with room
        self.last_counts = counts
        return [out[i, : counts[i]].copy() if status[i] == 0 else out[i, :0].copy() for i in range(n)], status

    def detect_enqueue(self, frames_per_rank, cap=1024, tags_per_frame=0, format=None):
        """detect() over one contiguous device tensor per rank (as saddles_enqueue; every integer layout, float32 planes are
        refused): every rank's chain, device tail and tag packing, then the gather of the packed tag slabs to devices[0].
        Returns immediately; detect_fetch waits.  tags_per_frame: average tags per frame a rank's slab holds (0 = 128)."""
        assert len(frames_per_rank) == len(self.devices)
        fmt, bpp = TagDetector._tensor_format(frames_per_rank[0], format)
        if fmt == _ffi.AGX_LF32:
            raise AgxError(_ffi.AGX_ERR_FORMAT, "detect takes frames of integer pixels")
        n, w, h, rs, fs = TagDetector._tensor_geometry(frames_per_rank[0], fmt, bpp)
        for t in frames_per_rank:
            assert tuple(t.shape) == tuple(frames_per_rank[0].shape) and t.is_contiguous() and t.is_cuda
        ptrs = (C.c_void_p * len(frames_per_rank))(*[t.data_ptr() for t in frames_per_rank])
        self._detect = None
        self._check(self._lib.agx_group_detect_enqueue(self._g, ptrs, n, w, h, rs, fs, fmt, cap, tags_per_frame))
        self._keep = list(frames_per_rank)
        self._frames_per_rank = n
        self._detect = (n * len(self.devices), cap)

    def detect_fetch_raw(self, n_threads=0):
        """agx_group_detect_fetch -> (rc, out [N, cap] TAG_DTYPE, counts uint32 [N], status int32 [N]), global frame r*F + f, as
        TagDetector.detect_batch_fetch_raw.  Nothing is raised for a frame status."""
        if self._detect is None:
            raise AgxError(_ffi.AGX_ERR_STATE, "no detect batch enqueued")
        n, cap = self._detect
        self._detect = None
        out = np.zeros((n, cap), TagDetector.TAG_DTYPE)
        counts = np.zeros(n, np.uint32)
        status = np.full(n, _ffi.AGX_ERR_STATE, np.int32)
        rc = self._lib.agx_group_detect_fetch(self._g, out.ctypes.data, counts.ctypes.data, status.ctypes.data, n_threads)
        self._keep = None
        if rc not in (_ffi.AGX_OK, _ffi.AGX_ERR_CAPACITY):
            self._check(rc)
        return rc, out, counts, status

    def detect_fetch(self, n_threads=0, raise_on_overflow=True):
        """-> (list of {tag_id: 4x2 corners} per global frame r*F + f, None for a frame that is not AGX_OK; status array)."""
        rc, out, counts, status = self.detect_fetch_raw(n_threads)
        if rc != _ffi.AGX_OK and raise_on_overflow:
            self._check(rc)
        res = [None if status[i] != 0 else {int(t["id"]): t["xy"].reshape(4, 2).copy() for t in out[i, : counts[i]]}
               for i in range(len(counts))]
        return res, status
