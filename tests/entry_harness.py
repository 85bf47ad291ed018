"""Raw ctypes calls of every batch entry point, shared by tests/test_gpu_batch_state.py and tests/test_gpu_entry_arg_matrix.py.

Both modules pin statuses only, so every buffer here is zero-filled (no saddle, no tag, nothing to overflow) and every call
goes straight to the C ABI: no wrapper of detector.py gets to refuse an argument first.  One detector, one group of one rank
and one set of device buffers per module (Harness)."""
import ctypes as C

import numpy as np

OK, ERR_ARG, ERR_FORMAT, ERR_STATE = 0, -1, -2, -7
L8, L16, LF32, LA8 = 0, 1, 3, 4
DBG_MIN = 2                 # agx_debug_fetch's cheapest item: one float of the chain's batch
MAX_FRAMES = 65535
PIN_BYTES = (1 << 31) + (1 << 20)  # the frames' pool: a second row 0x7fffffff bytes behind the first is still inside it
LEAD = 4096                 # frames start this far into the pool
# which fetch resolves the batch of which enqueue (agx_planes_enqueue has none)
FETCH_OF = {"saddles": "agx_saddles_batch_fetch", "detect": "agx_detect_batch_fetch", "refine": "agx_refine_points_fetch",
            "decode": "agx_decode_quads_fetch", "find": "agx_find_boards_fetch"}
KINDS = ("saddles", "detect", "refine", "decode", "find", "planes")
FETCHES = ("saddles", "detect", "refine", "decode", "find", "debug")


class Harness:
    def __init__(self):
        import torch
        import aprilgrid_rs_amd as A
        from aprilgrid_rs_amd import _ffi
        self.torch = torch
        self.lib = _ffi.lib()
        self.det = A.TagDetector("t36h11", None, device=0)
        self.h = self.det._h
        self.det.set_limits(64, 64, 64)  # small per-frame lists: a batch of 65535 tiny frames stays a small workspace
        self.group = A.DetectorGroup("t36h11", [0], None, transport="peer")
        self.g = self.group._g
        self.rank0 = C.c_void_p(self.lib.agx_group_detector(self.g, 0))
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.pin = z(PIN_BYTES)
        self.frames = self.pin.data_ptr() + LEAD
        self.items = z(MAX_FRAMES * 4 * 8)      # points (4 per frame) / quads (1 per frame, 32 bytes) / saddles (8 per frame)
        self.out_a = z(MAX_FRAMES * 36 + 4096)  # caller-owned results: tags / saddle records / refined points / quads
        self.out_b = z((MAX_FRAMES + 1) * 16)   # ... frame table / counts / statuses
        self.out_c = z((MAX_FRAMES + 1) * 16)   # ... statuses / bits
        self.out_d = z(MAX_FRAMES * 8)          # ... n_quads
        self.planes = z(MAX_FRAMES * 16 + (1 << 22))  # agx_planes_enqueue's blur planes
        self.host = np.zeros(PIN_BYTES, np.uint8)            # host images (untouched pages cost nothing)
        self.host_out = np.zeros(1 << 24, np.uint8)          # host results
        self.host_items = np.zeros(64, np.float32)
        torch.cuda.synchronize()

    def close(self):
        self.group.close()
        self.det.close()

    def last_error(self, h=None):
        return self.lib.agx_last_error(h or self.h).decode()

    # ---- the six enqueues + the group's, on frames (ptr, n, w, h, row stride, frame stride, format) -----------------------
    def enqueue(self, kind, f, to=False, image=0, h=None):
        l, h = self.lib, h or self.h
        p = C.c_void_p(f[0])
        a, b, c, d = (t.data_ptr() for t in (self.out_a, self.out_b, self.out_c, self.out_d))
        items = self.items.data_ptr()
        if kind == "saddles":
            if to:
                return l.agx_saddles_batch_enqueue_to(h, p, *f[1:], a, 4096, b)
            return l.agx_saddles_batch_enqueue(h, p, *f[1:])
        if kind == "detect":
            if to:
                return l.agx_detect_batch_enqueue_to(h, p, *f[1:], a, 1, b, c)
            return l.agx_detect_batch_enqueue(h, p, *f[1:], 1)
        if kind == "refine":
            return l.agx_refine_points_enqueue(h, p, *f[1:], image, items, 4, None, a if to else None, b if to else None)
        if kind == "decode":
            return l.agx_decode_quads_enqueue(h, p, *f[1:], items, 8, 1, None, None, a if to else None, b if to else None,
                                              c if to else None)
        if kind == "find":  # no frames: 8 saddles per frame, f[1] frames
            return l.agx_find_boards_enqueue(h, items, 20, f[1], 8, None, None, None, 8, a if to else None, None,
                                             d if to else None, c if to else None)
        if kind == "planes":
            return l.agx_planes_enqueue(h, p, *f[1:], 1.5, self.planes.data_ptr(), None, max(f[2], 0) * 4, max(f[2], 0) * max(f[3], 0) * 4)
        if kind == "group":
            ptrs = (C.c_void_p * 1)(f[0])
            return l.agx_group_detect_enqueue(self.g, ptrs, *f[1:], 1, 1)
        raise KeyError(kind)

    def group_fetch(self):
        o = self.host_out.ctypes.data
        return self.lib.agx_group_detect_fetch(self.g, o, o + (1 << 23), o + (1 << 23) + (1 << 19), 1)

    # ---- the five fetches + agx_debug_fetch, with outputs (null=True: without) ------------------------------------------
    def fetch(self, which, null=False, h=None):
        l, h = self.lib, h or self.h
        o = self.host_out.ctypes.data
        q = [None] * 4 if null else [o, o + (1 << 22), o + (2 << 22), o + (3 << 22)]
        if which == "saddles":
            return l.agx_saddles_batch_fetch(h, q[0], 64, q[1], q[2])
        if which == "detect":
            return l.agx_detect_batch_fetch(h, q[0], q[1], q[2], 1)
        if which == "refine":
            return l.agx_refine_points_fetch(h, q[0], q[1])
        if which == "decode":
            return l.agx_decode_quads_fetch(h, q[0], q[1], q[2])
        if which == "find":
            return l.agx_find_boards_fetch(h, q[0], None, q[1], q[2], 1)
        if which == "debug":
            n = C.c_size_t()
            return l.agx_debug_fetch(h, 0, DBG_MIN, o, 64, C.byref(n))
        raise KeyError(which)

    # ---- the host-image entry points, on one image (ptr, w, h, row stride, format) ----------------------------------------
    def host_call(self, name, f):
        l, h = self.lib, self.h
        p, (w, hh, rs, fmt) = C.c_void_p(f[0]), f[1:]
        o, it, n = self.host_out.ctypes.data, self.host_items.ctypes.data, C.c_uint32()
        if name == "agx_refined_saddle_points":
            return l.agx_refined_saddle_points(h, p, w, hh, rs, fmt, o, 256, C.byref(n))
        if name == "agx_detect":
            return l.agx_detect(h, p, w, hh, rs, fmt, o, 16, C.byref(n))
        if name == "agx_rochade_refine":
            return l.agx_rochade_refine(h, p, w, hh, rs, fmt, 0, it, 4, o, o + 4096, C.byref(n))
        if name == "agx_decode_quads":
            return l.agx_decode_quads(h, p, w, hh, rs, fmt, it, 1, o, o + 4096, o + 8192, C.byref(n))
        if name == "agx_gaussian_blur_f32":
            return l.agx_gaussian_blur_f32(h, p, w, hh, rs, fmt, 1.5, o)
        if name == "agx_hessian_response":
            return l.agx_hessian_response(h, p, w, hh, rs, fmt, o)
        raise KeyError(name)
