"""Frames, rows, output planes and internal per-frame arrays at byte offsets of 2^31, 2^32 and more.

Every kernel computes base + frame * frame_stride + row * row_stride; the ABI lets a row stride be 0x7fffffff, a frame stride
any size_t and a batch 65535 frames.  Here the products really are that large: frame strides of 2^31 + 4096 (frame 1 past 2^31,
frame 2 past 2^32), row strides of 2^25 (rows from 128 on past 2^32; H * row_stride >= 2^31 takes the blur kernel's plain
64-bit form instead of its 32-bit buffer offsets), 2^28 points per frame, and a batch of 1100 frames of 1280 x 800 whose blur
planes end past 2^32 bytes.  The yardsticks are the ones the rest of the suite uses (tests/util.check_frame, check_saddles and
check_tags against the oracle; the f64 point reference of tests/test_gpu_refine_points.py; the host decode and the yardstick
of tests/test_decode_quads_cpu.py; the oracle's planes): bit equality, ANGLE_TOL_DEG for theta and phi, nothing new.

That each test can fail is shown on the host before anything runs (can_fail): every frame or row that is compared lies at
least 2^31 (2^32) bytes behind the pointer handed over, and the bytes a 32-bit product would reach instead -- the offset modulo
2^32, and the offset sign-extended from 32 bits where that is inside the allocation -- differ from the true ones.

Memory: a test reads torch.cuda.mem_get_info() first and skips unless what it needs + 8 GiB is free; none holds more than 96 GiB."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import test_decode_quads_cpu as cases
from tests.util import bits_equal, check_frame, check_saddles, check_tags, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
L8, L16, RGB8, LF32, BGRA8, RGB8P, RGBA16 = 0, 1, 2, 3, 7, 8, 11
FORMAT = {"L8": L8, "L16": L16, "RGB8": RGB8, "LF32": LF32, "BGRA8": BGRA8, "RGB8P": RGB8P, "RGBA16": RGBA16}
BLURRED, PLANE = 0, 1
GIB = 1 << 30
W, H = 320, 200                  # the frame size of tests/test_gpu_decode_quads.py, a 6 x 6 board each
SEEDS = (2, 6, 22)               # synth.render_frame indices: the oracle finds 33, 34 and 33 tags and about 170 saddles in them
FRAME_STRIDE = (1 << 31) + 4096  # case 1: frame 1 starts past 2^31, frame 2 past 2^32
LEAD = 1 << 31                   # case 1: the pointer handed over lies this far into the allocation, so that frame 1's offset
                                 # sign-extended from 32 bits (4096 - 2^31) is inside it: a decoy frame is written there
ROW_STRIDE = 1 << 25             # case 2: row 128 starts at 2^32
TOP = 144                        # case 2: rows without a saddle above the rendered frame -- the board's rows, and the seam 8 rows
                                 # above them, all lie past 2^32
H2 = TOP + H
N2 = 2                           # case 2: frames, (H2 * ROW_STRIDE) apart
POOL_BYTES = N2 * H2 * ROW_STRIDE + 4096  # 21.5 GiB: serves both layouts (case 1 needs LEAD + 2 * FRAME_STRIDE + a frame)
SENTINEL = 0x7FC5A5A5            # tests/test_gpu_planes.py's: a NaN with a payload no arithmetic produces
MEM_CAP = 96 * GIB


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def need_memory(need_bytes, what):
    """Skip unless need + 8 GiB of device memory is free (both numbers printed); a test never asks for more than 96 GiB."""
    import torch
    assert need_bytes <= MEM_CAP, (what, need_bytes)
    free, total = torch.cuda.mem_get_info()
    print("%s: needs %.2f GiB, %.2f GiB of %.2f GiB free" % (what, need_bytes / GIB, free / GIB, total / GIB))
    if free < need_bytes + 8 * GIB:
        pytest.skip("%s needs %.2f GiB + 8 GiB, %.2f GiB free" % (what, need_bytes / GIB, free / GIB))


def release():
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def pool():
    """One uninitialised allocation for the strided inputs of cases 1 - 4: only the frames' own rows are ever written."""
    import torch
    need_memory(POOL_BYTES, "input pool")
    p = torch.empty(POOL_BYTES, dtype=torch.uint8, device="cuda")
    yield p
    del p
    release()


@pytest.fixture(scope="module")
def scene():
    """Three distinct 320 x 200 frames with their ground-truth quads, and the same frames under 144 rows without a saddle
    (case 2): each of those rows is one grey level, a different one from row to row and from frame to frame."""
    one = [cases.gt_case("T36H11", s, 1, W, H) for s in SEEDS]
    frames, quads = np.stack([o[0][0] for o in one]), [o[1][0] for o in one]
    assert len({f.tobytes() for f in frames}) == 3
    tall = np.zeros((3, H2, W), np.uint8)
    for f in range(3):
        tall[f, :TOP] = (90 + (np.arange(TOP) + 7 * f) % 61)[:, None]
    tall[:, TOP:] = frames
    return {"grey": frames, "tall": tall, "quads": quads}


def as_format(name, grey, oracle, seed):
    """grey [..., H, W] u8 -> (pixels in layout `name` as the library takes them, the native image the oracle is asked about)."""
    from tests.test_gpu_formats import make
    rng = np.random.default_rng(seed)
    if name == "L8":
        return grey, grey
    if name == "LF32":
        plane = np.stack([oracle.luma_f32(g) for g in grey.reshape((-1,) + grey.shape[-2:])]).reshape(grey.shape)
        return plane, plane
    if name == "L16":
        base = make("LA16", grey, rng)[1]
        return base, base
    if name == "RGB8":
        base = make("BGR8", grey, rng)[1]
        return base, base
    px, base, _ = make(name, grey, rng)
    return px, base


def byte_rows(px, name):
    """One frame's pixels as the rows the library reads: [rows, bytes] u8 (the planar layout: 3 H rows)."""
    a = np.ascontiguousarray(px)
    rows = a.shape[0] * a.shape[1] if name == "RGB8P" else a.shape[0]
    return a.reshape(rows, -1).view(np.uint8)


def gather(pool, starts, n):
    """n bytes from each of the byte offsets `starts` of the allocation -> u8 [len(starts), n]."""
    import torch
    idx = np.asarray(starts, np.int64)[:, None] + np.arange(n, dtype=np.int64)[None, :]
    return pool[torch.from_numpy(idx).to(pool.device)].cpu().numpy()


def write_rows(pool, start, row_stride, rows):
    """rows [R, n] u8 through a strided view: row r at byte start + r * row_stride; nothing else is touched."""
    import torch
    view = torch.as_strided(pool, rows.shape, (row_stride, 1), start)
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows)).to(pool.device))


def can_fail(pool, base, offsets, rows, floor, what):
    """The host-side precondition.  offsets[r]: byte offset of rows[r] from the pointer handed to the library, which lies
    `base` bytes into the allocation.  Asserts: every offset is at least `floor`; the rows are where the test says; and the
    bytes at the offset modulo 2^32 and at the offset sign-extended from 32 bits -- wherever those differ from the offset and
    lie inside the allocation -- differ from the true ones, for every row, and at least one of the two was there to look at."""
    offsets = np.asarray(offsets, np.int64)
    n = rows.shape[1]
    assert len(offsets) == len(rows) and (offsets >= floor).all(), (what, int(offsets.min()), floor)
    assert np.array_equal(gather(pool, base + offsets, n), rows), what + ": the rows are not where they should be"
    low = offsets & 0xFFFFFFFF
    looked = np.zeros(len(offsets), bool)
    for kind, wrong in (("modulo 2^32", low), ("sign-extended from 32 bits", low - ((low >> 31) << 32))):
        at = base + wrong
        inside = (wrong != offsets) & (at >= 0) & (at + n <= pool.numel())
        if inside.any():
            same = (gather(pool, at[inside], n) == rows[inside]).all(axis=1)
            assert not same.any(), "%s: the bytes at the offset %s equal the true ones (row %d)" % (what, kind, np.flatnonzero(inside)[same][0])
            looked |= inside
    assert looked.all(), what + ": no wrapped address inside the allocation for row %d" % np.flatnonzero(~looked)[0]


def k1_form(w, h, row_stride, frame_stride, ptr, n_frames):
    """Which form of k_blur_hessian launch_k1 (csrc/chain_kernels.hip) picks for this geometry: 'A4' / 'UF', the buffer-resource
    forms with 32-bit offsets, or '64-bit'."""
    import os
    byte_rows_ = ((row_stride | ptr | (frame_stride if n_frames > 1 else 0)) & 3) != 0
    small = w * h * 4 < (1 << 31) and h * row_stride < (1 << 31)
    if w % 4 == 0 and small and not byte_rows_:
        return "A4"
    if small and w >= 4 and os.environ.get("AGX_K1_UNALIGNED_FAST", "1") != "0":
        return "UF"
    return "64-bit"


def lay_out_frames(pool, name, px, layout):
    """Write the batch px (frame-major) into the pool in layout 'frames' (case 1) or 'rows' (case 2), run the precondition on
    every row that will be compared -> (device pointer, n, row stride, frame stride)."""
    rows = [byte_rows(p, name) for p in px]
    n, (R, rb) = len(rows), rows[0].shape
    if layout == "frames":
        base, rs, fs = LEAD, rb, FRAME_STRIDE
        assert n == 3 and base + 2 * fs + R * rs <= pool.numel()
        write_rows(pool, base + fs - (1 << 32), rs, rows[2])  # the decoy: where frame 1's offset sign-extended from 32 bits points
        for f in range(n):
            write_rows(pool, base + f * fs, rs, rows[f])
        for f, floor in ((1, 1 << 31), (2, 1 << 32)):
            can_fail(pool, base, f * fs + np.arange(R, dtype=np.int64) * rs, rows[f], floor, "%s frame %d" % (name, f))
    else:
        base, rs, fs = 0, ROW_STRIDE, R * ROW_STRIDE
        assert n == N2 and n * fs <= pool.numel() and rb <= rs
        for f in range(n):
            write_rows(pool, f * fs, rs, rows[f])
        # frame 0: the rows from 128 on (every saddle and its support: see tall_reference); frame 1: every row
        for f, first in ((0, (1 << 32) // rs), (1, 0)):
            r = np.arange(first, R, dtype=np.int64)
            can_fail(pool, base, f * fs + r * rs, rows[f][first:], 1 << 32, "%s frame %d rows %d.." % (name, f, first))
    return pool.data_ptr() + base, n, rs, fs


def fetched_status(det, n):
    res, status = det.saddles_batch_fetch()
    assert len(res) == n and (status == 0).all(), status
    return res


FORMS = {}  # what the summary reports: (case, format) -> the form of K1 the geometry selects


# ---- 1. frame strides, chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L8", "L16", "RGB8", "LF32", "BGRA8", "RGB8P", "RGBA16"])
def test_frames_2_and_4_gib_apart_through_the_chain(det, oracle, pool, scene, name):
    """Three frames, frame_stride_bytes = 2^31 + 4096, rows tight: every intermediate product of every frame and the fetched
    lists are the oracle's.  The front-end layouts (BGRA8, RGB8P -- 3 H rows per frame --, RGBA16) go through k_front_luma and
    are held to the native image they must agree with, as in tests/test_gpu_formats.py."""
    px, base = as_format(name, scene["grey"], oracle, 11)
    ptr, n, rs, fs = lay_out_frames(pool, name, px, "frames")
    det.saddles_batch_enqueue_ptr(ptr, n, W, H, rs, fs, FORMAT[name])
    res = fetched_status(det, n)
    if name in ("L8", "L16", "RGB8", "LF32"):
        FORMS[1, name] = k1_form(W, H, rs, fs, ptr, n)
    else:  # the blur kernel reads k_front_luma's tight u8 / u16 plane
        opx = 2 if name == "RGBA16" else 1
        FORMS[1, name] = k1_form(W, H, W * opx, W * H * opx, 0, n)
    assert FORMS[1, name] == "A4"
    for f in range(n):
        ref = check_frame(det, oracle, base[f], f, "%s frame %d at %d" % (name, f, f * fs))
        assert len(ref) >= 30
        check_saddles(res[f], ref, "%s frame %d" % (name, f))


# ---- 2. row strides: the blur kernel's 64-bit form ----------------------------------------------------------------------------
def tall_reference(oracle, img):
    """The oracle's saddles of a case-2 frame: at least 30, all of them -- and the 9 x 9 refinement windows and 7-tap blur
    columns under them -- in rows past 2^32."""
    ref = oracle.refined_saddle_points(img)
    assert len(ref) >= 30 and ref["y"].min() >= (1 << 32) // ROW_STRIDE + 8, (len(ref), ref["y"].min())
    return ref


@pytest.mark.parametrize("name", ["L8", "L16", "RGB8", "LF32", "BGRA8"])
def test_rows_32_mib_apart_take_the_64_bit_form(det, oracle, pool, scene, name):
    """Two frames of 320 x 344 with row_stride_bytes = 2^25: H * row_stride >= 2^31, so launch_k1's `small` is false.  Planes,
    tables and lists are the oracle's, and the records are byte for byte those of the same frames at a tight stride (the
    32-bit-offset forms).  BGRA8: the large stride is k_front_luma's; the blur kernel then reads the tight front-end plane."""
    import torch
    px, base = as_format(name, scene["tall"][:N2], oracle, 12)
    ptr, n, rs, fs = lay_out_frames(pool, name, px, "rows")
    native = name in ("L8", "L16", "RGB8", "LF32")
    FORMS[2, name] = k1_form(W, H2, rs, fs, ptr, n) if native else "A4 (behind k_front_luma)"
    assert not native or FORMS[2, name] == "64-bit"
    det.saddles_batch_enqueue_ptr(ptr, n, W, H2, rs, fs, FORMAT[name])
    res = fetched_status(det, n)
    for f in range(n):
        want = tall_reference(oracle, base[f])
        ref = check_frame(det, oracle, base[f], f, "%s frame %d, rows 2^25 apart" % (name, f))
        check_saddles(res[f], ref, "%s frame %d" % (name, f))
        assert len(ref) == len(want)
    a = np.ascontiguousarray(px)
    tight = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    det.saddles_batch_enqueue(tight, format=FORMAT[name] if name == "BGRA8" else None)
    res_tight = fetched_status(det, n)
    assert k1_form(W, H2, tight.stride(1) * tight.element_size(), tight.stride(0) * tight.element_size(), tight.data_ptr(), n) == "A4"
    for f in range(n):
        assert res[f].tobytes() == res_tight[f].tobytes(), "%s frame %d: the 64-bit form and the 32-bit form differ" % (name, f)


def test_a_row_stride_of_2_to_the_31_is_refused(det):
    """row_stride_bytes = 0x80000000 is AGX_ERR_ARG at every entry point that takes the row stride of frames in device memory
    (the entry points for host images stage them through hipMemcpy2D with a size_t pitch and have no such limit) -- and so is
    an out_row_stride_bytes of 0x80000000 at agx_planes_enqueue, which k_hessian_response would read as an int.  Nothing is
    launched: the arguments are refused before any of the memory is looked at."""
    import torch
    import aprilgrid_rs_amd as A
    lib, h = det._lib, det._h
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p, bad = buf.data_ptr(), 0x80000000
    w = hh = 32
    det._follow_torch_stream()
    for fmt in (L8, L16, RGB8, LF32, BGRA8):
        assert lib.agx_saddles_batch_enqueue(h, p, 1, w, hh, bad, 0, fmt) == AGX_ERR_ARG, fmt
        assert lib.agx_saddles_batch_enqueue_to(h, p, 1, w, hh, bad, 0, fmt, p, 64, p) == AGX_ERR_ARG, fmt
        assert lib.agx_refine_points_enqueue(h, p, 1, w, hh, bad, 0, fmt, BLURRED, p, 4, None, None, None) == AGX_ERR_ARG, fmt
        assert lib.agx_planes_enqueue(h, p, 1, w, hh, bad, 0, fmt, 1.5, p, None, 4 * w, 4 * w * hh) == AGX_ERR_ARG, fmt
        if fmt != LF32:
            assert lib.agx_detect_batch_enqueue(h, p, 1, w, hh, bad, 0, fmt, 16) == AGX_ERR_ARG, fmt
            assert lib.agx_detect_batch_enqueue_to(h, p, 1, w, hh, bad, 0, fmt, p, 16, p, p) == AGX_ERR_ARG, fmt
            assert lib.agx_decode_quads_enqueue(h, p, 1, w, hh, bad, 0, fmt, p, 8, 4, None, None, None, None, None) == AGX_ERR_ARG, fmt
    assert lib.agx_refine_points_enqueue(h, p, 1, w, hh, bad, 0, LF32, PLANE, p, 4, None, None, None) == AGX_ERR_ARG
    # the output planes' row stride: blur + response (the response kernel reads the blur plane back), and blur alone
    assert lib.agx_planes_enqueue(h, p, 1, w, hh, w, 0, L8, 1.5, p, p + 4 * w * hh, bad, bad * hh) == AGX_ERR_ARG
    assert lib.agx_planes_enqueue(h, p, 1, w, hh, w, 0, L8, 1.5, p, None, 0x100000000, 0x100000000 * hh) == AGX_ERR_ARG
    g = A.DetectorGroup("t36h11", [0], transport="peer")
    try:
        ptrs = (C.c_void_p * 1)(p)
        assert lib.agx_group_saddles_enqueue(g._g, ptrs, 1, w, hh, bad, 0, L8, 0) == AGX_ERR_ARG
        assert lib.agx_group_detect_enqueue(g._g, ptrs, 1, w, hh, bad, 0, L8, 16, 0) == AGX_ERR_ARG
    finally:
        g.close()
    for fetch in (det.saddles_batch_fetch, det.detect_batch_fetch, det.refine_points_fetch, det.decode_quads_fetch):
        det._batch = det._detect = det._refine = det._decode = None
        with pytest.raises(A.AgxError) as e:  # (none of the refused calls left a batch behind)
            fetch()
        assert e.value.status == AGX_ERR_STATE


# ---- 3. device-resident detect, device tail and host tail -------------------------------------------------------------------
@pytest.mark.parametrize("device_tail", [1, 0])
@pytest.mark.parametrize("layout", ["frames", "rows"])
@pytest.mark.parametrize("name", ["L8", "L16", "RGB8"])
def test_detect_on_the_same_inputs(oracle, pool, scene, name, layout, device_tail):
    """agx_detect_batch_enqueue / _fetch on the inputs of cases 1 and 2: the oracle's tags, bit for bit.  L8 frames are their
    own to_luma8 -- the tail and the decode read them at luma_row_stride * y past 2^32 (device tail), the fetch copies them
    down row by row (host tail) --; L16 / RGB8 go through k_luma8 with these strides."""
    import aprilgrid_rs_amd as A
    grey = scene["grey"] if layout == "frames" else scene["tall"][:N2]
    h = H if layout == "frames" else H2
    px, base = as_format(name, grey, oracle, 13)
    d = A.TagDetector("t36h11", None, device=0)
    try:
        try:
            d.set_option("device_tail", device_tail)
        except A.AgxError as e:
            if device_tail == 1 and e.status == AGX_ERR_STATE:
                pytest.skip("device tail refused on this host (AGX_ERR_STATE)")
            raise
        ptr, n, rs, fs = lay_out_frames(pool, name, px, layout)
        d.detect_batch_enqueue_ptr(ptr, n, W, h, rs, fs, FORMAT[name], cap=128)
        got = d.detect_batch_fetch(n_threads=2)
        if device_tail:
            assert d.get_option("last_device_tail_frames") == n
        found = 0
        for f in range(n):
            ref = oracle.detect(base[f])
            check_tags(got[f], ref, "%s %s device_tail %d frame %d" % (name, layout, device_tail, f))
            found += len(ref)
        assert found >= 30 * n, found
    finally:
        d.close()


# ---- 4. caller-given points, quads and planes ---------------------------------------------------------------------------------
def jittered_corners(scene, f, dy=0):
    from tests.test_gpu_refine_points import gt_corners
    synth = synth_module()
    _, gt = synth.render_frame(SEEDS[f], W, H)
    g = gt_corners(gt, W, H)
    rng = np.random.default_rng(40 + f)
    pts = (g + rng.uniform(-1, 1, g.shape)).astype(np.float32)[:64]
    assert len(pts) == 64
    pts[:, 1] += dy
    return pts


@pytest.mark.parametrize("layout", ["frames", "rows"])
@pytest.mark.parametrize("image", ["plane", "blurred"])
def test_refine_points_on_strided_images(det, oracle, pool, scene, image, layout):
    """agx_refine_points_enqueue on an LF32 plane (AGX_REFINE_PLANE: the oracle's blur, read by k_refine_points with these
    strides) and on L8 frames (AGX_REFINE_BLURRED): the f64 reference of tests/test_gpu_refine_points.py, point by point."""
    import torch
    from tests.test_gpu_refine_points import REFINED, check_points
    grey = scene["grey"] if layout == "frames" else scene["tall"][:N2]
    h, dy = (H, 0) if layout == "frames" else (H2, TOP)
    blur = np.stack([oracle.gaussian_blur_f32(oracle.luma_f32(g)) for g in grey])
    name, px = ("LF32", blur) if image == "plane" else ("L8", grey)
    ptr, n, rs, fs = lay_out_frames(pool, name, px, layout)
    pts = np.stack([jittered_corners(scene, f, dy) for f in range(n)])
    d_pts = torch.from_numpy(pts).cuda()
    det._follow_torch_stream()
    det._check(det._lib.agx_refine_points_enqueue(det._h, ptr, n, W, h, rs, fs, FORMAT[name], PLANE if image == "plane" else BLURRED,
                                                  d_pts.data_ptr(), 64, None, None, None))
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    rec = np.zeros((n, 64), SADDLE_DTYPE)
    st = np.full((n, 64), 0xFFFFFFFF, np.uint32)
    det._check(det._lib.agx_refine_points_fetch(det._h, rec.ctypes.data, st.ctypes.data))
    for f in range(n):
        acc = check_points(oracle, blur[f], pts[f], rec[f], st[f], "%s %s frame %d" % (image, layout, f))
        assert acc.sum() >= 16 and (st[f] == REFINED).sum() == acc.sum(), acc.sum()


@pytest.mark.parametrize("layout", ["frames", "rows"])
def test_decode_quads_on_strided_frames(det, pool, scene, layout):
    """agx_decode_quads_enqueue on L8 frames with these strides (k_decode_quads reads luma_row_stride * y past 2^32): the
    host's decode on the contiguous frame, every slot and field, and the yardstick of tests/test_decode_quads_cpu.py."""
    import torch
    from tests.test_gpu_decode_quads import DECODED, TAG_DTYPE, same, tail
    grey = scene["grey"] if layout == "frames" else scene["tall"][:N2]
    h, dy = (H, 0) if layout == "frames" else (H2, TOP)
    n = len(grey)
    q = min(len(scene["quads"][f]) for f in range(n))
    quads = np.stack([scene["quads"][f][:q] for f in range(n)]).astype(np.float32).copy()
    quads[:, :, 1::2] += dy
    ptr, n, rs, fs = lay_out_frames(pool, "L8", grey, layout)
    d_quads = torch.from_numpy(quads).cuda()
    det._follow_torch_stream()
    det._check(det._lib.agx_decode_quads_enqueue(det._h, ptr, n, W, h, rs, fs, L8, d_quads.data_ptr(), 8, q, None, None, None, None, None))
    tags, st, bits = np.zeros((n, q), TAG_DTYPE), np.zeros((n, q), np.uint32), np.zeros((n, q), np.uint64)
    det._check(det._lib.agx_decode_quads_fetch(det._h, tags.ctypes.data, st.ctypes.data, bits.ctypes.data))
    for f in range(n):
        got = (tags[f], st[f], bits[f])
        same(got, tail("t36h11", grey[f], quads[f]), "%s frame %d" % (layout, f))
        cases.check_against_yardstick(got, cases.yardstick_many(grey[f], quads[f], "T36H11"), "%s frame %d" % (layout, f))
    assert (st == DECODED).sum() >= st.size // 2, np.bincount(st.reshape(-1))


@pytest.mark.parametrize("layout", ["frames", "rows"])
def test_planes_from_strided_frames(det, oracle, pool, scene, layout):
    """agx_planes_enqueue reading RGB8 frames with these strides (k_gauss_blur and k_hessian_response) into tight planes, at
    sigma 1.5 and at sigma 4 (radius 8): the oracle's planes, bit for bit."""
    import torch
    grey = scene["grey"] if layout == "frames" else scene["tall"][:N2]
    h = H if layout == "frames" else H2
    px, base = as_format("RGB8", grey, oracle, 14)
    ptr, n, rs, fs = lay_out_frames(pool, "RGB8", px, layout)
    det._follow_torch_stream()
    for sigma in (1.5, 4.0):
        blur = torch.full((n, h, W), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        resp = torch.full((n, h, W), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        det._check(det._lib.agx_planes_enqueue(det._h, ptr, n, W, h, rs, fs, RGB8, sigma, blur.data_ptr(), resp.data_ptr(), 4 * W, 4 * W * h))
        torch.cuda.synchronize()
        for f in range(n):
            ref = oracle.gaussian_blur_f32(oracle.luma_f32(base[f]), sigma)
            assert bits_equal(blur[f].cpu().numpy(), ref), "%s sigma %g frame %d: blur" % (layout, sigma, f)
            assert bits_equal(resp[f].cpu().numpy(), oracle.hessian_response(ref)), "%s sigma %g frame %d: response" % (layout, sigma, f)
        # only the response: the hessian kernel reads the strided frames itself
        det._check(det._lib.agx_planes_enqueue(det._h, ptr, n, W, h, rs, fs, RGB8, 0.0, None, resp.data_ptr(), 4 * W, 4 * W * h))
        torch.cuda.synchronize()
        for f in range(n):
            assert bits_equal(resp[f].cpu().numpy(), oracle.hessian_response(oracle.luma_f32(base[f]))), "%s frame %d: response, no blur" % (layout, f)


def test_planes_into_rows_and_frames_past_4_gib(det, oracle, scene):
    """agx_planes_enqueue writing blur and response planes of three frames with out_row_stride_bytes = 2^25 -- rows from 128 on
    start past 2^32 -- and out_frame_stride_bytes = (H + 2) * 2^25, so that frame 1 starts 6.3 GiB and frame 2 12.6 GiB behind
    the pointer; the response shares the allocation, 2048 bytes into every row's gap.  Every row that is to be written and
    one row before and one behind every frame carry a sentinel first: a row whose address wrapped at 2^32 (it would land on one
    of frame 0's first 128 rows) keeps the sentinel where it belongs and fails the comparison.  The guard rows stay as they
    were, and the planes are the oracle's, bit for bit."""
    import torch
    grey = scene["grey"]
    n, rs = 3, ROW_STRIDE
    fs = (H + 2) * rs
    total = n * fs
    need_memory(total, "output planes")
    out = torch.empty(total // 4, dtype=torch.float32, device="cuda")
    frames = torch.from_numpy(grey).cuda()
    try:
        base = rs  # bytes: the blur pointer, one row into the allocation (the sentinel row in front of frame 0)
        resp_off = 2048
        assert 4 * W <= resp_off and resp_off + 4 * W <= rs
        ints = out.view(torch.int32)

        def rows_view(first_byte, rows):
            return torch.as_strided(ints, (rows, W), (rs // 4, 1), first_byte // 4)

        offsets = {}
        for f in range(n):
            for plane_off in (0, resp_off):
                start = base + f * fs + plane_off
                # one row before, the frame's rows, one row behind: all sentinel now; the frame's rows are overwritten
                rows_view(start - rs, H + 2).fill_(SENTINEL)
                offsets[f, plane_off] = start - base + np.arange(H, dtype=np.int64) * rs
        # host-side preconditions: frame 1 past 2^31, frame 2 past 2^32, the last rows of every frame past 2^32 -- and such a
        # row's offset modulo 2^32 is another row inside the allocation
        assert offsets[1, 0][0] >= 1 << 31 and offsets[2, 0][0] >= 1 << 32 and offsets[0, 0][-1] >= 1 << 32
        for f in range(n):
            o = offsets[f, 0]
            past = o >= 1 << 32
            assert past[-1] and (f == 0 or past.all())
            wrapped = base + (o[past] & 0xFFFFFFFF)
            assert (wrapped >= 0).all() and (wrapped + 4 * W <= total).all()
        det._follow_torch_stream()
        t0 = time.perf_counter()
        for sigma in (1.5, 4.0):  # radius 3 and radius 8
            det._check(det._lib.agx_planes_enqueue(det._h, frames.data_ptr(), n, W, H, W, W * H, L8, sigma, out.data_ptr() + base,
                                                   out.data_ptr() + base + resp_off, rs, fs))
            torch.cuda.synchronize()
            for f in range(n):
                ref = oracle.gaussian_blur_f32(oracle.luma_f32(grey[f]), sigma)
                for plane_off, want, what in ((0, ref, "blur"), (resp_off, oracle.hessian_response(ref), "response")):
                    start = base + f * fs + plane_off
                    got = rows_view(start - rs, H + 2).cpu().numpy().view(np.uint32)
                    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "sigma %g frame %d %s: a guard row was written" % (sigma, f, what)
                    assert bits_equal(got[1:-1].view(np.float32), want), "sigma %g frame %d: %s" % (sigma, f, what)
                    rows_view(start, H).fill_(SENTINEL)  # (for the next sigma: a row that is not written again would show)
        print("planes into 2^25-byte rows: %.2f GiB held, offsets up to %d, %.2f s" % (total / GIB, int(offsets[2, resp_off][-1]), time.perf_counter() - t0))
    finally:
        del out, frames
        release()


def test_refine_points_with_2_to_the_28_points_per_frame(det, oracle, scene):
    """points_per_frame = 2^28, two frames, counts 60 and 64: frame 1's points start 2^31 bytes, its records 5 * 2^30 bytes
    and its statuses 2^30 bytes behind the pointers handed over.  The points' pointer lies 2^31 bytes into its allocation,
    so that frame 1's byte offset sign-extended from 32 bits is inside it: other points are written there.  Records and
    statuses are pre-filled with a sentinel: the slots of both counts are the f64 reference's, the slot behind each count and
    the slots where offsets wrapped at 2^32 would land keep the sentinel."""
    import torch
    from tests.test_gpu_refine_points import check_points
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    ppf, n, lead = 1 << 28, 2, 1 << 31
    counts = np.array([60, 64], np.int32)
    need = lead + n * ppf * 8 + n * ppf * 20 + n * ppf * 4
    need_memory(need, "2^28 points per frame")
    grey = scene["grey"][:n]
    blur = [oracle.gaussian_blur_f32(oracle.luma_f32(g)) for g in grey]
    pts = np.stack([jittered_corners(scene, f) for f in range(n)])
    t0 = time.perf_counter()
    d_points = torch.empty((lead + n * ppf * 8) // 4, dtype=torch.float32, device="cuda")
    d_out = torch.empty(n * ppf * 5, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n * ppf, dtype=torch.int32, device="cuda")
    frames = torch.from_numpy(grey).cuda()
    d_counts = torch.from_numpy(counts).cuda()
    try:
        d_out.fill_(0x5A5A5A5A)
        d_st.fill_(0x5A5A5A5A)
        first = lead // 4  # (floats) the pointer handed over
        decoy = np.ascontiguousarray(pts[0][::-1])
        for f in range(n):
            d_points[first + f * ppf * 2: first + f * ppf * 2 + 128] = torch.from_numpy(pts[f].reshape(-1)).cuda()
        d_points[first + ppf * 2 - (1 << 30): first + ppf * 2 - (1 << 30) + 128] = torch.from_numpy(decoy.reshape(-1)).cuda()
        # host-side preconditions
        off_points, off_rec, off_st = ppf * 8, ppf * 20, ppf * 4
        assert off_points >= 1 << 31 and off_rec >= 1 << 32 and off_st >= 1 << 30
        signed = (off_points & 0xFFFFFFFF) - (((off_points & 0xFFFFFFFF) >> 31) << 32)
        assert signed == -(1 << 31) and lead + signed >= 0
        at = d_points[(lead + signed) // 4: (lead + signed) // 4 + 128].cpu().numpy()
        assert not np.array_equal(at, pts[1].reshape(-1)) and np.array_equal(at, decoy.reshape(-1))
        wrapped_rec = (off_rec & 0xFFFFFFFF) // 4  # (words) where a record offset modulo 2^32 lands: inside frame 0's unwritten slots
        assert wrapped_rec == (1 << 30) // 4 and wrapped_rec > 64 * 5
        det._follow_torch_stream()
        det._check(det._lib.agx_refine_points_enqueue(det._h, frames.data_ptr(), n, W, H, W, W * H, L8, BLURRED, d_points.data_ptr() + lead,
                                                      ppf, d_counts.data_ptr(), d_out.data_ptr(), d_st.data_ptr()))
        det._check(det._lib.agx_refine_points_fetch(det._h, None, None))
        for f in range(n):
            c = int(counts[f])
            rec = d_out[f * ppf * 5: f * ppf * 5 + 5 * (c + 1)].cpu().numpy().view(np.uint32)
            st = d_st[f * ppf: f * ppf + c + 1].cpu().numpy().view(np.uint32)
            assert (rec[5 * c:] == 0x5A5A5A5A).all() and st[c] == 0x5A5A5A5A, "frame %d: the slot behind the count was written" % f
            acc = check_points(oracle, blur[f], pts[f][:c], rec[:5 * c].view(SADDLE_DTYPE), st[:c], "2^28 points per frame, frame %d" % f)
            assert acc.sum() >= 16
        assert (d_out[wrapped_rec: wrapped_rec + 5 * 64].cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all()
        assert (d_st[64: 64 + 4096].cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all()
        print("2^28 points per frame: %.2f GiB held, %.2f s" % (need / GIB, time.perf_counter() - t0))
    finally:
        del d_points, d_out, d_st, frames, d_counts
        release()


# ---- 5. internal arrays past 4 GiB --------------------------------------------------------------------------------------------
class CachedOracle:
    """The oracle's answers for the frames of case 5, computed once on several threads (ctypes releases the GIL) and handed to
    tests/util.check_frame in place of a second, serial evaluation."""

    def __init__(self, O, images, threads=16):
        from concurrent.futures import ThreadPoolExecutor
        O.lib()
        with ThreadPoolExecutor(threads) as ex:
            answers = list(ex.map(lambda im: O.refined_saddle_points(im, debug=True), images))
        self.answers = {im.tobytes(): a for im, a in zip(images, answers)}

    def refined_saddle_points(self, img, params=None, debug=False):
        ref, d = self.answers[np.ascontiguousarray(img).tobytes()]
        return (ref, d) if debug else ref


def test_a_batch_whose_blur_planes_end_past_4_gib(oracle):
    """1100 frames of 1280 x 800 in one agx_saddles_batch_enqueue: the blur-plane array is 4.2 GiB, frame 1049's plane is the
    first to start past 2^32 bytes.  The batch is 32 rendered frames, frame i = frame i % 32 shifted by 3 * (i // 32) columns:
    frame i and the frames a wrapped plane offset would reach (i - 1049, i - 1048) are different images.  Every status is 0;
    frames 0 and 1049 .. 1099 have the oracle's planes, tables and lists -- and once more with store_response, whose response
    array crosses 2^32 as well."""
    import torch
    import aprilgrid_rs_amd as A
    synth = synth_module()
    n, w, h, n_base = 1100, 1280, 800, 32
    plane_bytes = w * h * 4
    first_past = -(-(1 << 32) // plane_bytes)
    assert first_past == 1049 and (n - 1) * plane_bytes >= 1 << 32
    need_memory(56 * GIB, "1100 frames of 1280 x 800")  # (the workspace is measured below: the estimate is 31 MB per frame + the response planes)
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    base, _ = synth.render_batch(500, n_base, w, h, device="cuda")
    frames = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    for i in range(n):
        frames[i] = torch.roll(base[i % n_base], 3 * (i // n_base), dims=1)
    del base
    checked = [0] + list(range(first_past, n))
    # host-side precondition: the plane offset of every checked frame but frame 0 is past 2^32, and the pixels at that offset
    # modulo 2^32 (an offset into the planes of frames i - 1049 and i - 1048) are not this frame's
    flat = frames.view(-1)
    for i in checked[1:]:
        off = i * plane_bytes
        assert off >= 1 << 32
        px = (off & 0xFFFFFFFF) // 4
        assert px // (w * h) in (i - first_past, i - first_past + 1)
        assert not torch.equal(flat[px: px + w * h], frames[i].view(-1)), i
    host = {i: frames[i].cpu().numpy() for i in checked}
    assert len({a.tobytes() for a in host.values()}) == len(checked)
    cached = CachedOracle(oracle, [host[i] for i in checked])
    assert k1_form(w, h, w, w * h, frames.data_ptr(), n) == "A4"
    FORMS[5, "L8"] = "A4"
    t_setup = time.perf_counter() - t0
    d = A.TagDetector("t36h11", None, device=0)
    try:
        for store in (0, 1):
            t1 = time.perf_counter()
            d.set_option("store_response", store)
            d.saddles_batch_enqueue(frames)
            res, status = d.saddles_batch_fetch()
            t_batch = time.perf_counter() - t1
            held = free0 - torch.cuda.mem_get_info()[0]
            assert held <= MEM_CAP, held
            assert (status == 0).all(), np.flatnonzero(status)
            for i in checked:
                ref = check_frame(d, cached, host[i], i, "frame %d of %d, store_response %d" % (i, n, store))
                check_saddles(res[i], ref, "frame %d" % i)
                assert len(ref) >= 30
            print("1100 x 1280 x 800, store_response %d: %.2f GiB of device memory held (frames + workspace), batch %.2f s, "
                  "checks %.2f s, set-up %.2f s" % (store, held / GIB, t_batch, time.perf_counter() - t1 - t_batch, t_setup))
    finally:
        d.close()
        del frames, flat
        release()
