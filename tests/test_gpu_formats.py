"""The integer layouts behind the front-end kernel k_front_luma (AGX_LA8, RGBA8, BGR8, BGRA8, planar RGB8, LA16, RGB16,
RGBA16) through every entry point that takes a format.  Each layout is built from a base image (alpha = random bytes,
channels permuted, planes split); the yardstick is the native path on the base -- RGB8 for the 8-bit colour layouts, L8 for
LA8, L16 for LA16, and for RGB16 / RGBA16 the L16 path fed the numpy luma16 plane -- which itself goes through
tests/util.check_frame against the oracle.  Equality is bitwise: no tolerance, no excluded frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT, bits_equal, check_frame, check_tags, load_image, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_STATE = 0, -1, -2, -7
FORMATS = {"LA8": 4, "RGBA8": 5, "BGR8": 6, "BGRA8": 7, "RGB8P": 8, "LA16": 9, "RGB16": 10, "RGBA16": 11}
L8, L16, RGB8 = 0, 1, 2
BPP = {"LA8": 2, "RGBA8": 4, "BGR8": 3, "BGRA8": 4, "RGB8P": 1, "LA16": 4, "RGB16": 6, "RGBA16": 8}
NAMES = sorted(FORMATS)


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


def luma16_of(rgb16):
    v = rgb16.astype(np.uint64)
    n = 2126 * v[..., 0] + 7152 * v[..., 1] + 722 * v[..., 2]
    assert int(n.max()) < 2 ** 32  # u32 arithmetic holds it
    return (n // 10000).astype(np.uint16)


def make(name, grey, rng):
    """grey: [..., H, W] uint8 base image(s).  -> (the pixels in layout `name` as the library takes them: [..., H, W, C], or
    [..., 3, H, W] for the planar layout; the base in the native format the layout must agree with; that format)."""
    g = grey.astype(np.int64)
    alpha8 = rng.integers(0, 256, grey.shape + (1,), dtype=np.uint8)
    if name == "LA8":
        return np.concatenate([grey[..., None], alpha8], -1), grey, L8
    if name in ("RGBA8", "BGR8", "BGRA8", "RGB8P"):
        rgb = np.stack([np.clip(g + d + rng.integers(-2, 3, grey.shape), 0, 255).astype(np.uint8) for d in (-3, 0, 4)], -1)
        if name == "RGBA8":
            px = np.concatenate([rgb, alpha8], -1)
        elif name == "BGR8":
            px = np.ascontiguousarray(rgb[..., ::-1])
        elif name == "BGRA8":
            px = np.concatenate([rgb[..., ::-1], alpha8], -1)
        else:
            px = np.ascontiguousarray(np.moveaxis(rgb, -1, -3))
        return np.ascontiguousarray(px), rgb, RGB8
    wide = np.clip(g * 257 + rng.integers(0, 60, grey.shape), 0, 65535)
    alpha16 = rng.integers(0, 65536, grey.shape + (1,), dtype=np.uint16)
    if name == "LA16":
        l16 = wide.astype(np.uint16)
        return np.concatenate([l16[..., None], alpha16], -1), l16, L16
    rgb16 = np.stack([np.clip(wide + d + rng.integers(-40, 41, grey.shape), 0, 65535).astype(np.uint16) for d in (-300, 0, 500)], -1)
    px = rgb16 if name == "RGB16" else np.concatenate([rgb16, alpha16], -1)
    return np.ascontiguousarray(px), luma16_of(rgb16), L16


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def synth_grey(first, n, w, h):
    synth = synth_module()
    return np.stack([np.asarray(synth.render_frame(first + i, w, h)[0]) for i in range(n)])


def run_batch(det, tensor, fmt=None):
    det.saddles_batch_enqueue(tensor, format=fmt)
    return det.saddles_batch_fetch()


def assert_same_lists(a, b, what):
    (ra, sa), (rb, sb) = a, b
    assert np.array_equal(sa, sb), (what, sa, sb)
    assert len(ra) == len(rb)
    for i in range(len(ra)):
        assert ra[i].tobytes() == rb[i].tobytes(), "%s: frame %d" % (what, i)


# ---- the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_chain_equals_the_native_path(det, oracle, name):
    """A 3-frame device batch and a single host frame (a synthetic board and a photograph): saddle lists and statuses are those
    of the native path on the base, and the base's intermediate products are the oracle's."""
    rng = np.random.default_rng(FORMATS[name])
    grey = synth_grey(21, 3, 640, 480)
    px, base, native_fmt = make(name, grey, rng)
    want = run_batch(det, to_device(base))
    assert (want[1] == 0).all() and all(len(r) > 100 for r in want[0])
    for i in range(3):
        check_frame(det, oracle, base[i], i, "%s base frame %d" % (name, i))
    got = run_batch(det, to_device(px), FORMATS[name])
    assert_same_lists(want, got, name + " device batch")
    # the blur plane too: every pixel of the front-end plane took part
    det.saddles_batch_enqueue(to_device(px), format=FORMATS[name])
    blur = [det.debug_fetch(i, "blur", (480, 640)) for i in range(3)]
    det.saddles_batch_enqueue(to_device(base))
    for i in range(3):
        assert bits_equal(blur[i], det.debug_fetch(i, "blur", (480, 640))), (name, i)
    photo = load_image("EuRoC.png")
    photo = photo if photo.ndim == 2 else photo[..., 0]
    photo = photo if photo.dtype == np.uint8 else (photo >> 8).astype(np.uint8)
    for img in (grey[1], np.ascontiguousarray(photo)):
        p1, b1, _ = make(name, img, rng)
        a = det.refined_saddle_points(b1, as_array=True)
        check_frame(det, oracle, b1, 0, name + " single base")
        b = det.refined_saddle_points(p1, as_array=True, format=FORMATS[name])
        assert a.tobytes() == b.tobytes() and len(a) > 100, name


@pytest.mark.parametrize("name", NAMES)
def test_random_colours_and_the_device_luma_planes(det, name):
    """Fully random channels (a swapped channel moves the luma by up to a whole range): the blur plane of the layout is the native
    path's on the numpy luma plane, and to_luma8 as the device computes it -- for a single frame (the narrowing instantiation of
    the 16-bit layouts) and for a batch with the host tail (k_luma8 on the 16-bit front plane) -- is agx_luma8's, byte for byte."""
    import aprilgrid_rs_amd as A
    rng = np.random.default_rng(400 + FORMATS[name])
    fmt = FORMATS[name]
    for w, h in ((96, 64), (97, 61)):
        ch = BPP[name] // (2 if name.endswith("16") else 1)
        dt = np.uint16 if name.endswith("16") else np.uint8
        px = rng.integers(0, np.iinfo(dt).max + 1, (2, 3, h, w) if name == "RGB8P" else (2, h, w, ch), dtype=dt)
        px.reshape(-1)[:8] = np.iinfo(dt).max  # the largest numerator
        rgb = np.moveaxis(px, 1, -1) if name == "RGB8P" else (px[..., 2::-1] if name.startswith("BGR") else px[..., :3])
        if ch == 2 and name != "RGB8P":
            plane = px[..., 0]
        else:
            v = rgb.astype(np.uint64)
            plane = ((2126 * v[..., 0] + 7152 * v[..., 1] + 722 * v[..., 2]) // 10000).astype(dt)
        plane = np.ascontiguousarray(plane)
        want8 = [A.TagDetector.luma8(px[i], format=fmt) for i in range(2)]
        assert np.array_equal(want8[0], plane[0] if dt == np.uint8 else ((plane[0].astype(np.uint32) + 128) // 257).astype(np.uint8))
        det.saddles_batch_enqueue(to_device(plane))
        det.saddles_batch_fetch(raise_on_overflow=False)
        want_blur = [det.debug_fetch(i, "blur", (h, w)) for i in range(2)]
        det.saddles_batch_enqueue(to_device(px), format=fmt)
        det.saddles_batch_fetch(raise_on_overflow=False)
        for i in range(2):
            assert bits_equal(det.debug_fetch(i, "blur", (h, w)), want_blur[i]), (name, w, h, i)
        det.detect(px[1], format=fmt)
        assert det.debug_fetch(0, "luma8", (h, w)).tobytes() == want8[1].tobytes(), (name, w, h, "single frame")
        d0 = A.TagDetector("t36h11", None, device=0)
        try:
            d0.set_option("device_tail", 0)
            rc, _, _, status = d0.detect_batch_raw(px, n_threads=2, cap=64, format=fmt)
            assert rc == AGX_OK and (status == 0).all()
            assert d0.debug_fetch(0, "luma8", (h, w)).tobytes() == want8[0].tobytes(), (name, w, h, "batch, host tail")
        finally:
            d0.close()


# ---- geometry -------------------------------------------------------------------------------------------------------------
def padded(px, name, pad, offset, frame_pad=0):
    """The batch px ([n, H, W, C] or [n, 3, H, W]) laid out with rows `pad` bytes longer than the pixels, `frame_pad` more bytes
    between frames and the whole `offset` bytes into the allocation, every other byte 0xC3.
    -> (device byte tensor, offset, row stride, frame stride)."""
    import torch
    n = px.shape[0]
    rows = px.reshape(n, -1, px.shape[-1] if name == "RGB8P" else px.shape[-2] * px.shape[-1]).view(np.uint8)
    r, rb = rows.shape[1], rows.shape[2]
    stride = rb + pad
    fs = r * stride + frame_pad
    buf = np.full(offset + n * fs + 64, 0xC3, np.uint8)
    for f in range(n):
        view = buf[offset + f * fs: offset + f * fs + r * stride].reshape(r, stride)
        view[:, :rb] = rows[f]
    return torch.from_numpy(buf).cuda(), offset, stride, fs


GEOMETRY = [  # (width, height, row padding in bytes for 8-bit / 16-bit layouts, base pointer offset in units of the alignment)
    (640, 96, (0, 0), 0), (640, 96, (1, 2), 0), (640, 96, (2, 4), 0), (640, 96, (3, 6), 0), (640, 96, (0, 0), 1),
    (613, 96, (0, 0), 0), (613, 37, (1, 2), 0), (613, 37, (2, 4), 1), (613, 37, (3, 6), 0),
    (2, 2, (0, 0), 0), (2, 9, (1, 2), 1), (9, 2, (3, 6), 0), (2, 96, (2, 4), 0),
]


@pytest.mark.parametrize("name", NAMES)
def test_widths_strides_and_misaligned_bases(det, name):
    """Widths 640, 613 and 2, heights down to 2, rows padded by 1, 2 and 3 bytes (16-bit layouts: 2, 4 and 6 -- an odd stride is
    refused for them, as for AGX_L16), a base pointer 1 byte (16-bit: 2 bytes) into the allocation: lists, statuses and the
    whole blur plane of both frames are the native path's on the tightly packed base."""
    rng = np.random.default_rng(100 + FORMATS[name])
    sixteen = name in ("LA16", "RGB16", "RGBA16")
    full = synth_grey(60, 2, 640, 96)
    for w, h, pads, off in GEOMETRY:
        grey = np.ascontiguousarray(full[:, :h, :w])
        px, base, native_fmt = make(name, grey, rng)
        what = "%s %dx%d pad %s offset %d" % (name, w, h, pads, off)
        want = run_batch(det, to_device(base))
        want_blur = [det.debug_fetch(i, "blur", (h, w)) for i in range(2)]
        buf, offset, stride, fs = padded(px, name, pads[1] if sixteen else pads[0], off * (2 if sixteen else 1), frame_pad=4 if off else 0)
        det.saddles_batch_enqueue_ptr(buf.data_ptr() + offset, 2, w, h, stride, fs, FORMATS[name])
        got = det.saddles_batch_fetch()
        assert_same_lists(want, got, what)
        for i in range(2):
            assert bits_equal(det.debug_fetch(i, "blur", (h, w)), want_blur[i]), (what, i)
    assert len(want_blur) == 2


@pytest.mark.parametrize("name", NAMES)
def test_a_full_size_batch(det, oracle, name):
    """8 frames of 1280 x 800 per layout (the vector path at the benchmark's geometry)."""
    rng = np.random.default_rng(200 + FORMATS[name])
    grey = synth_grey(100, 8, 1280, 800)
    px, base, _ = make(name, grey, rng)
    want = run_batch(det, to_device(base))
    check_frame(det, oracle, base[7], 7, name + " 1280x800 base")
    got = run_batch(det, to_device(px), FORMATS[name])
    assert_same_lists(want, got, name + " 1280x800")
    assert all(len(r) > 100 for r in got[0])


# ---- detect ---------------------------------------------------------------------------------------------------------------
def tags_of(out, counts, status, i):
    assert status[i] == 0, (i, status)
    return {int(t["id"]): t["xy"].reshape(4, 2).copy() for t in out[i, : counts[i]]}


@pytest.mark.parametrize("name", NAMES)
def test_detect_through_every_entry_point(oracle, name):
    """agx_detect, agx_detect_batch (host frames, 2 threads), agx_detect_batch_enqueue / _fetch and agx_detect_batch_enqueue_to
    with the host tail (device_tail 0), the default and the device tail asked for: the oracle's ids and corners, bit for bit,
    at least 30 tags per frame."""
    import torch
    import aprilgrid_rs_amd as A
    rng = np.random.default_rng(300 + FORMATS[name])
    n, cap = 3, 128
    grey = synth_grey(0, n, 640, 400)
    px, base, _ = make(name, grey, rng)
    refs = [oracle.detect(base[i]) for i in range(n)]
    assert all(len(r) >= 30 for r in refs)
    fmt = FORMATS[name]
    dev_px = to_device(px)
    for tail in (None, 0, 1):
        d = A.TagDetector("t36h11", None, device=0)
        try:
            if tail is not None:
                try:
                    d.set_option("device_tail", tail)
                except A.AgxError as e:
                    assert tail == 1 and e.status == AGX_ERR_STATE, e  # refused on this host: that leg is skipped
                    continue
            what = "%s device_tail %s" % (name, tail)
            if tail is None:
                for i in range(n):
                    check_tags(d.detect(px[i], format=fmt), refs[i], what + " agx_detect frame %d" % i)
            rc, out, counts, status = d.detect_batch_raw(px, n_threads=2, cap=cap, format=fmt)
            assert rc == AGX_OK
            for i in range(n):
                check_tags(tags_of(out, counts, status, i), refs[i], what + " agx_detect_batch frame %d" % i)
            d.detect_batch_enqueue(dev_px, cap=cap, format=fmt)
            rc, out, counts, status = d.detect_batch_fetch_raw(2)
            assert rc == AGX_OK
            for i in range(n):
                check_tags(tags_of(out, counts, status, i), refs[i], what + " enqueue / fetch frame %d" % i)
            dev_out = (torch.full((n, cap, 9), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                       torch.full((n,), -1, dtype=torch.int32, device="cuda"))
            d.detect_batch_enqueue(dev_px, cap=cap, out=dev_out, format=fmt)
            rc, tags, cnt, st = d.detect_batch_fetch_raw(2)
            assert rc == AGX_OK
            out = np.ascontiguousarray(tags.cpu().numpy()).view(A.TagDetector.TAG_DTYPE).reshape(n, cap)
            for i in range(n):
                check_tags(tags_of(out, cnt.cpu().numpy(), st.cpu().numpy(), i), refs[i], what + " enqueue_to frame %d" % i)
        finally:
            d.close()


# ---- the Python wrapper ---------------------------------------------------------------------------------------------------
def test_tensor_formats_are_inferred_and_overridden(det):
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
    tf = A.TagDetector._tensor_format
    assert tf(z(2, 8, 12)) == (_ffi.AGX_L8, 1) and tf(z(2, 8, 12, dtype=torch.int16)) == (_ffi.AGX_L16, 2)
    assert tf(z(2, 8, 12, 3)) == (_ffi.AGX_RGB8, 3) and tf(z(2, 8, 12, dtype=torch.float32)) == (_ffi.AGX_LF32, 4)
    assert tf(z(2, 3, 8, 3)) == (_ffi.AGX_RGB8, 3)  # every mapping that existed stays
    assert tf(z(2, 8, 12, 4)) == (_ffi.AGX_RGBA8, 4) and tf(z(2, 8, 12, 2)) == (_ffi.AGX_LA8, 2)
    assert tf(z(2, 3, 8, 12)) == (_ffi.AGX_RGB8P, 1)
    assert tf(z(2, 8, 12, 2, dtype=torch.int16)) == (_ffi.AGX_LA16, 4)
    assert tf(z(2, 8, 12, 3, dtype=torch.int16)) == (_ffi.AGX_RGB16, 6)
    assert tf(z(2, 8, 12, 4, dtype=torch.int16)) == (_ffi.AGX_RGBA16, 8)
    assert tf(z(2, 8, 12, 3), _ffi.AGX_BGR8) == (_ffi.AGX_BGR8, 3) and tf(z(2, 8, 12, 4), _ffi.AGX_BGRA8) == (_ffi.AGX_BGRA8, 4)
    for bad, fmt in ((z(2, 8, 12, 3), _ffi.AGX_BGRA8), (z(2, 8, 12, 5), None), (z(2, 8, 12, 3), 12)):
        with pytest.raises(A.AgxError) as e:
            tf(bad, fmt)
        assert e.value.status == AGX_ERR_FORMAT
    # a channel-first batch is its channel-last form; BGR named by format= is the RGB image
    rng = np.random.default_rng(9)
    grey = synth_grey(5, 2, 320, 240)
    planar, rgb, _ = make("RGB8P", grey, rng)
    chw = to_device(planar)
    assert tuple(chw.shape) == (2, 3, 240, 320)
    want = run_batch(det, chw.permute(0, 2, 3, 1).contiguous())
    assert np.array_equal(chw.permute(0, 2, 3, 1).cpu().numpy(), rgb)
    assert_same_lists(want, run_batch(det, chw), "channel-first")
    assert_same_lists(want, run_batch(det, to_device(rgb[..., ::-1]), _ffi.AGX_BGR8), "BGR by format=")
    assert sum(len(r) for r in want[0]) > 100
    tags = det.detect_batch_device(chw, cap=64)
    want_tags = det.detect_batch_device(chw.permute(0, 2, 3, 1).contiguous(), cap=64)
    for i in range(2):
        check_tags(tags[i], want_tags[i], "channel-first detect frame %d" % i)


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_error_rules_are_unchanged(det):
    import torch
    import aprilgrid_rs_amd as A
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for call in (lambda: det.saddles_batch_enqueue_ptr(p, 1, 32, 32, 256, 8192, 12),
                 lambda: det.saddles_batch_enqueue_ptr(p, 1, 32, 32, 256, 8192, -1),
                 lambda: det.detect_batch_enqueue_ptr(p, 1, 32, 32, 256, 8192, 12),
                 lambda: det.detect_batch_enqueue_ptr(p, 1, 32, 32, 128, 4096, 3),  # AGX_LF32 has no u8 luma to derive
                 lambda: det.detect(np.zeros((32, 32, 4), np.uint8), format=12)):
        with pytest.raises(A.AgxError) as e:
            call()
        assert e.value.status == AGX_ERR_FORMAT
    for name in ("LA16", "RGB16", "RGBA16"):
        row = 32 * BPP[name]
        for args in ((p, 2, 32, 32, row + 1, 32 * (row + 1) + 1), (p + 1, 2, 32, 32, row, 32 * row), (p, 2, 32, 32, row, 32 * row + 1)):
            with pytest.raises(A.AgxError) as e:
                det.saddles_batch_enqueue_ptr(*args, FORMATS[name])
            assert e.value.status == AGX_ERR_ARG, (name, args)
    with pytest.raises(A.AgxError) as e:  # a frame of the planar layout spans three planes
        det.saddles_batch_enqueue_ptr(p, 2, 32, 32, 32, 32 * 32, FORMATS["RGB8P"])
    assert e.value.status == AGX_ERR_ARG
    with pytest.raises(A.AgxError) as e:
        det.saddles_batch_enqueue_ptr(p, 1, 32, 32, 32 * 4 - 1, 8192, FORMATS["RGBA8"])
    assert e.value.status == AGX_ERR_ARG


# ---- memory safety --------------------------------------------------------------------------------------------------------
def test_guard_bytes_stay_intact_at_a_ragged_width():
    """A handle with guard bytes around every buffer, every layout at 613 x 37 (the per-pixel path, rows and frames that end
    off the dword grid) and at 640 x 48 (the vector path): no guard byte is touched, and the front-end plane has joined the
    guarded buffers behind the existing ones."""
    import aprilgrid_rs_amd as A
    os.environ["AGX_REDZONE_BYTES"] = str(1 << 16)
    try:
        d = A.TagDetector("t36h11", None, device=0)
    finally:
        del os.environ["AGX_REDZONE_BYTES"]
    try:
        rng = np.random.default_rng(77)
        full = synth_grey(60, 3, 640, 96)
        run_batch(d, to_device(full))  # every buffer the native formats use exists before the count is taken
        rgb = make("BGR8", full, rng)[1]
        d.detect_batch_device(to_device(rgb), cap=128)
        d.detect(rgb[0])
        before = d.debug_fetch(0, "redzones")
        assert before["buffers"] >= 20 and before["damaged_bytes"] == 0, before
        address = before["buffer0_address"]
        for name in NAMES:
            for w, h in ((613, 37), (640, 48), (2, 2)):
                px, base, _ = make(name, np.ascontiguousarray(full[:, :h, :w]), rng)
                want = run_batch(d, to_device(base))
                assert_same_lists(want, run_batch(d, to_device(px), FORMATS[name]), name)
                d.detect_batch_device(to_device(px), cap=128, format=FORMATS[name])
                d.detect(px[0], format=FORMATS[name])
                r = d.debug_fetch(0, "redzones")
                assert r["damaged_bytes"] == 0, (name, w, h, r)
                assert r["buffers"] > before["buffers"], (name, r, before)
        assert d.debug_fetch(0, "redzones")["buffer0_address"] == address  # buffer 0 is still the blur plane
    finally:
        d.close()


# ---- HIP graph ------------------------------------------------------------------------------------------------------------
def test_an_rgba8_batch_replays_from_a_hip_graph():
    """tools/graph_capture_formats.py: one captured RGBA8 batch replayed twice gives the eager result, which is the native RGB8
    path's (in its own process: a failed capture would leave the stream in an error state)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "graph_capture_formats.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "eager RGBA8 equals native RGB8: True" in r.stdout and r.stdout.count("equals eager: True") == 2, r.stdout[-2000:]
