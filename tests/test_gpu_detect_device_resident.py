"""agx_detect_batch_enqueue / _enqueue_to / agx_detect_batch_fetch: detect (reference src/detector.rs:505-540) over a batch that
exists only in device memory, stream-ordered, without blocking until the fetch.

The yardstick is agx_detect_batch on the same pixels (host frames plus their device copy): same call status, per-frame statuses,
counts and tag bytes, with the device tail, with the host tail, for the frames the kernel hands back, in every format, into host
arrays and into the caller's device arrays."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_CAPACITY, AGX_ERR_STATE = 0, -1, -2, -3, -7
SENTINEL = -0x21524111  # 0xDEADBEEF as int32


def _detector(device_tail=None):
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    if device_tail is not None:
        try:
            d.set_option("device_tail", device_tail)
        except A.AgxError as e:  # this process's atan2f is not the routine the kernel restates: the device tail is refused
            d.close()
            if device_tail == 1 and e.status == AGX_ERR_STATE:
                pytest.skip("device tail refused on this host (AGX_ERR_STATE)")
            raise
    return d


@pytest.fixture(scope="module")
def bench():
    """configs[1]'s 256 frames (1280 x 800 L8, one board each) on the device, and their host copy."""
    synth = synth_module()
    fr, _ = synth.render_batch(0, 256, 1280, 800, device="cuda")
    return fr, fr.cpu().numpy()


@pytest.fixture(scope="module")
def det():
    d = _detector()
    yield d
    d.close()


@pytest.fixture
def tail_det():
    d = _detector(device_tail=1)
    yield d
    d.close()


def assert_same(ref, got, what):
    rc, out, cnt, st = ref
    rc2, out2, cnt2, st2 = got
    assert rc == rc2, (what, rc, rc2)
    assert np.array_equal(st, st2), (what, np.nonzero(st != st2))
    assert np.array_equal(cnt, cnt2), (what, np.nonzero(cnt != cnt2))
    for f in range(len(cnt)):
        if st[f] == AGX_OK:
            assert out[f, : cnt[f]].tobytes() == out2[f, : cnt2[f]].tobytes(), "%s: frame %d" % (what, f)


def device_as_host(res):
    """(rc, tags, counts, status) device tensors -> the host form of detect_batch_raw."""
    import aprilgrid_rs_amd as A
    rc, tags, counts, status = res
    n, cap = tags.shape[:2]
    out = np.ascontiguousarray(tags.cpu().numpy()).view(A.TagDetector.TAG_DTYPE).reshape(n, cap)
    return rc, out, counts.cpu().numpy().astype(np.uint32), status.cpu().numpy()


def device_out(n, cap):
    import torch
    return (torch.full((n, cap, 9), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"))


def both_forms(d, frames, cap, what, ref, n_threads=0):
    """The host-array form and the device-array form of the new pair, each against `ref`; -> the device tensors."""
    d.detect_batch_enqueue(frames, cap=cap)
    assert_same(ref, d.detect_batch_fetch_raw(n_threads), what + " (host arrays)")
    out = device_out(len(frames), cap)
    d.detect_batch_enqueue(frames, cap=cap, out=out)
    got = d.detect_batch_fetch_raw(n_threads)
    assert got[1] is out[0]
    assert_same(ref, device_as_host(got), what + " (device arrays)")
    return out


def test_the_benchmarks_frames(det, bench):
    """256 frames of 1280 x 800 that exist on the device only: the tags of agx_detect_batch on the same pixels, bit for bit,
    through both forms; detect_batch_device and split_device_tags say the same."""
    fr, host = bench
    ref = det.detect_batch_raw(host, n_threads=0, cap=128, device_frames=fr)
    assert ref[0] == AGX_OK and ref[2].mean() > 30
    tags, counts, status = both_forms(det, fr, 128, "bench frames", ref)
    got = det.detect_batch_device(fr, cap=128)
    want = det.detect_batch(host, cap=128, device_frames=fr)
    assert len(got) == len(want) == 256
    for i in range(0, 256, 17):
        assert sorted(got[i]) == sorted(want[i]) and all(np.array_equal(got[i][k], want[i][k]) for k in want[i]), i
    ids, corners = det.split_device_tags(tags)
    assert tuple(corners.shape) == (256, 128, 4, 2) and str(corners.dtype) == "torch.float32"
    n0 = int(counts[0])
    assert [int(v) for v in ids[0, :n0].cpu()] == [int(t["id"]) for t in ref[1][0, :n0]]
    assert np.array_equal(corners[0, :n0].cpu().numpy().reshape(n0, 8).view(np.uint32), ref[1][0, :n0]["xy"].view(np.uint32))


@pytest.mark.parametrize("fmt", ["L16", "RGB8"])
def test_l16_and_rgb8_frames(det, fmt):
    """The k_luma8 path: the decode reads the device's to_luma8 planes."""
    synth = synth_module()
    fr, _ = synth.render_batch(300, 40, 320, 240, device="cuda", fmt=fmt)
    host = fr.cpu().numpy()
    if fmt == "L16":
        host = host.view(np.uint16)
    ref = det.detect_batch_raw(host, n_threads=2, cap=64, device_frames=fr)
    assert ref[0] == AGX_OK and ref[2].sum() > 0
    both_forms(det, fr, 64, fmt, ref, n_threads=2)


@pytest.mark.parametrize("fmt", ["L8", "L16"])
def test_a_raw_pointer_with_padded_rows(det, fmt):
    """agx_detect_batch_enqueue on a view cut out of a larger allocation: rows 80 bytes longer than the frame's, 3 rows of
    padding between frames."""
    import torch
    synth = synth_module()
    fr, _ = synth.render_batch(700, 12, 320, 240, device="cuda", fmt=fmt)
    host = fr.cpu().numpy()
    if fmt == "L16":
        host = host.view(np.uint16)
    n, h, w = fr.shape
    bpp = fr.element_size()
    pad = torch.zeros((n, h + 3, w * bpp + 80), dtype=torch.uint8, device="cuda")
    pad[:, :h, : w * bpp] = fr.contiguous().view(torch.uint8).reshape(n, h, w * bpp)
    ref = det.detect_batch_raw(host, n_threads=2, cap=64)
    assert ref[0] == AGX_OK and ref[2].sum() > 0
    code = {"L8": 0, "L16": 1}[fmt]
    rs, fs = w * bpp + 80, (w * bpp + 80) * (h + 3)
    det.detect_batch_enqueue_ptr(pad.data_ptr(), n, w, h, rs, fs, code, cap=64)
    assert_same(ref, det.detect_batch_fetch_raw(2), fmt + " padded rows (host arrays)")
    out = device_out(n, 64)
    det.detect_batch_enqueue_ptr(pad.data_ptr(), n, w, h, rs, fs, code, cap=64, out=out)
    assert_same(ref, device_as_host(det.detect_batch_fetch_raw(2)), fmt + " padded rows (device arrays)")


def test_the_hand_back_path_without_host_frames(tail_det, bench):
    """Option "tail_debug_band" widens the kernel's guard band so that a known share of frames is handed back: their saddle
    lists and u8 luma come from the device (the L8 frames' own rows, the L16 frames' k_luma8 planes), the host tail runs on
    the pool, and the fetch writes their rows, counts and statuses into the device arrays.  Results unchanged."""
    fr, host = bench
    fr, host = fr[:96], host[:96]
    ref = tail_det.detect_batch_raw(host, n_threads=0, cap=128, device_frames=fr)
    tail_det.set_option("tail_debug_band", 50)
    try:
        tail_det.detect_batch_enqueue(fr, cap=128)
        assert_same(ref, tail_det.detect_batch_fetch_raw(0), "wide band (host arrays)")
        assert tail_det.get_option("last_device_tail_frames") == 96
        back = tail_det.get_option("last_device_tail_fallbacks")
        assert back > 0 and tail_det.get_option("last_device_tail_uncertain") > 0
        out = device_out(96, 128)
        tail_det.detect_batch_enqueue(fr, cap=128, out=out)
        assert_same(ref, device_as_host(tail_det.detect_batch_fetch_raw(0)), "wide band (device arrays)")
        assert tail_det.get_option("last_device_tail_fallbacks") == back
        synth = synth_module()
        f16, _ = synth.render_batch(300, 40, 320, 240, device="cuda", fmt="L16")
        ref16 = tail_det.detect_batch_raw(f16.cpu().numpy().view(np.uint16), n_threads=2, cap=64, device_frames=f16)
        both_forms(tail_det, f16, 64, "L16, wide band", ref16, n_threads=2)
        assert tail_det.get_option("last_device_tail_fallbacks") > 0
    finally:
        tail_det.set_option("tail_debug_band", 0)


def test_the_host_tail_for_every_frame(bench):
    """device_tail = 0 (what a host whose libm the device tail refuses gets): the fetch runs the host tail on every frame from
    the compact saddle lists and the luma planes copied down.  Same results; nothing here needs the device tail."""
    d = _detector(device_tail=0)
    try:
        fr, host = bench
        ref = d.detect_batch_raw(host[:64], n_threads=0, cap=128, device_frames=fr[:64])
        both_forms(d, fr[:64], 128, "host tail", ref)
        assert d.get_option("last_device_tail_frames") == 0
        synth = synth_module()
        rgb, _ = synth.render_batch(900, 24, 320, 240, device="cuda", fmt="RGB8")
        ref = d.detect_batch_raw(rgb.cpu().numpy(), n_threads=3, cap=64, device_frames=rgb)
        both_forms(d, rgb, 64, "host tail, RGB8", ref, n_threads=3)
    finally:
        d.close()


@pytest.mark.parametrize("device_tail", [1, 0])
def test_capacity(bench, device_tail):
    """cap = 4 below every board's tags: AGX_ERR_CAPACITY per frame with the true count, as agx_detect_batch, and no row
    written for such a frame (the sentinel stays); flat frames keep AGX_OK with no tags.  A frame whose chain lists overflow
    (max_saddles 40) reads AGX_ERR_CAPACITY with count 0."""
    import torch
    d = _detector(device_tail=device_tail)
    try:
        fr, host = bench
        flat = torch.full((2,) + tuple(fr.shape[1:]), 128, dtype=torch.uint8, device="cuda")
        frames = torch.cat([fr[:30], flat]).contiguous()
        ref = d.detect_batch_raw(frames.cpu().numpy(), n_threads=0, cap=4, device_frames=frames)
        assert ref[0] == AGX_ERR_CAPACITY
        assert (ref[3][:30] == AGX_ERR_CAPACITY).all() and (ref[2][:30] > 4).all() and (ref[3][30:] == 0).all()
        tags, counts, status = both_forms(d, frames, 4, "cap 4", ref)
        t = tags.cpu().numpy()
        assert (t[:30] == SENTINEL).all() and (t[30:] == SENTINEL).all()  # no truncated row; no row beyond a count
        d.set_limits(max_saddles=40)
        ref = d.detect_batch_raw(frames.cpu().numpy(), n_threads=0, cap=128, device_frames=frames)
        assert (ref[3][:30] == AGX_ERR_CAPACITY).all() and (ref[2][:30] == 0).all()
        tags, _, _ = both_forms(d, frames, 128, "chain overflow", ref)
        assert (tags.cpu().numpy() == SENTINEL).all()
    finally:
        d.close()


def test_state_errors(bench):
    """One batch in flight per handle, the last one enqueued (the saddle pair's rule); the pairs do not mix; a fetch without a
    batch, a second fetch, a NULL or closed handle and float32 planes are refused."""
    import aprilgrid_rs_amd as A
    d = _detector()
    lib, h = d._lib, d._h
    fr, host = bench
    small = fr[:4]
    counts = np.zeros(4, np.uint32)
    out = np.zeros((4, 64), d.TAG_DTYPE)
    st = np.zeros(4, np.int32)
    saddle_out = np.zeros((4, 4096), A.SADDLE_DTYPE)

    def detect_fetch():
        return lib.agx_detect_batch_fetch(h, out.ctypes.data, counts.ctypes.data, st.ctypes.data, 0)

    def saddles_fetch():
        return lib.agx_saddles_batch_fetch(h, saddle_out.ctypes.data, 4096, counts.ctypes.data, st.ctypes.data)

    try:
        assert detect_fetch() == AGX_ERR_STATE  # nothing enqueued
        with pytest.raises(A.AgxError):
            d.detect_batch_fetch()
        # a saddle batch is not a detect batch, and the refusal leaves it in flight
        d.saddles_batch_enqueue(small)
        assert detect_fetch() == AGX_ERR_STATE
        assert saddles_fetch() == AGX_OK
        # and the reverse; the detect batch survives the refusal and is resolved by one fetch
        ref = d.detect_batch_raw(host[:4], n_threads=2, cap=64, device_frames=small)
        d.detect_batch_enqueue(small, cap=64)
        assert saddles_fetch() == AGX_ERR_STATE
        assert_same(ref, d.detect_batch_fetch_raw(2), "after a refused saddle fetch")
        assert detect_fetch() == AGX_ERR_STATE
        # a later enqueue of either pair replaces the batch in flight
        d.detect_batch_enqueue(small, cap=64)
        d.saddles_batch_enqueue(small)
        assert detect_fetch() == AGX_ERR_STATE
        assert saddles_fetch() == AGX_OK
        ref2 = d.detect_batch_raw(host[4:8], n_threads=2, cap=64, device_frames=fr[4:8])
        d.detect_batch_enqueue(small, cap=64)
        d.detect_batch_enqueue(fr[4:8], cap=64)
        assert_same(ref2, d.detect_batch_fetch_raw(2), "the second of two enqueues")
        # arguments
        assert lib.agx_detect_batch_enqueue(None, small.data_ptr(), 4, 1280, 800, 1280, 1280 * 800, 0, 64) == AGX_ERR_ARG
        assert lib.agx_detect_batch_fetch(None, None, None, None, 0) == AGX_ERR_ARG
        assert lib.agx_detect_batch_enqueue(h, small.data_ptr(), 1, 320, 800, 1280, 1280 * 800, 3, 64) == AGX_ERR_FORMAT
        assert lib.agx_detect_batch_enqueue_to(h, small.data_ptr(), 4, 1280, 800, 1280, 1280 * 800, 0, None, 64, None, None) == AGX_ERR_ARG
        import torch
        with pytest.raises(A.AgxError) as e:
            d.detect_batch_enqueue(torch.zeros((2, 64, 64), dtype=torch.float32, device="cuda"))
        assert e.value.status == AGX_ERR_FORMAT
        assert lib.agx_detect_batch_enqueue(h, small.data_ptr(), 4, 1280, 800, 1280, 1280 * 800, 0, 64) == AGX_OK
        assert lib.agx_detector_sync(h) == AGX_OK
    finally:
        d.close()
    with pytest.raises(A.AgxError) as e:  # a closed handle
        d.detect_batch_enqueue(small, cap=64)
    assert e.value.status == AGX_ERR_ARG


def test_stream_order_behind_a_side_stream(det, bench):
    """The frames are written on a side torch stream behind a long queue of other work; the current stream waits for it and the
    enqueue follows the current stream, with no host synchronisation in between: the tags are the frames' own."""
    import torch
    fr, host = bench
    ref = det.detect_batch_raw(host[:64], n_threads=0, cap=128, device_frames=fr[:64])
    for form in ("host", "device"):
        dst = torch.zeros_like(fr[:64])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            a = torch.randn(4096, 4096, device="cuda")
            for _ in range(12):  # tens of milliseconds of queued work in front of the frames
                a = a @ a
                a = a / a.abs().max()
            dst.copy_(fr[:64])
        torch.cuda.current_stream().wait_stream(side)
        if form == "host":
            det.detect_batch_enqueue(dst, cap=128)
            assert_same(ref, det.detect_batch_fetch_raw(0), "behind a side stream")
        else:
            out = device_out(64, 128)
            det.detect_batch_enqueue(dst, cap=128, out=out)
            assert_same(ref, device_as_host(det.detect_batch_fetch_raw(0)), "behind a side stream, device arrays")
        dst.record_stream(side)


_GUARDED = """
import sys, numpy as np, torch, aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth

def check(d, what):
    r = d.debug_fetch(0, "redzones")
    print(what, r, flush=True)
    assert r["damaged_bytes"] == 0, (what, r)
    return r["buffers"]

def run(d, fr, cap, threads=0):
    n = len(fr)
    out = (torch.full((n, cap, 9), -1, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
           torch.zeros(n, dtype=torch.int32, device="cuda"))
    host = fr.cpu().numpy()
    if host.dtype == np.int16:
        host = host.view(np.uint16)
    rc, o, c, s = d.detect_batch_raw(host, n_threads=threads, cap=cap, device_frames=fr)
    d.detect_batch_enqueue(fr, cap=cap, out=out)
    rc2, tags, counts, status = d.detect_batch_fetch_raw(threads)
    assert rc == rc2 and np.array_equal(c.astype(np.int32), counts.cpu().numpy()) and np.array_equal(s, status.cpu().numpy())
    t = tags.cpu().numpy().view(A.TagDetector.TAG_DTYPE).reshape(n, cap)
    for f in range(n):
        if s[f] == 0:
            assert o[f, : c[f]].tobytes() == t[f, : c[f]].tobytes(), f

d = A.TagDetector("t36h11", None, device=0)
try:
    d.set_option("device_tail", 1)
except A.AgxError as e:
    print("DEVICE TAIL REFUSED", e.status, flush=True)
    d.set_option("device_tail", 0)
fr = synth.render_batch(0, 48, 1280, 800, device="cuda")[0]
run(d, fr, 128)
n0 = check(d, "device arrays")
if d.get_option("device_tail") == 1:
    assert n0 >= 26, n0  # the workspace's 21, the code list, the tail's tables in pinned host memory and in device memory
run(d, fr, 4)
check(d, "cap 4")
d.set_option("tail_debug_band", 50)
run(d, fr, 128)
assert d.get_option("last_device_tail_fallbacks") > 0 or d.get_option("device_tail") == 0
check(d, "hand-back")
run(d, synth.render_batch(300, 40, 320, 240, device="cuda", fmt="L16")[0], 64, threads=2)
check(d, "hand-back, L16")
d.set_option("tail_debug_band", 0)
d.set_option("device_tail", 0)
run(d, fr[:20], 128, threads=3)
check(d, "host tail")
d.close()
print("GUARDS INTACT", flush=True)
"""


def test_guard_bytes_around_the_new_buffers():
    """A handle created with guard bytes (AGX_REDZONE_BYTES) in a child process under a time limit: the device tail's device
    tables, the caller's arrays written by k_publish_tags and the fetch, the pinned luma planes of the frames handed back (L8
    and L16), a capacity of 4 and the host tail for every frame leave every guard intact."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AGX_REDZONE_BYTES=str(1 << 16))
    r = subprocess.run([sys.executable, "-c", _GUARDED], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0 and "GUARDS INTACT" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
