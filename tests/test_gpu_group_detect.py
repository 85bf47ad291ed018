"""agx_group_detect_enqueue / agx_group_detect_fetch: detect (reference src/detector.rs:505-540) on every rank of a detector
group, the tags gathered to the root as packed slabs (frame table + the frames' tag records back to back: k_pack_tags).

The yardstick in every case is ONE plain TagDetector's detect_batch_raw(host, device_frames=...) over the concatenated frames:
same counts and statuses, rows byte for byte.  Ranks go round-robin over the visible devices, so a one-GPU box runs them all on
device 0 (the peer transport, or tests/stub_rccl behind the RCCL branch)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_CAPACITY, AGX_ERR_STATE = 0, -1, -2, -3, -7
TAG_BYTES = 36


def assert_same(ref, got, what):
    rc, out, cnt, st = ref
    rc2, out2, cnt2, st2 = got
    assert rc == rc2, (what, rc, rc2)
    assert np.array_equal(st, st2), (what, st, st2)
    assert np.array_equal(cnt, cnt2), (what, cnt, cnt2)
    for f in range(len(cnt)):
        if st[f] == AGX_OK:
            assert out[f, : cnt[f]].tobytes() == out2[f, : cnt2[f]].tobytes(), "%s: frame %d" % (what, f)


def _devices(ranks):
    import torch
    n_dev = torch.cuda.device_count()
    return [r % n_dev for r in range(ranks)]


def _sync(devices):
    import torch
    for d in set(devices):
        torch.cuda.synchronize(d)


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _shard(frames, devices):
    """One device tensor [N, ...] -> contiguous per-rank tensors, rank r's on devices[r]."""
    fpr = len(frames) // len(devices)
    assert fpr * len(devices) == len(frames)
    return [frames[r * fpr:(r + 1) * fpr].to("cuda:%d" % devices[r]).contiguous() for r in range(len(devices))]


def _group(devices, transport="peer", device_tail=None):
    """A group whose ranks' detectors all have option device_tail set (None: left alone)."""
    import aprilgrid_rs_amd as A
    grp = A.DetectorGroup("t36h11", devices, transport=transport)
    if device_tail is not None:
        for r in range(len(devices)):
            st = _set(grp, r, "device_tail", device_tail)
            if st != AGX_OK:
                grp.close()
                if device_tail == 1 and st == AGX_ERR_STATE:
                    pytest.skip("device tail refused on this host (AGX_ERR_STATE)")
                raise A.AgxError(st, "set_option device_tail")
    return grp


def _handle(grp, r):
    h = grp._lib.agx_group_detector(grp._g, r)
    assert h
    return C.c_void_p(h)


def _set(grp, r, name, value):
    return grp._lib.agx_detector_set_option(_handle(grp, r), name.encode(), int(value))


def _get(grp, r, name):
    v = C.c_int(0)
    assert grp._lib.agx_detector_get_option(_handle(grp, r), name.encode(), C.byref(v)) == AGX_OK
    return v.value


def _sum(grp, name):
    return sum(_get(grp, r, name) for r in range(len(grp.devices)))


def _last_error(grp):
    return grp._lib.agx_group_last_error(grp._g).decode()


@pytest.fixture(scope="module")
def plain():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def l8(plain):
    """Frames 50 .. 61 of the synthetic sequence, 640 x 400 L8, on device 0, and the plain detector's result for them."""
    fr, _ = synth_module().render_batch(50, 12, 640, 400, device="cuda:0")
    ref = plain.detect_batch_raw(_host(fr), n_threads=0, cap=1024, device_frames=fr)
    assert ref[0] == AGX_OK and (ref[2] >= 30).all()
    return fr, ref


@pytest.fixture(scope="module")
def l16(plain):
    fr, _ = synth_module().render_batch(300, 40, 320, 240, device="cuda:0", fmt="L16")
    ref = plain.detect_batch_raw(_host(fr), n_threads=2, cap=64, device_frames=fr)
    assert ref[0] == AGX_OK and ref[2].sum() > 0
    return fr, ref


def _ref_slice(ref, n):
    rc, out, cnt, st = ref
    return (AGX_OK if (st[:n] == 0).all() else AGX_ERR_CAPACITY), out[:n], cnt[:n], st[:n]


@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_peer_transport(l8, ranks):
    """4 frames per rank through the peer-copy gather, twice (slab reuse): equal to the plain detector; for two ranks also to the
    oracle's detect, ids equal and corners bit for bit."""
    fr, ref = l8
    devices = _devices(ranks)
    grp = _group(devices)
    try:
        frames = _shard(fr[: 4 * ranks], devices)
        _sync(devices)
        for rep in range(2):
            grp.detect_enqueue(frames, cap=1024)
            got = grp.detect_fetch_raw()
            assert_same(_ref_slice(ref, 4 * ranks), got, "%d ranks, run %d" % (ranks, rep))
        if ranks == 2:
            from oracle import oracle as O
            O.lib()
            grp.detect_enqueue(frames, cap=1024)
            res, status = grp.detect_fetch()
            assert (status == 0).all() and len(res) == 8
            host = _host(fr)
            for i in range(8):
                want = O.detect(host[i])
                assert 33 <= len(want) <= 36 and sorted(res[i]) == sorted(want), i
                for k in want:
                    assert np.array_equal(np.asarray(want[k], np.float32).view(np.uint32), res[i][k].view(np.uint32)), (i, k)
    finally:
        grp.close()


_STAND_IN = r"""
import ctypes as C
import os
import numpy as np
import torch
import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth

so = os.environ["AGX_RCCL_LIBRARY"]
ranks, fpr, cap = 3, 3, 1024
fr = synth.render_batch(50, ranks * fpr, 640, 400, device="cuda:0")[0]
plain = A.TagDetector("t36h11", None, device=0)
rc, out, cnt, st = plain.detect_batch_raw(fr.cpu().numpy(), n_threads=0, cap=cap, device_frames=fr)
assert rc == 0 and (cnt >= 30).all()
grp = A.DetectorGroup("t36h11", [0] * ranks, transport="rccl")
frames = [fr[r * fpr:(r + 1) * fpr].contiguous() for r in range(ranks)]
torch.cuda.synchronize(0)
stub = C.CDLL(so)
before = (C.c_int * 8)()
stub.stub_rccl_stats(before)
grp.detect_enqueue(frames, cap=cap, tags_per_frame=64)
rc2, out2, cnt2, st2 = grp.detect_fetch_raw()
after = (C.c_int * 8)()
stub.stub_rccl_stats(after)
assert rc2 == 0 and np.array_equal(st, st2) and np.array_equal(cnt, cnt2), (rc2, list(st2), list(cnt2))
for f in range(ranks * fpr):
    assert out[f, : cnt[f]].tobytes() == out2[f, : cnt2[f]].tobytes(), f
ops = after[1] - before[1]
assert after[4] == 0 and after[0] - before[0] == 1 and ops == after[2] - before[2] and 0 < ops <= 2 * (ranks - 1), list(after)
# the stand-in counts whole KiB per send: at most 1 KiB per send is missing from its sum
moved = (after[3] - before[3] + ops) * 1024
print("moved at most", moved, "bytes in", ops, "sends", flush=True)
assert moved < 2 * fpr * 1024 * 36 / 10, moved
grp.close()
plain.close()
print("STAND-IN OK", flush=True)
"""


def test_rccl_branch_through_the_stand_in(tmp_path):
    """Three ranks on one device through group.cpp's RCCL branch (tests/stub_rccl behind AGX_RCCL_LIBRARY), cap 1024 and 64 tag
    records per frame of slab: results equal to the plain detector's.  The two sending ranks' unpacked rows would be 2 x 3 x 1024
    x 36 bytes; a table of 3 x 16 bytes and a slab of 3 x 64 x 36 bytes per rank is less than a tenth of that (13 920 of 221 184)
    whatever the frames hold.  In a child process, with AGX_RCCL_LIBRARY in the child's environment only: the stand-in must not
    stay mapped in the process the rest of the suite runs in (tests/test_gpu_multi_device.py checks which librccl a group
    bound by reading the process's maps)."""
    so = str(tmp_path / "librccl_stub.so")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "stub_rccl", "stub_rccl.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "AGX_RCCL_LIBRARY" not in os.environ
    env = dict(os.environ, AGX_RCCL_LIBRARY=so)
    r = subprocess.run([sys.executable, "-c", _STAND_IN], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "STAND-IN OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "librccl_stub" not in open("/proc/self/maps").read()


def test_l16_frames_over_two_ranks(l16):
    fr, ref = l16
    devices = _devices(2)
    grp = _group(devices)
    try:
        frames = _shard(fr, devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=64)
        assert_same(ref, grp.detect_fetch_raw(2), "L16")
    finally:
        grp.close()


def test_rgb8_and_bgra8_frames_and_f32_refused(plain):
    """k_luma8 behind the chain (RGB8), the front-end kernel's plane as the luma (BGRA8, built from L8 frames); AGX_LF32 is
    AGX_ERR_FORMAT."""
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    synth = synth_module()
    devices = _devices(2)
    grp = _group(devices)
    try:
        rgb, _ = synth.render_batch(900, 24, 320, 240, device="cuda:0", fmt="RGB8")
        ref = plain.detect_batch_raw(_host(rgb), n_threads=2, cap=64, device_frames=rgb)
        assert ref[0] == AGX_OK and ref[2].sum() > 0
        frames = _shard(rgb, devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=64)
        assert_same(ref, grp.detect_fetch_raw(2), "RGB8")

        grey, _ = synth.render_batch(700, 6, 320, 240, device="cuda:0")
        g = grey.cpu().numpy()
        alpha = np.random.default_rng(7).integers(0, 256, g.shape, dtype=np.uint8)
        bgra = torch.from_numpy(np.ascontiguousarray(np.stack([g, g, g, alpha], -1))).to("cuda:0")
        ref = plain.detect_batch_raw(bgra.cpu().numpy(), n_threads=2, cap=64, device_frames=bgra, format=_ffi.AGX_BGRA8)
        assert ref[0] == AGX_OK and ref[2].sum() > 0
        frames = _shard(bgra, devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=64, format=_ffi.AGX_BGRA8)
        assert_same(ref, grp.detect_fetch_raw(2), "BGRA8")

        f32 = [torch.zeros((2, 240, 320), dtype=torch.float32, device="cuda:%d" % d) for d in devices]
        with pytest.raises(A.AgxError) as e:
            grp.detect_enqueue(f32, cap=64)
        assert e.value.status == AGX_ERR_FORMAT
        ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in f32])
        assert grp._lib.agx_group_detect_enqueue(grp._g, ptrs, 2, 320, 240, 1280, 1280 * 240, _ffi.AGX_LF32, 64, 0) == AGX_ERR_FORMAT
    finally:
        grp.close()


def test_the_hand_back_path(l16):
    """tail_debug_band 50 on every rank: a share of the frames is handed back and resolved by the host tail on its own rank's
    saddle lists and luma; the results are the ones taken with band 0."""
    fr, ref = l16
    devices = _devices(2)
    grp = _group(devices, device_tail=1)
    try:
        for r in range(2):
            assert _set(grp, r, "tail_debug_band", 50) == AGX_OK
        frames = _shard(fr, devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=64)
        assert_same(ref, grp.detect_fetch_raw(2), "wide band")
        assert _sum(grp, "last_device_tail_fallbacks") > 0
        assert _sum(grp, "last_device_tail_frames") == 40
        assert _sum(grp, "last_device_tail_uncertain") <= _sum(grp, "last_device_tail_fallbacks")
    finally:
        for r in range(2):
            _set(grp, r, "tail_debug_band", 0)
        grp.close()


def test_the_host_tail_for_every_frame(l8):
    fr, ref = l8
    devices = _devices(2)
    grp = _group(devices, device_tail=0)
    try:
        frames = _shard(fr[:8], devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=1024)
        assert_same(_ref_slice(ref, 8), grp.detect_fetch_raw(), "host tail")
        assert _sum(grp, "last_device_tail_frames") == 0
    finally:
        grp.close()


def _raw_fetch(grp, n, cap, fill=0xA5):
    """agx_group_detect_fetch into sentinel-filled arrays -> (rc, out as bytes [n, cap * 36], counts, status)."""
    out = np.full((n, cap * TAG_BYTES), fill, np.uint8)
    counts = np.zeros(n, np.uint32)
    status = np.full(n, AGX_ERR_STATE, np.int32)
    rc = grp._lib.agx_group_detect_fetch(grp._g, out.ctypes.data, counts.ctypes.data, status.ctypes.data, 0)
    grp._detect = None
    return rc, out, counts, status


def test_capacity_per_frame(l8, plain):
    """cap_per_frame 16: whole boards (33 .. 36 tags) next to frames cut down to a strip of theirs.  Every frame with more than
    16 tags reports AGX_ERR_CAPACITY with its true count and no row, the others are intact, the call returns -3 -- all as the
    plain detector reports the same pixels with cap 16 -- and nothing beyond a frame's own rows is written."""
    fr, full = l8
    devices = _devices(2)
    grp = _group(devices)
    try:
        batch = fr[:8].clone()
        for i, keep in ((1, 200), (3, 260), (6, 320)):  # (columns of the frame that stay; the rest is black)
            batch[i, :, keep:] = 0
        ref = plain.detect_batch_raw(_host(batch), n_threads=0, cap=16, device_frames=batch)
        print("tags per frame:", list(ref[2]), "status:", list(ref[3]))
        assert ref[0] == AGX_ERR_CAPACITY and (ref[3] == 0).any()
        assert all((ref[3][i] == AGX_ERR_CAPACITY) == (ref[2][i] > 16) for i in range(8))
        assert all(ref[2][i] == full[2][i] > 16 for i in (0, 2, 4, 5, 7))
        frames = _shard(batch, devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=16)
        rc, out, counts, status = _raw_fetch(grp, 8, 16)
        assert rc == AGX_ERR_CAPACITY
        assert np.array_equal(counts, ref[2]) and np.array_equal(status, ref[3]), (counts, status)
        for i in range(8):
            n = int(counts[i]) * TAG_BYTES if status[i] == AGX_OK else 0
            assert out[i, :n].tobytes() == ref[1][i, : counts[i]].tobytes()[:n], i
            assert (out[i, n:] == 0xA5).all(), i
    finally:
        grp.close()


def test_a_full_slab_closes_and_a_retry_succeeds(l8, plain):
    """tags_per_frame 8 with 9 frames per rank: slabs of 72 records.  Rank 0's first two frames (33 .. 36 tags each) fit, its
    third closes the slab: it and every later frame of the rank report AGX_ERR_CAPACITY with the true count and no row.  Rank 1
    holds two frames with tags and seven empty ones, which fit.  A retry with tags_per_frame = the largest count equals the
    plain detector's result."""
    import torch
    fr, _ = l8
    devices = _devices(2)
    grp = _group(devices, device_tail=1)
    try:
        blank = torch.zeros_like(fr[:7])
        batch = torch.cat([fr[:9], fr[9:11], blank]).contiguous()
        ref = plain.detect_batch_raw(_host(batch), n_threads=0, cap=64, device_frames=batch)
        assert ref[0] == AGX_OK and (ref[2][:11] >= 33).all() and (ref[2][11:] == 0).all()
        assert ref[2][0] + ref[2][1] <= 72 < ref[2][0] + ref[2][1] + ref[2][2]
        frames = _shard(batch, devices)
        _sync(devices)
        grp.detect_enqueue(frames, cap=64, tags_per_frame=8)
        rc, out, counts, status = _raw_fetch(grp, 18, 64)
        assert rc == AGX_ERR_CAPACITY
        assert np.array_equal(counts, ref[2])  # the true count, fitting or not
        assert list(status) == [0, 0] + [AGX_ERR_CAPACITY] * 7 + [0] * 9, status
        msg = _last_error(grp)
        assert "slab" in msg and "rank 0" in msg and "frame 2" in msg, msg
        for i in range(18):
            n = int(counts[i]) * TAG_BYTES if status[i] == AGX_OK else 0
            assert out[i, :n].tobytes() == ref[1][i, : counts[i]].tobytes()[:n], i
            assert (out[i, n:] == 0xA5).all(), i  # nothing beyond a frame's own rows
        grp.detect_enqueue(frames, cap=64, tags_per_frame=int(counts.max()))
        assert_same(ref, grp.detect_fetch_raw(), "retry")
    finally:
        grp.close()


def _pack_model(counts, status, slab):
    """What k_pack_scan must report: -> (offsets, frames that find the slab closed), from the frames' true counts and statuses."""
    rows = np.where(status == AGX_OK, counts, 0).astype(np.int64)
    off = np.cumsum(rows) - rows
    return off, (status == AGX_OK) & (off + rows > slab)


@pytest.mark.parametrize("n_frames,boundary", [(130, 64), (1100, 1024)])
def test_offsets_across_waves_and_chunks_and_a_slab_closed_late(l8, plain, n_frames, boundary):
    """One rank with 130 and with 1100 frames, so that k_pack_scan's offsets cross its waves (64 frames) and its chunks (1024
    frames, the running carry).  The head of the batch is three empty frames for every whole board (33 .. 36 tags); the tail
    alternates whole boards with frames cut down to a strip of theirs (about a dozen tags).  tags_per_frame is chosen, from the
    plain detector's counts, so that the slab closes behind `boundary` on a whole board while it still has room for a cut-down
    frame: every frame behind it, those smaller ones included, must report AGX_ERR_CAPACITY with its true count and no row --
    nothing is squeezed in -- and every frame before it must hold the plain detector's rows, which proves its offset."""
    import torch
    fr, full = l8
    small = fr[[1, 3]].clone()
    small[0, :, 200:] = 0
    small[1, :, 260:] = 0
    n_tail = 60 if n_frames == 130 else 100
    pick = np.full(n_frames, -1)  # -1 an empty frame, 0 .. 11 a whole board, 12 / 13 a cut-down one
    head = np.arange(0, n_frames - n_tail, 4)
    pick[head] = (head // 4) % 12
    tail = np.arange(n_frames - n_tail, n_frames)
    pick[tail] = np.where(tail % 2 == 0, (tail // 2) % 12, 12 + (tail // 2) % 2)
    pool = torch.cat([fr, small, torch.zeros_like(fr[:1])]).contiguous()  # (-1 indexes the empty frame)
    pool_cnt = plain.detect_batch_raw(_host(pool), n_threads=0, cap=64, device_frames=pool)[2].astype(np.int64)
    assert (pool_cnt[:12] >= 33).all() and (pool_cnt[12:14] > 0).all() and (pool_cnt[12:14] < 20).all() and pool_cnt[14] == 0, pool_cnt

    def closing(pick, tpf):
        """-> (slab, offsets, closed, first closed frame) if tags_per_frame tpf closes the slab as the test wants it, else None."""
        cnt = pool_cnt[pick]
        slab = n_frames * tpf
        off, closed = _pack_model(cnt, np.zeros(n_frames, np.int32), slab)
        c = int(np.argmax(closed))
        later = np.arange(n_frames) > c
        if closed.any() and c > boundary and pick[c] < 12 and (later & (cnt > 0) & (cnt <= slab - off[c])).any():
            return slab, off, closed, c
        return None

    # the slab is a multiple of n_frames records: empty as many of the head's boards as it takes for one to close it that way
    choice = None
    for emptied in range(len(head)):
        for tpf in range(1, 64):
            choice = closing(pick, tpf)
            if choice:
                break
        if choice:
            break
        pick[head[emptied]] = -1
    assert choice is not None, "no tags_per_frame closes the slab behind frame %d with room for a smaller frame" % boundary
    slab, off, closed, c = choice
    batch = pool[torch.from_numpy(pick).to(fr.device)].contiguous()
    ref = plain.detect_batch_raw(_host(batch), n_threads=0, cap=64, device_frames=batch)
    rc, rows, cnt, st = ref
    assert rc == AGX_OK and np.array_equal(cnt, pool_cnt[pick])  # (a frame's tags do not depend on its neighbours)
    assert (np.arange(n_frames)[c + 1:][(cnt[c + 1:] > 0) & (cnt[c + 1:] <= slab - off[c])]).size > 0
    print("%d frames, %d tags; tags_per_frame %d: the slab of %d closes at frame %d (offset %d, %d tags), %d frames behind it"
          % (n_frames, int(cnt.sum()), tpf, slab, c, off[c], cnt[c], int(closed[c + 1:].sum())))
    grp = _group([0], device_tail=1)
    try:
        _sync([0])
        grp.detect_enqueue([batch], cap=64, tags_per_frame=tpf)
        rc2, out, counts, status = _raw_fetch(grp, n_frames, 64)
        assert rc2 == AGX_ERR_CAPACITY
        assert _sum(grp, "last_device_tail_frames") == n_frames and _sum(grp, "last_device_tail_fallbacks") == 0  # (all packed)
        assert np.array_equal(counts, cnt)
        assert np.array_equal(status, np.where(closed, AGX_ERR_CAPACITY, st)), np.nonzero(status != np.where(closed, AGX_ERR_CAPACITY, st))
        assert closed[c:][st[c:] == AGX_OK].all()  # (the model's own rule: closed stays closed)
        msg = _last_error(grp)
        assert "slab" in msg and "rank 0" in msg and "frame %d:" % c in msg, msg
        for i in range(n_frames):
            n = int(counts[i]) * TAG_BYTES if status[i] == AGX_OK else 0
            assert out[i, :n].tobytes() == rows[i, : counts[i]].tobytes()[:n], i
            assert (out[i, n:] == 0xA5).all(), i
        # with room for every tag the same batch comes back whole
        grp.detect_enqueue([batch], cap=64, tags_per_frame=-(-int(cnt.sum()) // n_frames))
        assert_same(ref, grp.detect_fetch_raw(), "exactly enough room")
    finally:
        grp.close()


def test_state_and_argument_rules(l8):
    import aprilgrid_rs_amd as A
    fr, ref = l8
    devices = _devices(2)
    grp = _group(devices)
    lib = grp._lib
    try:
        frames = _shard(fr[:6], devices)
        _sync(devices)
        n, cap = 6, 64
        out = np.zeros((n, cap * TAG_BYTES), np.uint8)
        counts = np.zeros(n, np.uint32)
        sad = np.zeros((n, 2048, 5), np.float32)
        ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in frames])
        geom = (3, 640, 400, 640, 640 * 400, 0)

        def fetch():
            return lib.agx_group_detect_fetch(grp._g, out.ctypes.data, counts.ctypes.data, None, 0)

        def saddles_fetch():
            return lib.agx_group_saddles_fetch(grp._g, sad.ctypes.data, 2048, counts.ctypes.data, None)

        assert fetch() == AGX_ERR_STATE  # nothing enqueued
        assert lib.agx_group_detect_enqueue(grp._g, None, *geom, cap, 0) == AGX_ERR_ARG
        assert lib.agx_group_detect_enqueue(grp._g, ptrs, 0, *geom[1:], cap, 0) == AGX_ERR_ARG
        one_null = (C.c_void_p * 2)(frames[0].data_ptr(), None)
        assert lib.agx_group_detect_enqueue(grp._g, one_null, *geom, cap, 0) == AGX_ERR_ARG
        assert fetch() == AGX_ERR_STATE  # ... and none of them left a batch behind

        assert lib.agx_group_detect_enqueue(grp._g, ptrs, *geom, cap, 0) == AGX_OK
        assert saddles_fetch() == AGX_ERR_STATE  # the other kind's fetch
        assert lib.agx_group_detect_fetch(grp._g, out.ctypes.data, None, None, 0) == AGX_ERR_ARG
        assert lib.agx_group_detect_fetch(grp._g, None, counts.ctypes.data, None, 0) == AGX_ERR_ARG
        # a borrowed detector's own fetches of the group's batch
        for r in range(2):
            h = _handle(grp, r)
            assert lib.agx_detect_batch_fetch(h, out.ctypes.data, counts.ctypes.data, None, 0) == AGX_ERR_STATE
            assert lib.agx_saddles_batch_fetch(h, sad.ctypes.data, 2048, counts.ctypes.data, None) == AGX_ERR_STATE
        assert fetch() == AGX_OK  # ... and the batch is still whole
        got = out.view(A.TagDetector.TAG_DTYPE).reshape(n, cap)
        assert np.array_equal(counts, ref[2][:6])
        for i in range(6):
            assert got[i, : counts[i]].tobytes() == ref[1][i, : counts[i]].tobytes(), i
        assert fetch() == AGX_ERR_STATE  # resolved by its fetch
        assert saddles_fetch() == AGX_ERR_STATE

        grp.saddles_enqueue(frames)
        assert fetch() == AGX_ERR_STATE  # the reverse
        res, status = grp.saddles_fetch()
        assert (status == 0).all() and all(len(s) > 50 for s in res)
        # a detect batch replaces a saddle batch in flight
        grp.saddles_enqueue(frames)
        grp.detect_enqueue(frames, cap=cap)
        assert saddles_fetch() == AGX_ERR_STATE
        assert_same(_ref_slice((ref[0], ref[1][:, :cap], ref[2], ref[3]), 6), grp.detect_fetch_raw(), "after a saddle batch")
    finally:
        grp.close()


def test_the_gathered_results_are_the_same_bytes_every_run(l8):
    fr, _ = l8
    devices = _devices(3)
    grp = _group(devices)
    try:
        frames = _shard(fr, devices)
        _sync(devices)
        runs = []
        for rep in range(2):
            grp.detect_enqueue(frames, cap=48, tags_per_frame=40)
            rc, out, counts, status = _raw_fetch(grp, 12, 48)
            assert rc == AGX_OK
            runs.append(out.tobytes() + counts.tobytes() + status.tobytes())
        assert runs[0] == runs[1]
    finally:
        grp.close()


_GUARDED = r"""
import ctypes as C
import numpy as np
import torch
import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth

n_dev = torch.cuda.device_count()
devices = [r % n_dev for r in range(2)]
grp = A.DetectorGroup("t36h11", devices, transport="peer")
dets = [C.c_void_p(grp._lib.agx_group_detector(grp._g, r)) for r in range(2)]

def guards(what):
    for r, h in enumerate(dets):
        buf = np.zeros(6, np.uint32)
        n = C.c_size_t(0)
        assert grp._lib.agx_debug_fetch(h, 0, 8, buf.ctypes.data, buf.nbytes, C.byref(n)) == 0
        assert buf[0] > 0 and buf[1] == 0, (what, r, list(buf))

def run(frames, cap, tpf, what):
    grp.detect_enqueue(frames, cap=cap, tags_per_frame=tpf)
    rc, out, counts, status = grp.detect_fetch_raw(2)
    guards(what)
    return rc, counts

fr = synth.render_batch(50, 8, 640, 400, device="cuda:0")[0]
frames = [fr[4 * r:4 * r + 4].to("cuda:%d" % devices[r]).contiguous() for r in range(2)]
for d in set(devices):
    torch.cuda.synchronize(d)
rc, counts = run(frames, 64, 0, "packed")
assert rc == 0 and counts.min() >= 30
rc, _ = run(frames, 64, 8, "slab full")
assert rc == -3
rc, _ = run(frames, 4, 0, "cap 4")
assert rc == -3
for h in dets:
    grp._lib.agx_detector_set_option(h, b"tail_debug_band", 50)
run(frames, 64, 0, "hand-back")
for h in dets:
    grp._lib.agx_detector_set_option(h, b"tail_debug_band", 0)
    assert grp._lib.agx_detector_set_option(h, b"device_tail", 0) == 0
rc, _ = run(frames, 64, 0, "host tail")
assert rc == 0
grp.close()
print("GUARDS INTACT", flush=True)
"""


def test_guard_bytes_of_every_ranks_detector():
    """The group's paths in a child process with AGX_REDZONE_BYTES set: packed, a full slab, cap 4, hand-back and the host tail
    leave every guard byte of both ranks' detectors intact (workspace, the tail's device tables k_pack_tags reads, the pinned luma
    planes).  The group's own tables and slabs are plain allocations outside those guards: what protects them is
    k_pack_tags' bound against slab_records, which the full-slab tests exercise."""
    env = dict(os.environ, AGX_REDZONE_BYTES=str(1 << 16))
    r = subprocess.run([sys.executable, "-c", _GUARDED], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "GUARDS INTACT" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
