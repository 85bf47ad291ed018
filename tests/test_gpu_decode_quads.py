"""Decode of caller-given quads on device batches (agx_decode_quads_enqueue / _fetch, agx_decode_quads; kernel k_decode_quads;
reference src/detector.rs:448-476).  Two references: the host's agx_decode_quads_tail on the same luma and quads -- every slot
and every field, bits included, no exclusions: kernel and host share their arithmetic -- and the yardstick of
tests/test_decode_quads_cpu.py (the oracle's decode stages composed) outside its knife-edge set.

Frames are 320 x 200 synthetic (tests/test_decode_quads_cpu.py checks on the CPU that the oracle decodes at least half of the
ground-truth quads of every family at that size, and that at most 10 % of any input set here is knife-edge)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_decode_quads_cpu as cases
from tests.test_decode_quads_cpu import DECODED, NO_MATCH, OUTSIDE, SKIPPED, TAG_DTYPE
from tests.util import ROOT, check_tags, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_STATE = 0, -1, -2, -7
L8, L16, RGB8, LF32, BGRA8, RGB8P = 0, 1, 2, 3, 7, 8
W, H = cases.GPU_SIZE
UNWRITTEN = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def tail(fam, luma, quads):
    import aprilgrid_rs_amd as A
    return A.decode_quads_tail(fam, luma, np.asarray(quads, np.float32).reshape(-1, 8), with_bits=True)


def same(got, ref, what):
    """(tags, status, bits) of the device against the host's, byte for byte."""
    for g, r, field in zip(got, ref, ("tags", "status", "bits")):
        assert np.asarray(g).tobytes() == np.asarray(r).tobytes(), "%s: %s differ at %s" % (
            what, field, np.flatnonzero(np.asarray(g).reshape(-1) != np.asarray(r).reshape(-1))[:8])


jittered_quads = cases.jittered_quads


@pytest.fixture(scope="module")
def base():
    """3 frames x 64 quads: the host's results and the yardstick's, computed once."""
    frames, quads = jittered_quads(3, 64, 11)
    ref = [tail("t36h11", frames[f], quads[f]) for f in range(3)]
    yard = [cases.yardstick_many(frames[f], quads[f], "T36H11") for f in range(3)]
    return {"frames": frames, "quads": quads, "ref": ref, "yard": yard, "d_frames": dev(frames), "d_quads": dev(quads)}


def run(det, d_frames, d_quads, counts=None, format=None):
    det.decode_quads_enqueue(d_frames, d_quads, counts=counts, format=format)
    return det.decode_quads_fetch()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
def test_parity_with_the_host_tail_and_the_yardstick(det, base):
    tags, st, bits = run(det, base["d_frames"], base["d_quads"])
    for f in range(3):
        same((tags[f], st[f], bits[f]), base["ref"][f], "frame %d" % f)
        cases.check_against_yardstick((tags[f], st[f], bits[f]), base["yard"][f], "frame %d" % f)
    assert (st == DECODED).sum() >= st.size // 3 and len(np.unique(st)) >= 3, np.bincount(st.reshape(-1))


# ---- 2. lane and wave geometry, counts, sentinels ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("qpf", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000])
def test_lane_and_wave_geometry_with_counts(det, qpf, n_frames):
    """Every slot against the host; per-frame counts 0, partial and above quads_per_frame; caller-owned outputs pre-filled with a
    sentinel, which the slots at or beyond a frame's count keep."""
    import torch
    frames, quads = jittered_quads(n_frames, qpf, 100 + qpf)
    counts = np.array([qpf + 7, 0, qpf // 2][:n_frames] if n_frames == 3 else [max(qpf - 1, 0) if qpf > 4 else qpf + 1], np.int32)
    for c in (None, counts):
        d_tags = torch.full((n_frames, qpf, 9), SENTINEL, dtype=torch.int32, device="cuda")
        d_st = torch.full((n_frames, qpf), SENTINEL, dtype=torch.int32, device="cuda")
        d_bits = torch.full((n_frames, qpf), SENTINEL, dtype=torch.int64, device="cuda")
        det.decode_quads_enqueue(dev(frames), dev(quads), counts=None if c is None else dev(c), out=d_tags, status=d_st, bits=d_bits)
        det.decode_quads_fetch()
        tags = d_tags.cpu().numpy().view(np.uint32)
        st, bits = d_st.cpu().numpy().view(np.uint32), d_bits.cpu().numpy()
        for f in range(n_frames):
            n = qpf if c is None else min(int(c[f]), qpf)
            ref = tail("t36h11", frames[f], quads[f][:n])
            same((tags[f, :n].reshape(-1).view(TAG_DTYPE), st[f, :n], bits[f, :n].view(np.uint64)), ref, "qpf %d frame %d" % (qpf, f))
            assert (tags[f, n:] == SENTINEL).all() and (st[f, n:] == SENTINEL).all() and (bits[f, n:] == SENTINEL).all(), (qpf, f)
        # the same batch into the internal buffers: the fetch leaves the slots beyond a count as they were
        t2, s2, b2 = run(det, dev(frames), dev(quads), counts=None if c is None else dev(c))
        for f in range(n_frames):
            n = qpf if c is None else min(int(c[f]), qpf)
            assert t2[f, :n].tobytes() == tags[f, :n].tobytes() and np.array_equal(s2[f, :n], st[f, :n]) and np.array_equal(b2[f, :n].view(np.int64), bits[f, :n])
            assert (s2[f, n:] == UNWRITTEN).all() and not t2[f, n:].tobytes().strip(b"\0") and not b2[f, n:].any()


# ---- 3. families -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", cases.FAMILIES)
def test_every_family(fam):
    """Edge 4, 5, 6 and border 1, 2: 16, 25 and 36 samples against the eight-lane sample loop; 30, 35, 242 and 587 codes against
    the 16-lane scan's remainder."""
    import aprilgrid_rs_amd as A
    frames, quads, ids = cases.gt_case(fam, 0, 3, W, H)
    q = max(len(x) for x in quads)
    packed = np.zeros((3, q, 8), np.float32)
    counts = np.array([len(x) for x in quads], np.int32)
    for f in range(3):
        packed[f, :len(quads[f])] = quads[f]
    d = A.TagDetector(fam, None, device=0)
    try:
        tags, st, bits = run(d, dev(frames), dev(packed), counts=dev(counts))
    finally:
        d.close()
    n_dec = 0
    for f in range(3):
        n = counts[f]
        got = (tags[f, :n], st[f, :n], bits[f, :n])
        same(got, tail(fam, frames[f], quads[f]), "%s frame %d" % (fam, f))
        cases.check_against_yardstick(got, cases.yardstick_many(frames[f], quads[f], fam), "%s frame %d" % (fam, f))
        dec = st[f, :n] == DECODED
        assert np.array_equal(tags[f, :n]["id"][dec], ids[f][dec]), fam
        n_dec += int(dec.sum())
    assert 2 * n_dec >= counts.sum(), (fam, n_dec, counts.sum())


# ---- 4. each reason through the batch path -----------------------------------------------------------------------------------
def test_each_reason_through_the_batch_path():
    import aprilgrid_rs_amd as A
    luma, cs = cases.constructed_cases()
    seen = set()
    for fam in sorted(set(c[2] for c in cs.values())):
        names = sorted(n for n in cs if cs[n][2] == fam)
        quads = np.array([cs[n][0] for n in names], np.float32)
        d = A.TagDetector(fam, None, device=0)
        try:
            tags, st, bits = run(d, dev(luma[None]), dev(quads[None]))
        finally:
            d.close()
        assert [int(s) for s in st[0]] == [cs[n][1] for n in names], dict(zip(names, st[0]))
        same((tags[0], st[0], bits[0]), tail(fam, luma, quads), fam)
        cases.check_against_yardstick((tags[0], st[0], bits[0]), cases.yardstick_many(luma, quads, fam), fam)
        seen |= set(int(s) for s in st[0])
    assert seen == {0, 1, 2, 3, 4}


# ---- 5. formats --------------------------------------------------------------------------------------------------------------
def test_l8_with_padded_row_and_frame_strides(det, base):
    import torch
    n, row, frame = 3, W + 24, (W + 24) * (H + 3) + 5
    buf = torch.full((n * frame + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    for f in range(n):
        buf[f * frame: f * frame + row * H].view(H, row)[:, :W] = base["d_frames"][f]
    det._follow_torch_stream()
    det._check(det._lib.agx_decode_quads_enqueue(det._h, buf.data_ptr(), n, W, H, row, frame, L8, base["d_quads"].data_ptr(), 8, 64, None, None,
                                                 None, None, None))
    tags, st, bits = np.zeros((n, 64), TAG_DTYPE), np.zeros((n, 64), np.uint32), np.zeros((n, 64), np.uint64)
    det._check(det._lib.agx_decode_quads_fetch(det._h, tags.ctypes.data, st.ctypes.data, bits.ctypes.data))
    for f in range(n):
        same((tags[f], st[f], bits[f]), base["ref"][f], "padded strides, frame %d" % f)


def other_format(frames, name, seed=3):
    """The L8 frames as another layout with a little colour / low-byte noise -> (array, agx_format)"""
    rng = np.random.default_rng(seed)
    x = frames.astype(np.int64)
    if name == "L16":
        return np.clip(x * 257 + rng.integers(-60, 61, x.shape), 0, 65535).astype(np.uint16), L16
    ch = [np.clip(x + rng.integers(-2, 3, x.shape), 0, 255).astype(np.uint8) for _ in range(3)]
    if name == "RGB8":
        return np.stack(ch, axis=-1), RGB8
    if name == "BGRA8":
        return np.stack([ch[2], ch[1], ch[0], rng.integers(0, 256, x.shape).astype(np.uint8)], axis=-1), BGRA8
    assert name == "RGB8P"
    return np.stack(ch, axis=1), RGB8P


@pytest.mark.parametrize("name", ["L16", "RGB8", "BGRA8", "RGB8P"])
def test_other_formats_decode_on_the_device_luma(det, base, name):
    import aprilgrid_rs_amd as A
    arr, fmt = other_format(base["frames"], name)
    tags, st, bits = run(det, dev(arr), base["d_quads"], format=fmt)
    for f in range(3):
        luma = A.TagDetector.luma8(arr[f], format=fmt)
        same((tags[f], st[f], bits[f]), tail("t36h11", luma, base["quads"][f]), "%s frame %d" % (name, f))
    assert (st == DECODED).sum() >= st.size // 3


def test_f32_planes_are_refused(det, base):
    import torch
    import aprilgrid_rs_amd as A
    planes = torch.zeros((1, H, W), dtype=torch.float32, device="cuda")
    with pytest.raises(A.AgxError) as e:
        det.decode_quads_enqueue(planes, base["d_quads"][:1])
    assert e.value.status == AGX_ERR_FORMAT
    with pytest.raises(A.AgxError) as e:
        det.decode_quads(np.zeros((H, W), np.float32), base["quads"][0])
    assert e.value.status == AGX_ERR_FORMAT


# ---- 6. refine, then decode, without leaving the device ----------------------------------------------------------------------
def test_refined_records_and_point_statuses_are_read_in_place(det, base):
    """agx_refine_points_enqueue into caller-owned device arrays, not fetched; agx_decode_quads_enqueue on those arrays (point
    stride 20, d_point_status); one fetch.  Equals: refine, fetch to the host, mark the quads with a corner that was not refined
    SKIPPED, repack [n][8], decode with stride 8."""
    import torch
    frames, quads, _ = cases.gt_case("T36H11", 0, 3, W, H)
    rng = np.random.default_rng(5)
    q = min(len(x) for x in quads)
    pts = np.stack([x[:q] for x in quads]).reshape(3, q * 4, 2)
    pts = (pts + rng.uniform(-1.0, 1.0, pts.shape)).astype(np.float32)
    pts[0, 5], pts[1, 17], pts[2, 4 * q - 1] = (-50.0, 10.0), (np.nan, 20.0), (W + 4.0, 30.0)  # forced AGX_POINT_OUTSIDE
    d_frames, d_pts = dev(frames), dev(pts)
    rec = torch.zeros((3, 4 * q, 5), dtype=torch.float32, device="cuda")
    pst = torch.zeros((3, 4 * q), dtype=torch.int32, device="cuda")
    det.refine_points_enqueue(d_frames, d_pts, out=rec, status=pst)
    det.decode_quads_enqueue(d_frames, refined=(rec, pst))  # (the refine batch is not fetched)
    tags, st, bits = det.decode_quads_fetch()
    # the reference sequence
    h_rec, h_pst = run_refine(det, d_frames, d_pts)
    assert np.array_equal(rec.cpu().numpy().view(np.uint32), np.stack([h_rec[k] for k in ("x", "y", "k", "theta", "phi")], axis=-1).view(np.uint32))
    skipped = (h_pst.reshape(3, q, 4) != 0).any(axis=2)
    # (the input serves its purpose if both kinds of quad are there: at this size a pixel of jitter costs most quads a corner)
    assert skipped[0, 1] and skipped[1, 4] and skipped[2, q - 1] and (~skipped).sum() >= 8
    packed = np.stack([h_rec["x"], h_rec["y"]], axis=-1).reshape(3, q, 8)
    t2, s2, b2 = run(det, d_frames, dev(packed))
    s2[skipped], b2[skipped] = SKIPPED, 0
    t2[skipped] = np.zeros((), TAG_DTYPE)
    same((tags, st, bits), (t2, s2, b2), "refine + decode on the device")
    assert (st == SKIPPED).sum() == skipped.sum() and (st == DECODED).sum() >= 1
    for f in range(3):  # and the host's decode of the refined corners
        keep = ~skipped[f]
        same((tags[f][keep], st[f][keep], bits[f][keep]), tail("t36h11", frames[f], packed[f][keep]), "refined corners, frame %d" % f)


def run_refine(det, d_frames, d_pts):
    det.refine_points_enqueue(d_frames, d_pts)
    return det.refine_points_fetch()


# ---- 7. output modes and state -----------------------------------------------------------------------------------------------
def test_output_modes(det, base):
    import torch
    internal = run(det, base["d_frames"], base["d_quads"])
    d_tags = torch.zeros((3, 64, 9), dtype=torch.int32, device="cuda")
    d_st = torch.zeros((3, 64), dtype=torch.int32, device="cuda")
    d_bits = torch.zeros((3, 64), dtype=torch.int64, device="cuda")
    det.decode_quads_enqueue(base["d_frames"], base["d_quads"], out=d_tags, status=d_st, bits=d_bits)
    out = det.decode_quads_fetch()
    assert out[0] is d_tags and out[1] is d_st and out[2] is d_bits
    same((d_tags.cpu().numpy().view(np.uint32).reshape(-1).view(TAG_DTYPE).reshape(3, 64), d_st.cpu().numpy().view(np.uint32),
          d_bits.cpu().numpy().view(np.uint64)), internal, "caller-owned outputs")
    ids, xy = det.split_device_tags(d_tags)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), internal[0]["id"])
    assert np.array_equal(xy.cpu().numpy().reshape(3, 64, 8).view(np.uint32), internal[0]["xy"].view(np.uint32))
    # d_bits NULL
    d_tags2, d_st2 = torch.zeros_like(d_tags), torch.zeros_like(d_st)
    det.decode_quads_enqueue(base["d_frames"], base["d_quads"], out=d_tags2, status=d_st2)
    det.decode_quads_fetch()
    assert torch.equal(d_tags2, d_tags) and torch.equal(d_st2, d_st)
    # the fetch's bits argument NULL
    det.decode_quads_enqueue(base["d_frames"], base["d_quads"])
    tags, st = np.zeros((3, 64), TAG_DTYPE), np.zeros((3, 64), np.uint32)
    det._check(det._lib.agx_decode_quads_fetch(det._h, tags.ctypes.data, st.ctypes.data, None))
    det._decode = None
    assert tags.tobytes() == internal[0].tobytes() and np.array_equal(st, internal[1])
    # one host image
    for f in range(3):
        same(det.decode_quads(base["frames"][f], base["quads"][f], with_bits=True), base["ref"][f], "agx_decode_quads, frame %d" % f)
    t, s = det.decode_quads(base["frames"][0], np.zeros((0, 8), np.float32))
    assert len(t) == 0 and len(s) == 0


def test_state_and_argument_rules(det, base):
    import torch
    import aprilgrid_rs_amd as A
    lib, h = det._lib, det._h
    tags, st, bits = np.zeros((3, 64), TAG_DTYPE), np.zeros((3, 64), np.uint32), np.zeros((3, 64), np.uint64)
    fetch = lambda: lib.agx_decode_quads_fetch(h, tags.ctypes.data, st.ctypes.data, bits.ctypes.data)
    det.sync()
    det.decode_quads_enqueue(base["d_frames"], base["d_quads"])
    det.decode_quads_fetch()
    assert fetch() == AGX_ERR_STATE  # a second fetch
    fresh = A.TagDetector("t36h11", None, device=0)
    try:
        assert fresh._lib.agx_decode_quads_fetch(fresh._h, tags.ctypes.data, st.ctypes.data, bits.ctypes.data) == AGX_ERR_STATE  # nothing in flight
    finally:
        fresh.close()
    # the other kinds' fetches on a decode batch
    det.decode_quads_enqueue(base["d_frames"], base["d_quads"])
    cnt, fst = np.zeros(3, np.uint32), np.zeros(3, np.int32)
    assert lib.agx_saddles_batch_fetch(h, None, 0, cnt.ctypes.data, fst.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_detect_batch_fetch(h, tags.ctypes.data, cnt.ctypes.data, fst.ctypes.data, 1) == AGX_ERR_STATE
    assert lib.agx_refine_points_fetch(h, tags.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    assert fetch() == AGX_OK  # ... which leave it in flight
    same((tags, st, bits), [np.stack([r[i] for r in base["ref"]]) for i in range(3)], "after the refused fetches")
    # a decode fetch on a saddle batch, and on a refine batch
    det.saddles_batch_enqueue(base["d_frames"])
    assert fetch() == AGX_ERR_STATE
    det.saddles_batch_fetch()
    det.refine_points_enqueue(base["d_frames"], dev(base["quads"][:, :, :2].copy()))
    assert fetch() == AGX_ERR_STATE
    det.refine_points_fetch()
    # arguments
    fr, q = base["d_frames"], base["d_quads"]
    t9 = torch.zeros((3, 64, 9), dtype=torch.int32, device="cuda")
    s1 = torch.zeros((3, 64), dtype=torch.int32, device="cuda")
    enq = lambda frames, quads, stride, qpf, dt, ds: lib.agx_decode_quads_enqueue(h, frames, 3, W, H, W, W * H, L8, quads, stride, qpf, None, None, dt, ds, None)
    assert enq(None, q.data_ptr(), 8, 64, None, None) == AGX_ERR_ARG
    assert enq(fr.data_ptr(), None, 8, 64, None, None) == AGX_ERR_ARG
    assert enq(fr.data_ptr(), q.data_ptr(), 8, 0, None, None) == AGX_ERR_ARG
    for stride in (0, 4, 10, 7):
        assert enq(fr.data_ptr(), q.data_ptr(), stride, 64, None, None) == AGX_ERR_ARG
    assert enq(fr.data_ptr(), q.data_ptr(), 8, 64, t9.data_ptr(), None) == AGX_ERR_ARG
    assert enq(fr.data_ptr(), q.data_ptr(), 8, 64, None, s1.data_ptr()) == AGX_ERR_ARG
    assert lib.agx_decode_quads_enqueue(h, fr.data_ptr(), 3, W, H, W, W * H, LF32, q.data_ptr(), 8, 64, None, None, None, None, None) == AGX_ERR_FORMAT
    assert fetch() == AGX_ERR_STATE  # (a refused enqueue leaves nothing in flight)


def test_on_a_callers_stream_with_an_event_behind_it(det, base):
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        frames = base["d_frames"].clone()
        quads = base["d_quads"] + 0.0
        d_tags = torch.zeros((3, 64, 9), dtype=torch.int32, device="cuda")
        d_st = torch.zeros((3, 64), dtype=torch.int32, device="cuda")
        det.decode_quads_enqueue(frames, quads, out=d_tags, status=d_st)  # (follows torch's current stream: s)
        ev = torch.cuda.Event()
        ev.record(s)
    ev.synchronize()  # the results are final behind the event, without a fetch
    assert np.array_equal(d_st.cpu().numpy().view(np.uint32), np.stack([r[1] for r in base["ref"]]))
    assert d_tags.cpu().numpy().view(np.uint32).tobytes() == np.stack([r[0] for r in base["ref"]]).tobytes()
    det.decode_quads_fetch()
    torch.cuda.current_stream().synchronize()


# ---- 8. the other batches are unchanged --------------------------------------------------------------------------------------
def test_detect_behind_a_decode_batch_equals_a_fresh_handle(det, base):
    import aprilgrid_rs_amd as A
    synth = synth_module()
    frames = np.stack([synth.render_frame(40 + i, 640, 400)[0].numpy() for i in range(2)])
    d_frames = dev(frames)
    arr, fmt = other_format(base["frames"], "RGB8")
    det.decode_quads_enqueue(dev(arr), base["d_quads"], format=fmt)  # (not fetched: the detect batch replaces it)
    got = det.detect_batch_device(d_frames)
    fresh = A.TagDetector("t36h11", None, device=0)
    try:
        ref = fresh.detect_batch_device(d_frames)
    finally:
        fresh.close()
    for f in range(2):
        check_tags(got[f], ref[f], "frame %d" % f)
        assert len(ref[f]) >= 30


# ---- 9. guard bytes ----------------------------------------------------------------------------------------------------------
def guard_child():
    """Runs in a child process with AGX_REDZONE_BYTES set: the 1000-quad and the 17-quad case and a colour format on a handle
    with guard bytes around every buffer; prints the guard report."""
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    before = d.debug_fetch(0, "redzones")["buffers"]
    for qpf in (1000, 17):
        frames, quads = jittered_quads(3, qpf, 100 + qpf)
        counts = np.array([qpf + 7, 0, qpf // 2], np.int32)
        tags, st, bits = run(d, dev(frames), dev(quads), counts=dev(counts))
        for f in range(3):
            n = min(int(counts[f]), qpf)
            same((tags[f, :n], st[f, :n], bits[f, :n]), tail("t36h11", frames[f], quads[f][:n]), "guarded, qpf %d frame %d" % (qpf, f))
    frames, quads = jittered_quads(3, 17, 117)
    arr, fmt = other_format(frames, "BGRA8")
    tags, st, bits = run(d, dev(arr), dev(quads), format=fmt)
    for f in range(3):
        same((tags[f], st[f], bits[f]), tail("t36h11", A.TagDetector.luma8(arr[f], format=fmt), quads[f]), "guarded BGRA8 frame %d" % f)
    same(d.decode_quads(frames[0], quads[0], with_bits=True), tail("t36h11", frames[0], quads[0]), "guarded host image")
    r = d.debug_fetch(0, "redzones")
    d.close()
    print("GUARDS buffers_before=%d buffers=%d damaged=%d" % (before, r["buffers"], r["damaged_bytes"]))


def test_guard_bytes_stay_intact_in_a_child_process():
    env = dict(os.environ, AGX_REDZONE_BYTES=str(1 << 16))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests import test_gpu_decode_quads as t; t.guard_child()" % ROOT],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("GUARDS")][-1]
    v = dict(kv.split("=") for kv in line.split()[1:])
    assert int(v["damaged"]) == 0, line
    # the code list, the luma pair, the staging buffer and the new side buffers (tags, statuses, bits, the host image's quads)
    assert int(v["buffers"]) - int(v["buffers_before"]) >= 8, line


# ---- 10. determinism ---------------------------------------------------------------------------------------------------------
def test_the_same_batch_twice_gives_the_same_bytes(det, base):
    a = run(det, base["d_frames"], base["d_quads"])
    b = run(det, base["d_frames"], base["d_quads"])
    same(a, b, "second run")
