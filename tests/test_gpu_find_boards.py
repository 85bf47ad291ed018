"""Board search in caller-given saddle lists on device batches (agx_find_boards_enqueue / _fetch, agx_find_board; kernel
k_find_boards; reference src/detector.rs:588-639).  Two references: the host form agx_find_board_tail on the same list -- count,
every quad and the order -- and, for the lists the chain produced, the oracle's orc_try_find_best_board
(tests/test_find_boards_cpu.py).

The lists come from agx_saddles_batch_enqueue_to on 8 synthetic frames of 640 x 400 showing the 6 x 6 board:
tests/test_find_boards_cpu.py checks on the CPU that the host form finds a board in the oracle's list of every one of them, and
that most reach the score-36 stop."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_find_boards_cpu as cases
from tests.util import ROOT, bits_equal, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
FOUND, NONE, CAPACITY, INPUT, PENDING = 0, 1, 2, 3, 4
W, H = cases.GPU_SIZE
N = cases.GPU_FRAMES
Q = 64  # rows per frame: the board has 36 tags
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(saddles):
    """The host form on one list -> (quads [n, 4] uint32, status, n)."""
    import aprilgrid_rs_amd as A
    return A.find_board_tail(np.ascontiguousarray(saddles, np.float32).reshape(-1, 5), cap=1024)


def check_frame(quads, n, status, ref, what):
    rq, rst, rn = ref
    assert (int(status), int(n)) == (rst, rn), "%s: status %d count %d, host %d %d" % (what, status, n, rst, rn)
    if rst == FOUND:
        assert np.array_equal(np.asarray(quads)[:rn].astype(np.int64), rq.astype(np.int64)), what + ": quads or their order"


def handed_back(det):
    return det.get_option("last_find_boards_frames"), det.get_option("last_find_boards_handed_back")


@pytest.fixture(scope="module")
def base(det):
    """The chain's device lists of the 8 frames, their host copies, the host form's answers."""
    import torch
    synth = synth_module()
    frames, gt = synth.render_batch(cases.GPU_FIRST, N, W, H, device="cuda")
    d_saddles = torch.zeros((N * 1024, 5), dtype=torch.float32, device="cuda")
    d_table = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    det.saddles_batch_enqueue_to(frames, d_saddles, d_table)
    det.sync()
    table = d_table.cpu().numpy()
    all_s = d_saddles.cpu().numpy()
    lists = [all_s[table[f, 1]:table[f, 1] + table[f, 0]].copy() for f in range(N)]
    assert not (table[:, 2] & 7).any() and all(len(l) > 100 for l in lists)
    ref = [host(l) for l in lists]
    assert all(r[1] == FOUND for r in ref) and sum(r[2] == 36 for r in ref) >= N // 2, [r[1:] for r in ref]
    # the same lists as a padded [N, S, 5] batch with counts
    S = max(len(l) for l in lists) + 3
    padded = np.full((N, S, 5), np.nan, np.float32)
    for f in range(N):
        padded[f, :len(lists[f])] = lists[f]
    return {"frames": frames, "gt": gt, "d_saddles": d_saddles, "d_table": d_table, "lists": lists, "ref": ref, "padded": padded,
            "counts": np.array([len(l) for l in lists], np.int32)}


# ---- 1. parity through the frame table ---------------------------------------------------------------------------------------
def test_parity_through_the_frame_table(det, base):
    det.find_boards_enqueue(base["d_saddles"], frame_table=base["d_table"], quads_per_frame=Q)
    quads, pts, n, st = det.find_boards_fetch()
    assert handed_back(det) == (N, 0)
    for f in range(N):
        check_frame(quads[f], n[f], st[f], base["ref"][f], "frame %d" % f)
        yard = cases.yardstick(base["lists"][f])
        assert yard is not None and np.array_equal(quads[f, :n[f]].astype(np.int64), yard.astype(np.int64)), "frame %d against the yardstick" % f
        l = base["lists"][f]
        assert bits_equal(pts[f, :n[f]], np.stack([l[:, 0][quads[f, :n[f]]], l[:, 1][quads[f, :n[f]]]], axis=-1)), "frame %d: quad points" % f
        assert (quads[f, n[f]:] == 0xFFFFFFFF).all()  # rows beyond the count: as the fetch found them


# ---- 2. the chain on the device ----------------------------------------------------------------------------------------------
def test_find_boards_feeds_decode_quads_in_place(base):
    """One board per frame and max_num_of_boards = 1: detect's tags are the first board's content."""
    import torch
    import aprilgrid_rs_amd as A
    prm = A.DetectorParams.default_params()
    prm.max_num_of_boards = 1
    d = A.TagDetector("t36h11", prm, device=0)
    try:
        frames = base["frames"]
        d_saddles = torch.zeros((N * 1024, 5), dtype=torch.float32, device="cuda")
        d_table = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
        d_quads = torch.zeros((N, Q, 4), dtype=torch.int32, device="cuda")
        d_pts = torch.zeros((N, Q, 4, 2), dtype=torch.float32, device="cuda")
        d_n = torch.zeros(N, dtype=torch.int32, device="cuda")
        d_st = torch.zeros(N, dtype=torch.int32, device="cuda")
        d.saddles_batch_enqueue_to(frames, d_saddles, d_table)
        d.find_boards_enqueue(d_saddles, frame_table=d_table, quads=d_quads, quad_points=d_pts, n_quads=d_n, status=d_st)
        d.decode_quads_enqueue(frames, d_pts, counts=d_n)  # (replaces the find-boards batch without waiting; same stream)
        tags, qst, _ = d.decode_quads_fetch()
        assert not (d_st.cpu().numpy() == PENDING).any()  # (else the chain would need the fetch in between)
        n = d_n.cpu().numpy()
        ref = d.detect_batch_device(frames)
        for f in range(N):
            got = {}
            for i in range(n[f]):
                if qst[f, i] == 0:
                    got[int(tags[f, i]["id"])] = np.array(tags[f, i]["xy"], np.float32).reshape(4, 2)
            assert sorted(got) == sorted(ref[f]) and len(got) >= 30, "frame %d: ids" % f
            for t in got:
                assert bits_equal(got[t], ref[f][t]), "frame %d: corners of tag %d" % (f, t)
    finally:
        d.close()


# ---- 3. the slot map ---------------------------------------------------------------------------------------------------------
def test_refined_records_and_point_statuses_are_read_in_place(det, base):
    import torch
    corners = [np.concatenate([base["gt"][f][t] for t in sorted(base["gt"][f])]).astype(np.float32) for f in range(N)]
    P = 2 * max(len(c) for c in corners)
    points = np.full((N, P, 2), -50.0, np.float32)  # off-image points between the corners, and behind them
    for f in range(N):
        points[f, 0:2 * len(corners[f]):2] = corners[f]
    d_out = torch.zeros((N, P, 5), dtype=torch.float32, device="cuda")
    d_pst = torch.zeros((N, P), dtype=torch.int32, device="cuda")
    det.refine_points_enqueue(base["frames"], dev(points), out=d_out, status=d_pst)
    det.find_boards_enqueue(d_out, point_status=d_pst, quads_per_frame=Q)  # (the refine batch is not fetched)
    quads, pts, n, st = det.find_boards_fetch()
    assert handed_back(det) == (N, 0)
    out, pst = d_out.cpu().numpy(), d_pst.cpu().numpy()
    n_found = 0
    for f in range(N):
        slots = np.flatnonzero(pst[f] == 0)
        assert 0 < len(slots) < P and (slots % 2 == 0).all()
        rq, rst, rn = host(out[f][slots])
        assert (st[f], n[f]) == (rst, rn), f
        if rst == FOUND:
            assert np.array_equal(quads[f, :rn].astype(np.int64), slots[rq.astype(np.int64)]), "frame %d: slot numbers" % f
            assert bits_equal(pts[f, :rn], out[f][:, :2][quads[f, :rn]])
            n_found += 1
    assert n_found >= N // 2


# ---- 4. the limits of the kernel's geometry ----------------------------------------------------------------------------------
def far_saddles(n, seed):
    """Sparse saddles far from any board, their thetas spread over many bins (few per bin)."""
    rng = np.random.default_rng(seed)
    pad = np.zeros((n, 5), np.float32)
    pad[:, 0] = rng.uniform(3000, 9000, n)
    pad[:, 1] = rng.uniform(3000, 9000, n)
    pad[:, 3] = (np.arange(n) % 170 - 85) + 0.25
    return pad


def seed_bin_of(l, k):
    """The list with saddles taken out of its most populated round(theta) bin until that bin holds k."""
    l = l.copy()
    while True:
        bins = np.round(l[:, 3]).astype(int)  # (no theta here is a half-integer: numpy's rounding is the reference's)
        vals, cnt = np.unique(bins, return_counts=True)
        if cnt.max() <= k:
            assert cnt.max() == k
            return l
        l = np.delete(l, np.flatnonzero(bins == vals[cnt.argmax()])[0], axis=0)


def limit_cases(base):
    l0, l1 = base["lists"][0], base["lists"][1]
    assert not (np.abs(l0[:, 3] - np.round(l0[:, 3])) == 0.5).any()
    out = [("length %d" % n, l0[:n]) for n in (1, 3, 4, 63, 64, 65)]
    out += [("length %d" % n, np.concatenate([l0, far_saddles(n - len(l0), n)])) for n in (1023, 1024, 1025)]
    out += [("seed bin of %d" % k, seed_bin_of(l0, k)) for k in (1, 8, 9, 30, 31)]
    shifted = l1.copy()
    shifted[:, 0] += 800.0
    out.append(("two boards", np.concatenate([l0, shifted])))
    return out


def test_limits_of_the_kernels_geometry(det, base):
    import torch
    cs = limit_cases(base)
    S = max(len(l) for _, l in cs)
    batch = np.full((len(cs), S, 5), np.nan, np.float32)
    for i, (_, l) in enumerate(cs):
        batch[i, :len(l)] = l
    counts = np.array([len(l) for _, l in cs], np.int32)
    d_quads = torch.full((len(cs), Q, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(len(cs), dtype=torch.int32, device="cuda")
    d_st = torch.zeros(len(cs), dtype=torch.int32, device="cuda")
    det.find_boards_enqueue(dev(batch), counts=dev(counts), quads=d_quads, n_quads=d_n, status=d_st)
    det.sync()
    before = d_st.cpu().numpy()
    long_one = [i for i, (w, _) in enumerate(cs) if w == "length 1025"]
    print("statuses before the fetch:", dict(zip([w for w, _ in cs], before.tolist())))
    assert np.flatnonzero(before == PENDING).tolist() == long_one  # more than 1024 listed saddles, and nothing else, is handed back
    det.find_boards_fetch()
    assert handed_back(det) == (len(cs), 1)
    quads, n, st = d_quads.cpu().numpy().view(np.uint32), d_n.cpu().numpy(), d_st.cpu().numpy()
    for i, (what, l) in enumerate(cs):
        ref = host(l)
        check_frame(quads[i], n[i], st[i], ref, what)
        assert (quads[i, n[i] if st[i] == FOUND else 0:] == SENTINEL).all(), what + ": rows beyond the count"
    assert st[-1] == FOUND and n[-1] >= 30, "two boards: one of them"


# ---- 5. hand-back on purpose -------------------------------------------------------------------------------------------------
def test_a_wide_guard_band_hands_frames_back_and_changes_nothing(det, base):
    import torch
    d_quads = torch.full((N, Q, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d_pts = torch.zeros((N, Q, 4, 2), dtype=torch.float32, device="cuda")
    d_n = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_st = torch.zeros(N, dtype=torch.int32, device="cuda")
    det.set_option("tail_debug_band", 20000)  # 20 degrees around 60 / 120: every real board has such an angle
    try:
        det.find_boards_enqueue(base["d_saddles"], frame_table=base["d_table"], quads=d_quads, quad_points=d_pts, n_quads=d_n, status=d_st)
        det.sync()
        before = d_st.cpu().numpy()
        assert (before == PENDING).sum() >= N // 2, before
        assert (d_n.cpu().numpy()[before == PENDING] == 0).all()
        det.find_boards_fetch()
        assert handed_back(det) == (N, int((before == PENDING).sum()))
    finally:
        det.set_option("tail_debug_band", 0)
    quads, pts, n, st = d_quads.cpu().numpy().view(np.uint32), d_pts.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()
    assert not (st == PENDING).any()
    for f in range(N):
        check_frame(quads[f], n[f], st[f], base["ref"][f], "frame %d" % f)
        l = base["lists"][f]
        assert bits_equal(pts[f, :n[f]], np.stack([l[:, 0][quads[f, :n[f]]], l[:, 1][quads[f, :n[f]]]], axis=-1))
        assert (quads[f, n[f]:] == SENTINEL).all()


def test_without_the_device_tail_every_frame_takes_the_host_form(base):
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    try:
        d.set_option("device_tail", 0)
        d.find_boards_enqueue(dev(base["padded"]), counts=dev(base["counts"]), quads_per_frame=Q)
        quads, pts, n, st = d.find_boards_fetch(n_threads=4)
        assert handed_back(d) == (N, N)
        for f in range(N):
            check_frame(quads[f], n[f], st[f], base["ref"][f], "frame %d" % f)
    finally:
        d.close()


# ---- 6. statuses and layouts -------------------------------------------------------------------------------------------------
def test_statuses_counts_strides_and_output_modes(det, base):
    import torch
    S = base["padded"].shape[1]
    wide = np.full((N, S, 7), np.nan, np.float32)  # a padded stride: 28 bytes
    wide[:, :, :5] = base["padded"]
    counts = base["counts"].copy()
    counts[1] = 0                      # NONE: an empty list
    counts[2] = S + 1000               # above saddles_per_frame: S slots, of which the last are NaN -> INPUT
    wide[3, 5, 3] = np.inf             # INPUT: a theta
    wide[4, :, 2] = np.nan             # k and phi are never read
    wide[4, :, 4] = np.inf
    want = [base["ref"][f] for f in range(N)]
    want[1] = (None, NONE, 0)
    want[2] = (None, INPUT, 0)
    want[3] = (None, INPUT, 0)
    # internal buffers
    det.find_boards_enqueue(dev(wide), counts=dev(counts), quads_per_frame=Q)
    quads, pts, n, st = det.find_boards_fetch()
    assert handed_back(det) == (N, 0)
    for f in range(N):
        check_frame(quads[f], n[f], st[f], want[f], "internal, frame %d" % f)
    # caller-owned arrays, without quad points; rows beyond a frame's count keep the sentinel
    d_quads = torch.full((N, Q, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d_n = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
    det.find_boards_enqueue(dev(wide), counts=dev(counts), quads=d_quads, n_quads=d_n, status=d_st)
    assert det.find_boards_fetch()[1] is None
    q2, n2, st2 = d_quads.cpu().numpy().view(np.uint32), d_n.cpu().numpy(), d_st.cpu().numpy()
    assert np.array_equal(n2, n) and np.array_equal(st2, st)
    for f in range(N):
        assert np.array_equal(q2[f, :n[f]], quads[f, :n[f]]) and (q2[f, n[f]:] == SENTINEL).all(), f
    # one row short: the true count, no row
    short = int(n[0]) - 1
    d_q3 = torch.full((N, short, 4), SENTINEL, dtype=torch.int32, device="cuda")
    det.find_boards_enqueue(dev(wide), counts=dev(counts), quads=d_q3, n_quads=d_n, status=d_st)
    det.find_boards_fetch()
    q3, n3, st3 = d_q3.cpu().numpy().view(np.uint32), d_n.cpu().numpy(), d_st.cpu().numpy()
    for f in range(N):
        if want[f][1] == FOUND and want[f][2] > short:
            assert (st3[f], n3[f]) == (CAPACITY, want[f][2]) and (q3[f] == SENTINEL).all(), f
        else:
            check_frame(q3[f], n3[f], st3[f], want[f], "short rows, frame %d" % f)
    # a frame-table entry with an overflow bit: nothing of the frame is read
    table = base["d_table"].clone()
    table[5, 2] = 4
    table[5, 1] = 0x7FFFFFF0  # (an offset that must not be followed)
    det.find_boards_enqueue(base["d_saddles"], frame_table=table, quads_per_frame=Q)
    _, _, n4, st4 = det.find_boards_fetch()
    assert (st4[5], n4[5]) == (INPUT, 0) and (np.delete(st4, 5) == FOUND).all()
    # such an entry through the host form: with option device_tail 0 the kernel reads no table and hands every frame back.  Two
    # lattices back to back in one flat array and a third entry with an overflow bit, with and without the device tail
    import aprilgrid_rs_amd as A
    from tests import board_cases as BC
    l7, l9 = BC.lattice(7, 7), BC.lattice(9, 9)
    flat = np.concatenate([np.zeros((3, 5), np.float32), l7, l9])
    small = np.array([[49, 3, 0, 0], [81, 52, 0, 0], [49, 3, 2, 0]], np.int32)
    w7, w9 = host(l7), host(l9)
    assert w7[1] == FOUND and w9[1] == FOUND

    def table_pass(d, host_only):
        i32 = dict(dtype=torch.int32, device="cuda")
        out = dict(quads=torch.full((3, Q, 4), SENTINEL, **i32), quad_points=torch.full((3, Q, 4, 2), -7.0, dtype=torch.float32, device="cuda"),
                   n_quads=torch.full((3,), SENTINEL, **i32), status=torch.full((3,), SENTINEL, **i32))
        d.find_boards_enqueue(dev(flat), frame_table=dev(small), **out)
        d.sync()
        if host_only:
            assert (out["status"].cpu().numpy() == PENDING).all()
        d.find_boards_fetch()
        res = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.float32).copy() for k, v in out.items()}
        assert list(res["status"]) == [FOUND, FOUND, INPUT] and list(res["n_quads"]) == [w7[2], w9[2], 0]
        assert res["quads"][0, :w7[2]].tobytes() == w7[0].tobytes() and res["quads"][1, :w9[2]].tobytes() == w9[0].tobytes()
        assert (res["quads"][2] == SENTINEL).all() and (res["quad_points"][2] == np.float32(-7.0)).all()
        return res

    first = table_pass(det, False)
    d0 = A.TagDetector("t36h11", None, device=0)
    try:
        d0.set_option("device_tail", 0)
        second = table_pass(d0, True)
        assert handed_back(d0) == (3, 3)
    finally:
        d0.close()
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)


def test_state_and_argument_rules(det, base):
    import torch
    import aprilgrid_rs_amd as A
    lib, h = det._lib, det._h
    quads, n, st = np.zeros((N, Q, 4), np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    fetch = lambda: lib.agx_find_boards_fetch(h, quads.ctypes.data, None, n.ctypes.data, st.ctypes.data, 0)
    enqueue = lambda: det.find_boards_enqueue(base["d_saddles"], frame_table=base["d_table"], quads_per_frame=Q)
    det.sync()
    enqueue()
    det.find_boards_fetch()
    assert fetch() == AGX_ERR_STATE  # a second fetch
    fresh = A.TagDetector("t36h11", None, device=0)
    try:
        assert fresh._lib.agx_find_boards_fetch(fresh._h, quads.ctypes.data, None, n.ctypes.data, st.ctypes.data, 0) == AGX_ERR_STATE
    finally:
        fresh.close()
    # the other four kinds' fetches on a find-boards batch leave it in flight
    enqueue()
    buf = np.zeros(N * Q * 16, np.uint64)
    cnt, fst = np.zeros(N, np.uint32), np.zeros(N, np.int32)
    assert lib.agx_saddles_batch_fetch(h, None, 0, cnt.ctypes.data, fst.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_detect_batch_fetch(h, buf.ctypes.data, cnt.ctypes.data, fst.ctypes.data, 1) == AGX_ERR_STATE
    assert lib.agx_refine_points_fetch(h, buf.ctypes.data, buf.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_decode_quads_fetch(h, buf.ctypes.data, buf.ctypes.data, None) == AGX_ERR_STATE
    assert lib.agx_find_boards_fetch(h, None, None, n.ctypes.data, st.ctypes.data, 0) == AGX_ERR_ARG  # internal buffers need the arrays
    assert fetch() == AGX_OK
    for f in range(N):
        check_frame(quads[f], n[f], st[f], base["ref"][f], "after the refused fetches, frame %d" % f)
    # a find-boards fetch on each of the other kinds
    det.saddles_batch_enqueue(base["frames"])
    assert fetch() == AGX_ERR_STATE
    det.saddles_batch_fetch()
    det.detect_batch_enqueue(base["frames"])
    assert fetch() == AGX_ERR_STATE
    det.detect_batch_fetch()
    det.refine_points_enqueue(base["frames"], dev(np.full((N, 4, 2), 100.0, np.float32)))
    assert fetch() == AGX_ERR_STATE
    det.refine_points_fetch()
    det.decode_quads_enqueue(base["frames"], dev(np.full((N, 1, 4, 2), 100.0, np.float32)))
    assert fetch() == AGX_ERR_STATE
    det.decode_quads_fetch()
    # arguments
    s, t = base["d_saddles"].data_ptr(), base["d_table"].data_ptr()
    c = torch.zeros(N, dtype=torch.int32, device="cuda").data_ptr()
    o = torch.zeros((N, Q, 4), dtype=torch.int32, device="cuda")
    enq = lambda sad=s, stride=20, spf=1024, counts=None, table=t, qpf=Q, dq=None, dn=None, ds=None: lib.agx_find_boards_enqueue(
        h, sad, stride, N, spf, counts, table, None, qpf, dq, None, dn, ds)
    assert enq(sad=None) == AGX_ERR_ARG
    for stride in (0, 16, 22, 8):
        assert enq(stride=stride) == AGX_ERR_ARG
    assert enq(spf=0) == AGX_ERR_ARG and enq(qpf=0) == AGX_ERR_ARG
    assert enq(counts=c) == AGX_ERR_ARG  # both counts and a frame table
    assert enq(dq=o.data_ptr()) == AGX_ERR_ARG and enq(dn=c, ds=c) == AGX_ERR_ARG and enq(dq=o.data_ptr(), dn=c) == AGX_ERR_ARG
    assert fetch() == AGX_ERR_STATE  # (a refused enqueue leaves nothing in flight)


# ---- 7. stream and handle state ----------------------------------------------------------------------------------------------
def run_to_device(det, base):
    import torch
    out = (torch.full((N, Q, 4), SENTINEL, dtype=torch.int32, device="cuda"), torch.zeros((N, Q, 4, 2), dtype=torch.float32, device="cuda"),
           torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"))
    det.find_boards_enqueue(base["d_saddles"], frame_table=base["d_table"], quads=out[0], quad_points=out[1], n_quads=out[2], status=out[3])
    return out


def test_on_a_callers_stream_with_an_event_behind_it(det, base):
    import torch
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        out = run_to_device(det, base)  # (follows torch's current stream: s)
        ev = torch.cuda.Event()
        ev.record(s)
    ev.synchronize()  # no frame is handed back here: the results are final behind the event, without a fetch
    quads, n, st = out[0].cpu().numpy().view(np.uint32), out[2].cpu().numpy(), out[3].cpu().numpy()
    for f in range(N):
        check_frame(quads[f], n[f], st[f], base["ref"][f], "frame %d" % f)
    det.find_boards_fetch()
    torch.cuda.current_stream().synchronize()


def test_the_same_batch_twice_gives_the_same_bytes(det, base):
    a = run_to_device(det, base)
    det.find_boards_fetch()
    b = run_to_device(det, base)
    det.find_boards_fetch()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_detect_behind_a_find_boards_batch_equals_a_fresh_handle(det, base):
    import aprilgrid_rs_amd as A
    from tests.util import check_tags
    run_to_device(det, base)  # (not fetched: the detect batch replaces it)
    got = det.detect_batch_device(base["frames"])
    fresh = A.TagDetector("t36h11", None, device=0)
    try:
        ref = fresh.detect_batch_device(base["frames"])
    finally:
        fresh.close()
    for f in range(N):
        check_tags(got[f], ref[f], "frame %d" % f)
        assert len(ref[f]) >= 30


# ---- 8. guard bytes ----------------------------------------------------------------------------------------------------------
def guard_child():
    """Runs in a child process with AGX_REDZONE_BYTES set: internal buffers at the longest lists, a hand-back, the host list."""
    import aprilgrid_rs_amd as A
    synth = synth_module()
    d = A.TagDetector("t36h11", None, device=0)
    before = d.debug_fetch(0, "redzones")["buffers"]
    frame = synth.render_frame(cases.GPU_FIRST, W, H)[0].numpy()
    l0 = d.refined_saddle_points(frame, as_array=True).view(np.float32).reshape(-1, 5)
    ls = [l0, np.concatenate([l0, far_saddles(1024 - len(l0), 1)]), np.concatenate([l0, far_saddles(1025 - len(l0), 2)]), l0[:1]]
    batch = np.full((len(ls), 1025, 5), np.nan, np.float32)
    for i, l in enumerate(ls):
        batch[i, :len(l)] = l
    d.find_boards_enqueue(dev(batch), counts=dev(np.array([len(l) for l in ls], np.int32)), quads_per_frame=Q)
    quads, pts, n, st = d.find_boards_fetch()
    for i, l in enumerate(ls):
        check_frame(quads[i], n[i], st[i], host(l), "guarded, list %d" % i)
    q, s, nq = d.find_board(l0, cap=Q)
    check_frame(q, nq, s, host(l0), "guarded host list")
    r = d.debug_fetch(0, "redzones")
    d.close()
    print("GUARDS buffers_before=%d buffers=%d damaged=%d" % (before, r["buffers"], r["damaged_bytes"]))


def test_guard_bytes_stay_intact_in_a_child_process():
    env = dict(os.environ, AGX_REDZONE_BYTES=str(1 << 16))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests import test_gpu_find_boards as t; t.guard_child()" % ROOT],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("GUARDS")][-1]
    v = dict(kv.split("=") for kv in line.split()[1:])
    assert int(v["damaged"]) == 0, line
    # the code list and the new side buffers (quads, points, counts, statuses, the host list)
    assert int(v["buffers"]) - int(v["buffers_before"]) >= 6, line
