"""agx_clusters_enqueue / agx_clusters_fetch / agx_cluster_centers and agx_filter_saddles_enqueue on the GPU.

The yardstick of the cluster rows is the oracle (tests/cluster_cases.py: orc_min_response, orc_cluster_centers), bit for bit; of
the staged chain -- planes, clusters, refine on the blur plane, filter, find boards, decode, with nothing but the stream between
the stages -- the fused chain (agx_saddles_batch_fetch) and detect (agx_detect_batch) of the same handle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cluster_cases as K
from tests.test_cluster_cases_cpu import FILTERED, filter_cases, filter_reference
from tests.util import ANGLE_TOL_DEG, ROOT, bits_equal, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
SENT = 0x7E7E7E7E
SENT_F = 123456.0
CPF = 64  # rows per frame: the fullest plane has 24 clusters
SW, SH = 320, 240


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(n, cpf):
    import torch
    return (torch.full((n, cpf, 4), SENT, dtype=torch.int32, device="cuda"), torch.full((n, cpf, 2), SENT_F, dtype=torch.float32, device="cuda"),
            torch.full((n,), SENT, dtype=torch.int32, device="cuda"), torch.full((n,), SENT, dtype=torch.int32, device="cuda"))


def as_rows(t):
    a = t.cpu().numpy().view(np.uint32)
    return a.view(K.CLUSTER_DTYPE).reshape(a.shape[0], a.shape[1])


def run_caller_owned(det, planes, cpf=CPF):
    """-> (rows [n, cpf] CLUSTER_DTYPE, points [n, cpf, 2], counts, status) from caller-owned device arrays."""
    o = outputs(planes.shape[0], cpf)
    det.clusters_enqueue(planes, clusters=o[0], points=o[1], counts=o[2], status=o[3])
    got = det.clusters_fetch()
    assert got[0] is o[0]
    return as_rows(o[0]), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32), o[3].cpu().numpy().view(np.uint32)


def check(names, rows, pts, counts, status, cpf=CPF, sent_rows=True):
    for f, name in enumerate(names):
        want, wst = K.expected(name)
        assert int(status[f]) == wst, "%s: status %d" % (name, status[f])
        assert int(counts[f]) == len(want), "%s: count %d, oracle %d" % (name, counts[f], len(want))
        n = len(want)
        assert rows[f, :n].tobytes() == want.tobytes(), "%s: rows differ from the oracle's" % name
        if pts is not None:
            assert bits_equal(pts[f, :n, 0], want["cx"]) and bits_equal(pts[f, :n, 1], want["cy"]), name + ": points"
            if sent_rows:
                assert (pts[f, n:] == np.float32(SENT_F)).all(), name + ": a point beyond the count was written"
        if sent_rows:
            assert (rows[f, n:].view(np.uint32) == SENT).all(), name + ": a row beyond the count was written"


# ---- 1. the hand-built planes against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("names", K.BATCHES, ids=["+".join(b) for b in K.BATCHES])
def test_rows_counts_and_statuses_equal_the_oracles(det, names):
    planes = dev(K.batch(names))
    check(names, *run_caller_owned(det, planes))
    # internal buffers + fetch: rows beyond a frame's count stay as the fetch found them
    det.clusters_enqueue(planes, clusters_per_frame=CPF)
    rows, pts, counts, status = det.clusters_fetch()
    check(names, rows, pts, counts, status, sent_rows=False)
    for f, name in enumerate(names):
        n = len(K.expected(name)[0])
        assert (rows[f, n:].view(np.uint32) == 0xFFFFFFFF).all() and np.isnan(pts[f, n:]).all()
    if "border" in names:  # the refused frame and its neighbours
        f = names.index("border")
        assert status[f] == K.BORDER and counts[f] == 0
        assert all(status[g] == K.OK for g in range(len(names)) if g != f) and counts[names.index("beyond")] == 4


def test_padded_strides_are_never_read(det):
    import torch
    for names in K.BATCHES:
        big = torch.full((3, K.H + 3, K.W + 7), -1e30, dtype=torch.float32, device="cuda")
        view = big[:, :K.H, :K.W]
        view.copy_(dev(K.batch(names)))
        assert view.stride(1) == K.W + 7 and view.stride(0) == (K.H + 3) * (K.W + 7)
        check(names, *run_caller_owned(det, view))


def test_one_row_short_is_capacity_with_the_true_count_and_no_row(det):
    names = K.BATCHES[0]
    n_small, n_wide = len(K.expected("small")[0]), len(K.expected("wide")[0])
    assert n_small > n_wide + 1
    rows, pts, counts, status = run_caller_owned(det, dev(K.batch(names)), cpf=n_small - 1)
    assert status[0] == K.CAPACITY and counts[0] == n_small
    assert (rows[0].view(np.uint32) == SENT).all() and (pts[0] == np.float32(SENT_F)).all()
    check(names[1:], rows[1:], pts[1:], counts[1:], status[1:], cpf=n_small - 1)
    rows, pts, counts, status = run_caller_owned(det, dev(K.batch(names)), cpf=n_small)  # exactly enough
    check(names, rows, pts, counts, status, cpf=n_small)


def test_force_generic_gives_the_same_bytes(det):
    for names in K.BATCHES:
        planes = dev(K.batch(names))
        a = run_caller_owned(det, planes)
        det.set_option("force_generic", 1)
        try:
            b = run_caller_owned(det, planes)
        finally:
            det.set_option("force_generic", 0)
        check(names, *b)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_host_form_and_small_frames(det):
    for name in K.CASES:
        want, wst = K.expected(name)
        rows, status, n = det.cluster_centers(K.CASES[name](), cap=CPF)
        assert (status, n) == (wst, len(want)) and rows.tobytes() == want.tobytes(), name
    plane = K.CASES["small"]()
    padded = np.full((K.H, K.W + 5), -1e30, np.float32)
    padded[:, :K.W] = plane
    rows, status, n = det.cluster_centers(padded[:, :K.W], cap=CPF)  # a strided host plane
    assert status == K.OK and rows.tobytes() == K.expected("small")[0].tobytes()
    rows, status, n = det.cluster_centers(plane, cap=3)
    assert status == K.CAPACITY and n == len(K.expected("small")[0]) and len(rows) == 0
    # odd sizes: no multiple of 64 / 32, a single word row, no interior at all
    rng = np.random.RandomState(11)
    for h, w in ((33, 65), (7, 131), (3, 3), (2, 9), (9, 2), (2, 2)):
        p = np.zeros((h, w), np.float32)
        if h >= 3 and w >= 3:
            inner = np.where(rng.rand(h - 2, w - 2) < 0.3, -10.0, 0.0).astype(np.float32)
            inner[0, 0] = -100.0
            p[1:-1, 1:-1] = inner
        else:
            p[:] = -1.0  # all ring, all at the minimum: no seed, no cluster, not refused
        want, wst = K.expected_of(p)
        rows, status, n = det.cluster_centers(p, cap=1024)
        assert (status, n) == (wst, len(want)) and rows.tobytes() == want.tobytes(), (h, w)
        assert wst == K.OK and (len(want) > 0) == (h >= 3 and w >= 3)


def dotted_plane(n):
    """512 x 384 (cap_roots = plane / 8 = 24576 clusters fit the workspace) with n components of one pixel, every fifth of
    two, none touching another or the ring: x = 1, 4, .., 508 (170 a row), y = 1, 3, .."""
    w, h, per_row = 512, 384, 170
    assert n <= per_row * ((h - 2) // 2)
    p = np.zeros((h, w), np.float32)
    i = np.arange(n)
    x, y = 1 + 3 * (i % per_row), 1 + 2 * (i // per_row)
    p[y, x] = -10.0
    p[y[::5], x[::5] + 1] = -20.0
    p[y[-1], x[-1]] = -100.0  # the minimum in the last component: thr = -5
    return p


def test_the_most_rows_a_frame_can_have(det):
    """clusters_per_frame = 16384: 64 KB of LDS and a 16384-key sort.  One frame fills every row, one has a cluster more
    (AGX_CLUSTERS_CAPACITY, the true count, no row), one has few."""
    top = 16384
    planes = np.stack([dotted_plane(top), dotted_plane(top + 1), dotted_plane(7)])
    want = [K.expected_of(p) for p in planes]
    assert [len(r) for r, _ in want] == [top, top + 1, 7] and all(s == K.OK for _, s in want)
    rows, pts, counts, status = run_caller_owned(det, dev(planes), cpf=top)
    assert list(status) == [K.OK, K.CAPACITY, K.OK] and list(counts) == [top, top + 1, 7]
    assert (rows[1].view(np.uint32) == SENT).all() and (pts[1] == np.float32(SENT_F)).all()
    for f in (0, 2):
        r, n = want[f][0], len(want[f][0])
        assert rows[f, :n].tobytes() == r.tobytes(), "frame %d: rows differ from the oracle's" % f
        assert bits_equal(pts[f, :n, 0], r["cx"]) and bits_equal(pts[f, :n, 1], r["cy"])
        assert (rows[f, n:].view(np.uint32) == SENT).all() and (pts[f, n:] == np.float32(SENT_F)).all()
    # the host form at its default cap, through internal buffers
    r, st, n = det.cluster_centers(planes[0])
    assert (st, n) == (K.OK, top) and r.tobytes() == want[0][0].tobytes()
    r, st, n = det.cluster_centers(planes[1])
    assert (st, n) == (K.CAPACITY, top + 1) and len(r) == 0


def test_fetch_copies_points_from_where_the_batch_wrote_them(det):
    """Internal rows, counts and statuses with a caller's d_points, and host `points` at the fetch: they are this batch's, read
    from the caller's array -- not what an earlier, smaller batch left in the handle's own points buffer."""
    import torch
    lib, h = det._lib, det._h
    det.clusters_enqueue(dev(K.batch(("wide",))), clusters_per_frame=8)  # one frame of 8 slots through the internal buffers
    det.clusters_fetch()
    names = K.BATCHES[0]
    planes = dev(K.batch(names))
    n = len(names)
    d_pts = torch.full((n, CPF, 2), SENT_F, dtype=torch.float32, device="cuda")
    assert lib.agx_clusters_enqueue(h, planes.data_ptr(), n, K.W, K.H, 4 * K.W, 4 * K.W * K.H, CPF, None, d_pts.data_ptr(), None, None) == AGX_OK
    h_rows, h_counts, h_status = np.zeros((n, CPF), K.CLUSTER_DTYPE), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    h_pts = np.full((n, CPF, 2), SENT_F, np.float32)
    assert lib.agx_clusters_fetch(h, h_rows.ctypes.data, h_pts.ctypes.data, h_counts.ctypes.data, h_status.ctypes.data) == AGX_OK
    check(names, h_rows, h_pts, h_counts, h_status, sent_rows=False)
    assert h_pts.tobytes() == d_pts.cpu().numpy().tobytes()  # (beyond the counts: the sentinel in both)
    # and without d_points: the handle's own, of this batch
    assert lib.agx_clusters_enqueue(h, planes.data_ptr(), n, K.W, K.H, 4 * K.W, 4 * K.W * K.H, CPF, None, None, None, None) == AGX_OK
    h_pts2 = np.full((n, CPF, 2), SENT_F, np.float32)
    assert lib.agx_clusters_fetch(h, h_rows.ctypes.data, h_pts2.ctypes.data, h_counts.ctypes.data, h_status.ctypes.data) == AGX_OK
    assert h_pts2.tobytes() == h_pts.tobytes()


# ---- 1b. coordinate sums at 2^24 and beyond 2^32 ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    d.set_limits(max_candidates=K.WIDE_CANDIDATES)  # (the largest plane is one component of 741 412 pixels: more than half a plane)
    yield d
    d.close()


@pytest.mark.parametrize("name", sorted(K.WIDE_CASES))
def test_centres_are_the_quotients_of_the_exact_integer_sums(wide_det, name):
    """First index and size are the oracle's, the centre is f32(exact integer sum) / f32(size) -- the oracle's own below 2^24 --
    and AGX_CLUSTERS_INEXACT is set from 2^24 on and not below; the small cluster beside the large one has the oracle's centre.
    Caller-owned arrays, the same under force_generic, and the host form agx_cluster_centers."""
    want, wst, sums = K.wide_expected(name)
    plane = K.WIDE_CASES[name]()
    planes = dev(plane[None])
    got = []
    for generic in (0, 1):
        wide_det.set_option("force_generic", generic)
        try:
            rows, pts, counts, status = run_caller_owned(wide_det, planes, cpf=8)
        finally:
            wide_det.set_option("force_generic", 0)
        what = "%s, force_generic %d" % (name, generic)
        assert int(status[0]) == wst, "%s: status %#x, expected %#x" % (what, status[0], wst)
        assert int(counts[0]) == len(want) == 2
        assert rows[0, :2].tobytes() == want.tobytes(), "%s: rows %s, expected %s" % (what, rows[0, :2], want)
        assert bits_equal(pts[0, :2, 0], want["cx"]) and bits_equal(pts[0, :2, 1], want["cy"])
        assert (rows[0, 2:].view(np.uint32) == SENT).all() and (pts[0, 2:] == np.float32(SENT_F)).all()
        got.append(rows.tobytes() + status.tobytes())
    assert got[0] == got[1]
    r, st, n = wide_det.cluster_centers(plane, cap=8)
    assert (st, n) == (wst, 2) and r.tobytes() == want.tobytes(), name + ": the host form"


# ---- 2. behind agx_planes_enqueue: the fused chain's cluster table, saddles and tags -----------------------------------------
@pytest.fixture(scope="module")
def boards():
    synth = synth_module()
    frames, _ = synth.render_batch(40, 2, SW, SH, device="cuda")
    return frames


def staged(d, frames, sigma, cpf=4096):
    """planes -> clusters -> refine on the blur plane -> filter, stream-ordered, no sync and no host copy in between.
    -> the device tensors (resp, blur, rows, pts, counts, cstatus, records, pstatus)."""
    import torch
    n = frames.shape[0]
    blur = torch.empty((n, SH, SW), dtype=torch.float32, device="cuda")
    resp = torch.empty_like(blur)
    rows, pts, counts, cstatus = outputs(n, cpf)
    records = torch.zeros((n, cpf, 5), dtype=torch.float32, device="cuda")
    pstatus = torch.full((n, cpf), SENT, dtype=torch.int32, device="cuda")
    d.planes_enqueue(frames, sigma, blur=blur, response=resp)
    d.clusters_enqueue(resp, clusters=rows, points=pts, counts=counts, status=cstatus)
    d.refine_points_enqueue(blur, pts, counts=counts, out=records, status=pstatus, image="plane")
    d.filter_saddles_enqueue(records, pstatus, counts=counts)
    return resp, blur, rows, pts, counts, cstatus, records, pstatus


@pytest.mark.parametrize("sigma", [1.5, 2.5])
def test_staged_chain_equals_the_fused_chain(boards, sigma):
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import SADDLE_DTYPE
    d = A.TagDetector("t36h11", None, device=0, blur_sigma=sigma)
    try:
        resp, blur, rows, pts, counts, cstatus, records, pstatus = staged(d, boards, sigma)
        d.sync()
        rows, counts, cstatus = as_rows(rows), counts.cpu().numpy(), cstatus.cpu().numpy()
        records, pstatus = records.cpu().numpy(), pstatus.cpu().numpy().view(np.uint32)
        d.saddles_batch_enqueue(boards)
        fused, st = d.saddles_batch_fetch()
        assert (st == 0).all() and (cstatus == K.OK).all()
        for f in range(boards.shape[0]):
            centers = d.debug_fetch(f, "centers")
            assert counts[f] == len(centers) > 50 and rows[f, :counts[f]].tobytes() == centers.tobytes(), "frame %d: cluster rows" % f
            assert (pstatus[f, counts[f]:] == SENT).all()
            keep = pstatus[f, :counts[f]] == 0
            assert (pstatus[f, :counts[f]] == FILTERED).any()
            got = records[f, :counts[f]][keep]
            ref = fused[f]
            assert len(got) == len(ref) > 30, "frame %d: %d survivors, the chain %d" % (f, len(got), len(ref))
            for i, name in enumerate(("x", "y", "k")):
                assert bits_equal(got[:, i], ref[name]), "frame %d: %s" % (f, name)
            for i, name in ((3, "theta"), (4, "phi")):
                assert np.max(np.abs(got[:, i] - ref[name])) <= ANGLE_TOL_DEG, (f, name)
            # the oracle's clusters of the response plane as the device wrote it
            want, wst = K.expected_of(resp[f].cpu().numpy())
            assert wst == K.OK and rows[f, :counts[f]].tobytes() == want.tobytes(), "frame %d against the oracle" % f
    finally:
        d.close()


def test_staged_detect_equals_detect_batch(boards):
    import torch
    import aprilgrid_rs_amd as A
    prm = A.DetectorParams.default_params()
    prm.max_num_of_boards = 1
    d = A.TagDetector("t36h11", prm, device=0)
    Q = 64
    try:
        n = boards.shape[0]
        _, _, _, _, counts, _, records, pstatus = staged(d, boards, 1.5)
        quads = torch.zeros((n, Q, 4), dtype=torch.int32, device="cuda")
        qpts = torch.zeros((n, Q, 4, 2), dtype=torch.float32, device="cuda")
        nq = torch.zeros(n, dtype=torch.int32, device="cuda")
        bst = torch.zeros(n, dtype=torch.int32, device="cuda")
        d.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
        d.decode_quads_enqueue(boards, qpts, counts=nq)
        tags, qst, _ = d.decode_quads_fetch()
        assert not (bst.cpu().numpy() == 4).any()  # (AGX_BOARD_PENDING: the chain would need the fetch in between)
        nq = nq.cpu().numpy()
        ref = d.detect_batch(boards.cpu().numpy())
        for f in range(n):
            got = {}
            for i in range(nq[f]):
                if qst[f, i] == 0:
                    got[int(tags[f, i]["id"])] = np.array(tags[f, i]["xy"], np.float32).reshape(4, 2)
            # (the board need not lie inside a 320 x 240 frame as a whole; more than one quad's worth of tags shows the stages ran)
            assert sorted(got) == sorted(ref[f]) and len(got) > 4, "frame %d: ids %d vs %d" % (f, len(got), len(ref[f]))
            for t in got:
                assert bits_equal(got[t], ref[f][t]), "frame %d: corners of tag %d" % (f, t)
    finally:
        d.close()


def test_both_exact_fronts_and_the_fused_front_alternate_on_one_handle():
    """agx_clusters_enqueue (k_plane_front), a chain batch at sigma 2.0 (k_response_front) and one at sigma 1.5 (K1) take turns on
    one handle and one mask: every word of the image area is written in every batch ("Two fronts, one contract"), so
    no batch sees a bit of the one before.  70 x 40: two waves across with a partial second, two word rows with a partial second.
    The planes are another image's responses than the chain's frames: a word left unwritten would hold foreign bits."""
    import aprilgrid_rs_amd as A
    from tests import sigma_oracle
    from tests.util import check_saddles
    w, h = 70, 40
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(11)
    def board(dx, dy):
        return (((x + dx) // 6 + (y + dy) // 6) % 2 * 180 + 30 + rng.integers(0, 8, (h, w))).astype(np.uint8)
    frames = np.stack([board(0, 0), board(1, 1)])
    others = [board(3, 3), board(5, 2)]
    planes = np.stack([sigma_oracle.refined_saddle_points(f, 2.0)[1]["resp"] for f in others])
    want = [K.expected_of(p) for p in planes]
    refs = {sg: [sigma_oracle.refined_saddle_points(f, sg) for f in frames] for sg in (2.0, 1.5)}
    for rows, st in want:  # premise: clusters in the second wave's columns and in the second word row
        assert st == K.OK and (rows["cx"] >= 64).any() and (rows["cy"] >= 32).any() and len(rows) >= 8
    for sg in refs:
        for ref, dbg in refs[sg]:
            assert len(ref) >= 4 and (dbg["centers"][:, 0] >= 64).any() and (dbg["centers"][:, 1] >= 32).any(), "premise"
    d = A.TagDetector("t36h11", None, device=0)
    try:
        d_planes, d_frames = dev(planes), dev(frames)
        for turn in range(2):
            rows, pts, counts, status = run_caller_owned(d, d_planes, cpf=128)  # (84 and 72 clusters)
            for f, (wr, wst) in enumerate(want):
                assert status[f] == wst and counts[f] == len(wr) and rows[f, :len(wr)].tobytes() == wr.tobytes(), "turn %d: plane %d" % (turn, f)
            for sg, front in ((2.0, 1), (1.5, 0)):
                d.set_blur_sigma(sg)
                d.saddles_batch_enqueue(d_frames)
                res, st = d.saddles_batch_fetch()
                assert (st == 0).all() and d.get_option("last_chain_front") == front
                for f in range(2):
                    check_saddles(res[f], refs[sg][f][0], "turn %d: sigma %g frame %d" % (turn, sg, f))
    finally:
        d.close()


# ---- 3. the filter ----------------------------------------------------------------------------------------------------------
def test_filter_edges_counts_and_the_host_form(det):
    import aprilgrid_rs_amd as A
    cs = filter_cases()
    P = max(len(r) for r, _ in cs) + 5
    n = len(cs) + 1
    records = np.zeros((n, P, 5), np.float32)
    status = np.full((n, P), SENT, np.uint32)
    counts = np.zeros(n, np.int32)
    for f, (r, s) in enumerate(cs):
        records[f, :len(r)], status[f, :len(s)], counts[f] = r, s, len(r)
    # the last frame: the first case again with a count that cuts off its largest k; what lies beyond the count is not read
    r, s = cs[0]
    records[-1, :len(r)], status[-1, :len(s)], counts[-1] = r, s, 3
    records[-1, 0, 2] = 0.5
    records[-1, 3, 2] = 1e9
    status[-1, 3] = 0
    d_rec, d_st = dev(records), dev(status.view(np.int32))
    det.filter_saddles_enqueue(d_rec, d_st, counts=dev(counts))
    det.sync()
    got = d_st.cpu().numpy().view(np.uint32)
    assert d_rec.cpu().numpy().tobytes() == records.tobytes()  # records untouched
    for f in range(n):
        c = counts[f]
        want = filter_reference(records[f, :c], status[f, :c])
        assert np.array_equal(got[f, :c], want), "frame %d" % f
        assert np.array_equal(got[f, :c], A.filter_saddles(records[f, :c], status[f, :c])), "frame %d: host form" % f
        assert np.array_equal(got[f, c:], status[f, c:]), "frame %d: a word beyond the count changed" % f
    assert list(got[0, :9]) == [0, 0, FILTERED, 0, 0, FILTERED, FILTERED, FILTERED, FILTERED]  # k == max/10, phi == 30, phi == 60 kept
    assert np.array_equal(got[1], status[1])  # nothing refined: unchanged
    # without counts: every slot
    full = np.concatenate([cs[3][0], cs[3][0][::-1]])[None]
    fst = np.concatenate([cs[3][1], cs[3][1][::-1]])[None]
    d_st = dev(fst.view(np.int32))
    det.filter_saddles_enqueue(dev(full), d_st)
    det.sync()
    assert np.array_equal(d_st.cpu().numpy().view(np.uint32)[0], filter_reference(full[0], fst[0]))


# ---- 4. state and arguments -------------------------------------------------------------------------------------------------
def test_state_and_argument_rules(det):
    import torch
    lib, h = det._lib, det._h
    planes = dev(K.batch(K.BATCHES[0]))
    n = 3
    rows, pts, counts, status = outputs(n, CPF)
    p = planes.data_ptr()
    rs, fs = 4 * K.W, 4 * K.W * K.H
    good = [p, n, K.W, K.H, rs, fs, CPF, rows.data_ptr(), pts.data_ptr(), counts.data_ptr(), status.data_ptr()]
    h_rows, h_counts, h_status = np.zeros((n, CPF), K.CLUSTER_DTYPE), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    fetch = lambda: lib.agx_clusters_fetch(h, h_rows.ctypes.data, None, h_counts.ctypes.data, h_status.ctypes.data)
    frames = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    # every bad argument is AGX_ERR_ARG and leaves the saddle batch in flight where it is
    det.saddles_batch_enqueue(frames)
    bad = {"null plane": {0: None}, "no frames": {1: 0}, "width 1": {2: 1}, "height 1": {3: 1}, "short row stride": {4: rs - 4},
           "odd row stride": {4: rs + 2}, "short frame stride": {5: fs - 4}, "odd frame stride": {5: fs + 2}, "misaligned plane": {0: p + 2},
           "no rows per frame": {6: 0}, "too many rows per frame": {6: 16385}, "rows without counts": {9: None},
           "counts without rows": {7: None}, "status alone missing": {10: None}, "misaligned rows": {7: rows.data_ptr() + 2},
           "misaligned points": {8: pts.data_ptr() + 1}}
    for what, change in bad.items():
        a = list(good)
        for i, v in change.items():
            a[i] = v
        assert lib.agx_clusters_enqueue(h, *a) == AGX_ERR_ARG, what
        assert fetch() == AGX_ERR_STATE and b"agx_saddles_batch_fetch" in lib.agx_last_error(h), what
    assert lib.agx_filter_saddles_enqueue(h, None, status.data_ptr(), n, CPF, None) == AGX_ERR_ARG
    assert lib.agx_filter_saddles_enqueue(h, pts.data_ptr(), status.data_ptr(), 0, CPF, None) == AGX_ERR_ARG
    assert lib.agx_filter_saddles_enqueue(h, pts.data_ptr(), status.data_ptr(), n, 0, None) == AGX_ERR_ARG
    assert lib.agx_filter_saddles_enqueue(h, pts.data_ptr() + 2, status.data_ptr(), n, CPF, None) == AGX_ERR_ARG
    res, st = det.saddles_batch_fetch()  # still there
    assert len(res) == 2 and (st == 0).all()
    # the kind replaces ...
    det.saddles_batch_enqueue(frames)
    assert lib.agx_clusters_enqueue(h, p, n, K.W, K.H, rs, fs, CPF, None, None, None, None) == AGX_OK
    cnt2, st2 = np.zeros(2, np.uint32), np.zeros(2, np.int32)
    sad = np.zeros((2, 8, 5), np.float32)
    assert lib.agx_saddles_batch_fetch(h, sad.ctypes.data, 8, cnt2.ctypes.data, st2.ctypes.data) == AGX_ERR_STATE
    assert b"agx_clusters_fetch" in lib.agx_last_error(h)
    assert lib.agx_refine_points_fetch(h, sad.ctypes.data, cnt2.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_detect_batch_fetch(h, None, cnt2.ctypes.data, st2.ctypes.data, 0) == AGX_ERR_STATE
    assert lib.agx_decode_quads_fetch(h, None, None, None) == AGX_ERR_STATE
    assert lib.agx_find_boards_fetch(h, None, None, None, None, 0) == AGX_ERR_STATE
    assert lib.agx_clusters_fetch(h, None, None, h_counts.ctypes.data, h_status.ctypes.data) == AGX_ERR_ARG  # internal buffers need the arrays
    assert fetch() == AGX_OK and fetch() == AGX_ERR_STATE  # a second fetch
    check(K.BATCHES[0], h_rows, None, h_counts, h_status, sent_rows=False)
    # ... and is replaced
    assert lib.agx_clusters_enqueue(h, *good) == AGX_OK
    det.saddles_batch_enqueue(frames)
    assert fetch() == AGX_ERR_STATE
    det.saddles_batch_fetch()
    assert lib.agx_clusters_enqueue(h, *good) == AGX_OK
    assert lib.agx_filter_saddles_enqueue(h, pts.data_ptr(), status.data_ptr(), n, 1, None) == AGX_OK  # no fetch of its own: nothing in flight
    assert fetch() == AGX_ERR_STATE
    det.sync()
    # caller-owned arrays: the fetch only waits
    assert lib.agx_clusters_enqueue(h, *good) == AGX_OK
    assert lib.agx_clusters_fetch(h, None, None, None, None) == AGX_OK
    check(K.BATCHES[0], as_rows(rows), pts.cpu().numpy(), counts.cpu().numpy().view(np.uint32), status.cpu().numpy().view(np.uint32))
    import aprilgrid_rs_amd as A
    fresh = A.TagDetector("t36h11", None, device=0)
    try:
        assert fresh._lib.agx_clusters_fetch(fresh._h, h_rows.ctypes.data, None, h_counts.ctypes.data, h_status.ctypes.data) == AGX_ERR_STATE
    finally:
        fresh.close()


def test_host_form_refuses_before_it_touches_anything(det):
    import torch
    lib, h = det._lib, det._h
    plane = K.CASES["small"]()
    out, n_out, st = np.zeros(CPF, K.CLUSTER_DTYPE), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    good = [plane.ctypes.data, K.W, K.H, 4 * K.W, out.ctypes.data, CPF, n_out.ctypes.data_as(u32p), st.ctypes.data_as(u32p)]
    frames = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    det.saddles_batch_enqueue(frames)
    bad = {"null plane": {0: None}, "misaligned plane": {0: plane.ctypes.data + 2}, "width 1": {1: 1}, "height 1": {2: 1},
           "short row stride": {3: 4 * K.W - 4}, "odd row stride": {3: 4 * K.W + 2}, "null rows": {4: None}, "no cap": {5: 0},
           "cap too large": {5: 16385}, "null count": {6: None}, "null status": {7: None}}
    for what, change in bad.items():
        a = list(good)
        for i, v in change.items():
            a[i] = v
        assert lib.agx_cluster_centers(h, *a) == AGX_ERR_ARG, what
    res, sst = det.saddles_batch_fetch()  # still in flight
    assert len(res) == 2 and (sst == 0).all()
    assert lib.agx_cluster_centers(h, *good) == AGX_OK and n_out[0] == len(K.expected("small")[0]) and st[0] == K.OK


# ---- 5. HIP graph -----------------------------------------------------------------------------------------------------------
def test_one_graph_replay_after_an_eager_batch():
    import torch
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    names = K.BATCHES[1]
    try:
        planes = dev(K.batch(names))
        o = outputs(3, CPF)
        with torch.cuda.stream(s):
            for _ in range(2):  # workspace, both counter sets, stream binding: all before the capture
                d.clusters_enqueue(planes, clusters=o[0], points=o[1], counts=o[2], status=o[3])
        s.synchronize()
        eager = [t.cpu().numpy().copy() for t in o]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d.clusters_enqueue(planes, clusters=o[0], points=o[1], counts=o[2], status=o[3])
        o[0].fill_(SENT), o[1].fill_(SENT_F), o[2].fill_(SENT), o[3].fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert all(t.cpu().numpy().tobytes() == e.tobytes() for t, e in zip(o, eager))
        check(names, as_rows(o[0]), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32), o[3].cpu().numpy().view(np.uint32))
        del g
    finally:
        torch.cuda.synchronize()
        d.close()


# ---- 6. guard bytes ---------------------------------------------------------------------------------------------------------
def guard_child():
    """Runs in a child process with AGX_REDZONE_BYTES set: the batches above through internal and caller-owned buffers, the
    generic path, the host form, the staged chain and the filter."""
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    before = d.debug_fetch(0, "redzones")["buffers"]
    for names in K.BATCHES:
        planes = dev(K.batch(names))
        check(names, *run_caller_owned(d, planes))
        d.clusters_enqueue(planes, clusters_per_frame=CPF)
        rows, pts, counts, status = d.clusters_fetch()
        check(names, rows, pts, counts, status, sent_rows=False)
        d.set_option("force_generic", 1)
        check(names, *run_caller_owned(d, planes))
        d.set_option("force_generic", 0)
    assert d.cluster_centers(K.CASES["small"](), cap=CPF)[0].tobytes() == K.expected("small")[0].tobytes()
    synth = synth_module()
    frames, _ = synth.render_batch(40, 2, SW, SH, device="cuda")
    staged(d, frames, 1.5)
    d.sync()
    r = d.debug_fetch(0, "redzones")
    d.close()
    print("GUARDS buffers_before=%d buffers=%d damaged=%d" % (before, r["buffers"], r["damaged_bytes"]))


def test_guard_bytes_stay_intact_in_a_child_process():
    env = dict(os.environ, AGX_REDZONE_BYTES=str(1 << 16))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests import test_gpu_clusters as t; t.guard_child()" % ROOT],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("GUARDS")][-1]
    v = dict(kv.split("=") for kv in line.split()[1:])
    assert int(v["damaged"]) == 0, line
    # the workspace and the new side buffers (rows, points, counts, statuses, the host plane)
    assert int(v["buffers"]) - int(v["buffers_before"]) >= 5 + 20, line
