"""agx_snap_points_enqueue (k_snap_points) on the GPU: every output array against the host form agx_snap_points_tail byte for
byte, guard words included (tests/test_snap_points_cpu.py holds the host form to a numpy brute force); the compacted rows as the
seeds of agx_grow_boards_enqueue and agx_init_quads_enqueue with nothing but the stream between; TagDetector.detect_tracked
against detect_batch.  Synthetic lists, no pixels but in the last part."""
import numpy as np
import pytest

from tests import snap_cases as S
from tests.test_find_boards_cpu import GPU_FIRST, GPU_FRAMES, GPU_SIZE, golden_list
from tests.util import bits_equal, synth_module

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = S.SENTINEL
GUARD = 64  # words of SENT in front of and behind every output
CHUNK = 1024  # k_snap_points' LDS chunk (csrc/tail_kernels.h: SNAP_CHUNK)
WAVE_ROWS, PASS_ROWS = 4, 16  # rows a wave / a workgroup answers per pass (SNAP_ROWS_PER_WAVE, x 4 waves)
OVERFLOW = 4  # AGX_FRAME_SADDLE_OVERFLOW


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_list(rng, n, span=300.0):
    s = np.zeros((n, 5), F32)
    s[:, :2] = rng.uniform(0, span, (n, 2)).astype(F32)
    s[:, 2:] = rng.uniform(-50, 50, (n, 3)).astype(F32)
    return s


def points_near(rng, l, rows, ppr, far=0.25):
    """rows x ppr points: most within 1 px of a saddle of l, a share `far` anywhere."""
    pts = rng.uniform(-20, 320, (rows, ppr, 2)).astype(F32)
    if len(l):
        at = rng.integers(0, len(l), (rows, ppr))
        near = l[at, :2] + rng.uniform(-1, 1, (rows, ppr, 2)).astype(F32)
        pts = np.where(rng.uniform(size=(rows, ppr, 1)) < far, pts, near).astype(F32)
    return pts


class Guarded:
    """A device array of uint32 words with GUARD words of SENT on either side, and the host picture of what it must hold."""

    def __init__(self, words):
        self.n = words
        self.t = dev(np.full(words + 2 * GUARD, SENT, np.uint32).view(np.int32))
        self.want = np.full(words + 2 * GUARD, SENT, np.uint32)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def expect(self, at, values):
        v = np.ascontiguousarray(values).reshape(-1).view(np.uint32)
        self.want[GUARD + at:GUARD + at + len(v)] = v

    def same(self):
        return self.t.cpu().numpy().view(np.uint32).tobytes() == self.want.tobytes()


def run(det, lists, points, limit, words=None, flags=0, stride=20, table=None, overflow=(), with_counts=True, tag_table=False, with_dist=True,
        with_index=True, what=""):
    """One batch against the host form.  lists[f] [n_f, 5]; points[f] [R_f, P, 2] (rows_per_frame = the largest R_f, the others by
    d_row_counts); words[f] the status words of frame f or None.  table: a permutation of the frames -- their lists packed in that
    order with gaps, read through d_frame_table; frames in `overflow` carry an overflow bit.  tag_table: the points are handed
    over as agx_tag rows (P = 4)."""
    n, ppr = len(lists), points[0].shape[1]
    R = max(max(len(p) for p in points), 1)
    fl = stride // 4
    if table is None:
        spf = max(max(len(l) for l in lists), 1) + 2
        buf = np.full((n, spf, fl), np.nan, F32)
        w = np.full((n, spf), 7, np.uint32)  # (behind a count: never looked at)
        first = [f * spf for f in range(n)]
        for f, l in enumerate(lists):
            buf[f, :len(l), :5] = l
            w[f, :len(l)] = 0 if words is None or words[f] is None else words[f]
        entries = None
    else:
        first, at = [0] * n, 3
        for f in table:
            first[f] = at
            at += len(lists[f]) + 5
        spf = at
        buf = np.full((spf, fl), np.nan, F32)
        w = np.full(spf, 7, np.uint32)
        entries = np.zeros((n, 4), np.uint32)
        for f, l in enumerate(lists):
            buf[first[f]:first[f] + len(l), :5] = l
            w[first[f]:first[f] + len(l)] = 0 if words is None or words[f] is None else words[f]
            entries[f] = (len(l), first[f], OVERFLOW if f in overflow else 0, 0)
    if tag_table:
        assert ppr == 4
        pbuf = np.zeros((n, R), S.TAG)
        pbuf["xy"] = np.nan
        for f, p in enumerate(points):
            pbuf["xy"][f, :len(p)] = p.reshape(-1, 8)
        d_pts = dev(pbuf.view(np.uint32).reshape(n, R, 9).view(np.int32))
        p_points, row_stride = d_pts.data_ptr() + 4, 36
    else:
        pbuf = np.full((n, R, ppr, 2), np.nan, F32)
        for f, p in enumerate(points):
            pbuf[f, :len(p)] = p
        d_pts = dev(pbuf)
        p_points, row_stride = d_pts.data_ptr(), 8 * ppr
    every_row = all(len(p) == R for p in points)
    d_buf, d_w = dev(buf), dev(w.view(np.int32))
    d_counts = dev(np.array([len(l) for l in lists], np.int32)) if table is None and with_counts else None
    d_table = dev(entries.view(np.int32)) if table is not None else None
    d_rc = None if every_row else dev(np.array([len(p) for p in points], np.int32))
    slots, dist, rows = Guarded(n * R * ppr), Guarded(n * R * ppr), Guarded(n * R * ppr)
    kept, index, status = Guarded(n), Guarded(n * R), Guarded(n)
    for f, (l, p) in enumerate(zip(lists, points)):
        wf = None if words is None else words[f]
        if table is None and not with_counts:  # every slot of the frame is read: the NaN padding is listed unless its word says no
            l = buf[f, :, :5]
            wf = w[f]
        if f in overflow:
            kept.expect(f, np.uint32(0)), status.expect(f, np.uint32(_ffi.AGX_SNAP_INPUT))
            continue
        h = S.Raw(l, p, limit, words=wf, flags=flags)
        assert h.rc == _ffi.AGX_OK
        kept.expect(f, np.uint32(h.kept.value)), status.expect(f, np.uint32(h.status.value))
        if h.status.value != _ffi.AGX_SNAP_OK:
            continue
        k = h.kept.value
        slots.expect(f * R * ppr, h.slots[:len(p) * ppr]), dist.expect(f * R * ppr, h.dist[:len(p) * ppr])
        rows.expect(f * R * ppr, h.rows[:k * ppr]), index.expect(f * R, h.index[:k])
    det._follow_torch_stream(d_buf)
    rc = det._lib.agx_snap_points_enqueue(det._h, d_buf.data_ptr(), stride, n, spf if table is not None else buf.shape[1],
                                          d_counts.data_ptr() if d_counts is not None else None,
                                          d_table.data_ptr() if d_table is not None else None, d_w.data_ptr() if words is not None or not with_counts else None,
                                          p_points, row_stride, 8, R, ppr, d_rc.data_ptr() if d_rc is not None else None, float(limit), flags,
                                          slots.ptr, dist.ptr if with_dist else None, rows.ptr, kept.ptr, index.ptr if with_index else None, status.ptr)
    det._check(rc)
    det.sync()
    for name, g, on in (("slots", slots, True), ("dist_sq", dist, with_dist), ("rows", rows, True), ("n_rows", kept, True),
                        ("row_index", index, with_index), ("status", status, True)):
        if not on:
            g.want[:] = SENT
        assert g.same(), "%s: %s differs from the host form (or a guard word was written)" % (what, name)
    return kept.want[GUARD:GUARD + n], status.want[GUARD:GUARD + n]


# ---- 1. the kernel against the host form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppr", [4, 1, 2, 3])
def test_short_lists_and_row_counts_around_a_waves_share(det, ppr):
    rng = np.random.default_rng(ppr)
    lists = [random_list(rng, n) for n in (0, 1, 63, 64, 65)]
    for row_counts in ((0, 1, WAVE_ROWS - 1, WAVE_ROWS, WAVE_ROWS + 1), (PASS_ROWS - 1, PASS_ROWS, PASS_ROWS + 1, 2 * PASS_ROWS + 1, 7)):
        points = [points_near(rng, l, r, ppr) for l, r in zip(lists, row_counts)]
        for flags in (0, _ffi.AGX_SNAP_REVERSE):
            kept, _ = run(det, lists, points, 2.0, flags=flags, what="ppr %d rows %s flags %d" % (ppr, row_counts, flags))
    assert kept[0] == 0 and kept[1:].sum() > 0
    run(det, lists, points, np.inf, with_dist=False, with_index=False, what="optional outputs absent")
    run(det, lists, [p[:5] for p in points], 2.0, what="no d_row_counts")


def test_lists_around_the_lds_chunk_and_past_the_other_kernels_limit(det):
    rng = np.random.default_rng(11)
    lists = [random_list(rng, n, span=900.0) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 1025, 2 * CHUNK + 77)]
    points = [points_near(rng, l, 21, 4) for l in lists]
    for l, p in zip(lists, points):  # a point whose nearest is the last slot of the list, and one right at the chunk's seam
        p[0, 0] = l[-1, :2] + F32(0.125)
        p[1, 1] = l[min(len(l) - 1, CHUNK), :2] - F32(0.125)
    words = [np.where(rng.uniform(size=len(l)) < 0.2, rng.integers(1, 6, len(l)), 0).astype(np.uint32) for l in lists]
    kept, status = run(det, lists, points, 3.0, what="counts")
    assert (status == _ffi.AGX_SNAP_OK).all() and (kept > 0).all()
    run(det, lists, points, 3.0, words=words, what="counts and status words")
    for stride in (20, 32):
        run(det, lists, points, 3.0, words=words, stride=stride, table=[3, 0, 4, 2, 1], overflow=(2,), what="frame table, stride %d" % stride)
    run(det, lists[:3], points[:3], 3.0, with_counts=False, words=[None] * 3, what="neither counts nor a table")


def test_exact_ties_and_a_tag_table_read_in_place(det):
    g = np.arange(0, 40, dtype=F32) * 2
    lattice = np.zeros((1600, 5), F32)
    lattice[:, 0], lattice[:, 1] = np.tile(g, 40), np.repeat(g, 40)
    rng = np.random.default_rng(12)
    lists = [lattice[rng.permutation(1600)] for _ in range(3)]
    centres = (2 * rng.integers(0, 39, (3, 18, 4, 2)) + 1).astype(F32)  # four saddles at d2 = 2 each, in two chunks of the list
    for flags in (0, _ffi.AGX_SNAP_REVERSE):
        kept, _ = run(det, lists, list(centres), 2.0, flags=flags, what="ties")
        assert kept.sum() > 0
        run(det, lists, list(centres), 2.0, flags=flags, tag_table=True, what="ties through a tag table")
    run(det, lists, list(centres), np.nextafter(F32(2.0), F32(0)), what="one bit below the ties' distance")


def test_a_saddle_that_is_not_finite_refuses_its_frame_alone(det):
    rng = np.random.default_rng(13)
    lists = [random_list(rng, n) for n in (200, 1500, 90, 40)]
    lists[1][1400, 1] = np.inf  # (in the second chunk)
    lists[2][7, 0] = np.nan
    lists[3][5, 0] = np.nan
    words = [None, None, None, np.zeros(40, np.uint32)]
    words[3][5] = _ffi.AGX_POINT_FILTERED  # not listed: not looked at
    points = [points_near(rng, l[:30], 9, 4) for l in lists]
    _, status = run(det, lists, points, 4.0, words=words, what="non-finite saddles")
    assert list(status) == [_ffi.AGX_SNAP_OK, _ffi.AGX_SNAP_INPUT, _ffi.AGX_SNAP_INPUT, _ffi.AGX_SNAP_OK]


def test_refused_arguments_leave_the_batch_in_flight(det):
    import torch
    l = dev(random_list(np.random.default_rng(14), 50)[None])
    pts = dev(np.zeros((1, 3, 4, 2), F32))
    i32 = dict(dtype=torch.int32, device="cuda")
    out = [torch.zeros((1, 3, 4), **i32), torch.zeros((1, 3, 4), **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)]
    det.saddles_batch_enqueue(torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda"))

    def call(saddles=l.data_ptr(), stride=20, n=1, spf=50, counts=None, table=None, points=pts.data_ptr(), row_stride=32, point_stride=8, rpf=3,
             ppr=4, limit=1.0, flags=0, slots=out[0].data_ptr(), rows=out[1].data_ptr(), kept=out[2].data_ptr(), status=out[3].data_ptr()):
        return det._lib.agx_snap_points_enqueue(det._h, saddles, stride, n, spf, counts, table, None, points, row_stride, point_stride, rpf, ppr, None,
                                                float(limit), flags, slots, None, rows, kept, None, status)

    E = _ffi.AGX_ERR_ARG
    for kw in (dict(saddles=None), dict(n=0), dict(stride=16), dict(stride=22), dict(spf=0), dict(counts=out[2].data_ptr(), table=out[3].data_ptr()),
               dict(points=None), dict(slots=None), dict(rows=None), dict(kept=None), dict(status=None), dict(ppr=0), dict(ppr=5), dict(rpf=0),
               dict(row_stride=30), dict(point_stride=6), dict(point_stride=4), dict(row_stride=28), dict(limit=-1.0), dict(limit=np.nan),
               dict(flags=2), dict(points=pts.data_ptr() + 2), dict(n=1 << 15, rpf=1 << 12)):
        assert call(**kw) == E, kw
    res, _ = det.saddles_batch_fetch()  # still there
    assert len(res) == 1
    assert call(limit=np.inf) == _ffi.AGX_OK
    det.sync()


# ---- 2. the compacted rows as seeds, with nothing but the stream between -----------------------------------------------------------
def test_snapped_rows_feed_grow_boards_and_init_quads_in_place(det):
    import torch
    names = ["EuRoC.png", "r45.png", "top.png"]
    lists = [S.as_records(golden_list(n)) for n in names]
    n, spf = len(lists), max(len(l) for l in lists)
    batch = np.full((n, spf, 5), np.nan, F32)
    quads = []
    for f, l in enumerate(lists):
        batch[f, :len(l)] = l
        q, st, _ = A.find_board_tail(l, cap=1024)
        assert st == _ffi.AGX_BOARD_FOUND
        quads.append(q)
    R = 6
    pts = np.stack([l[q[:R].astype(np.int64), :2] + np.array([1.5, -2.0], F32) for l, q in zip(lists, quads)]).astype(F32)  # [n, R, 4, 2]
    pts[1, 2, 3] = (-50, -50)  # a row that does not snap whole: the rows behind it move up
    i32 = dict(dtype=torch.int32, device="cuda")
    d_batch, d_counts = dev(batch), dev(np.array([len(l) for l in lists], np.int32))
    slots, seeds, nseeds, sst = torch.zeros((n, R, 4), **i32), torch.zeros((n, R, 4), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
    out = dict(quads=torch.zeros((n, 128, 4), **i32), n_quads=torch.zeros(n, **i32), status=torch.zeros(n, **i32), best_seed=torch.zeros(n, **i32))
    det.snap_points_enqueue(d_batch, dev(pts), slots, seeds, nseeds, sst, 25.0, counts=d_counts)
    det.grow_boards_enqueue(d_batch, seeds, counts=d_counts, seed_counts=nseeds, **out)  # no sync in between
    det.grow_boards_fetch()
    assert nseeds.cpu().tolist() == [R, R - 1, R]
    for f, l in enumerate(lists):
        _s, _d, rows, _i, st = A.snap_points(l, pts[f], 25.0)
        want = A.grow_board_tail(l, rows, cap=128)
        assert int(out["status"][f]) == want[1] == _ffi.AGX_BOARD_FOUND and int(out["n_quads"][f]) == want[2]
        assert np.array_equal(out["quads"][f, :want[2]].cpu().numpy().view(np.uint32), want[0]) and int(out["best_seed"][f]) == want[4]
    # one corner per row: the seed saddles of init_quads
    one = np.ascontiguousarray(pts[:, :, :1])
    slots1, seeds1 = torch.zeros((n, R, 1), **i32), torch.zeros((n, R, 1), **i32)
    cand, ncand, cst = torch.zeros((n, 2048, 4), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
    det.snap_points_enqueue(d_batch, dev(one), slots1, seeds1, nseeds, sst, 25.0, counts=d_counts)
    det.init_quads_enqueue(d_batch, cand, ncand, cst, seed_saddles=seeds1.view(n, R), seed_counts=nseeds, counts=d_counts)
    det.init_quads_fetch()
    for f, l in enumerate(lists):
        rows = A.snap_points(l, one[f], 25.0)[2]
        want = A.init_quads_tail(l, seeds=rows.reshape(-1), cap=2048)
        assert int(cst[f]) == want[1] == _ffi.AGX_BOARD_FOUND and int(ncand[f]) == want[2]
        assert np.array_equal(cand[f, :want[2]].cpu().numpy().view(np.uint32), want[0])


# ---- 3. detect_tracked ----------------------------------------------------------------------------------------------------------------
def same_results(got, ref, what):
    for f, (g, r) in enumerate(zip(got, ref)):
        assert sorted(g) == sorted(r), "%s frame %d: ids" % (what, f)
        for t in r:
            assert bits_equal(g[t], r[t]), "%s frame %d: corners of tag %d" % (what, f, t)


def test_detect_tracked_equals_detect_batch_and_falls_back_frame_by_frame(det):
    import torch
    frames, _ = synth_module().render_batch(GPU_FIRST, GPU_FRAMES, *GPU_SIZE, device="cuda")
    ref = det.detect_batch(frames.cpu().numpy())
    assert all(len(r) >= 30 for r in ref)
    shift = np.array([1.5, -2.0], F32)
    prior = [{t: xy + shift for t, xy in r.items()} for r in ref]
    got, tracked = det.detect_tracked(frames, prior, max_dist=5.0)
    same_results(got, ref, "tracked")
    assert tracked.dtype == bool and tracked.all()
    # the device form of the prior, one seed a frame
    table = np.stack([np.pad(S.tag_rows(p).view(np.uint32).reshape(-1, 9), ((0, 40 - len(p)), (0, 0))) for p in prior])
    counts = torch.tensor([len(p) for p in prior], dtype=torch.int32, device="cuda")
    got, tracked = det.detect_tracked(frames, (dev(table.view(np.int32)), counts), max_dist=5.0, seeds_per_frame=1)
    same_results(got, ref, "tracked from one seed of a device table")
    assert tracked.all()
    # a frame without a prior is not tracked and comes back with the same tags, through detect_staged
    prior[3] = {}
    got, tracked = det.detect_tracked(frames, prior, max_dist=5.0)
    assert tracked.tolist() == [f != 3 for f in range(GPU_FRAMES)]
    same_results(got, ref, "with one frame lost")
