"""agx_grow_boards_enqueue / _fetch (k_grow_boards): boards grown on the device from caller-given seed quads at the caller's
spacing ratio.  The reference is the host form agx_grow_board_tail per frame, which tests/test_grow_boards_cpu.py holds to the
numpy yardstick (tests/board_grow_oracle.py) on the same lists; what keeps this from comparing the host form with itself is the
status BEFORE the fetch: a frame the kernel handed back reads AGX_BOARD_PENDING there.  No pixels but in the chain test: batches
of a few lists."""
import numpy as np
import pytest

from tests import board_cases as BC
from tests.test_find_boards_cpu import golden_list
from tests.test_grow_boards_cpu import HUGE_RATIOS, RATIO_STEPS, as_list, first_tag_seed, fix_list, gapped_lattice, ratio_values
from tests.util import ALL_IMAGES, bits_equal, synth_module

import aprilgrid_rs_amd as A

pytestmark = pytest.mark.gpu

FOUND, NONE, CAPACITY, INPUT, PENDING = 0, 1, 2, 3, 4
AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
SENT = 0x5A5A5A5A
Q = 128


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(l, seeds, **kw):
    return A.grow_board_tail(l, seeds, cap=kw.pop("cap", 1024), **kw)


def first_quad(l):
    """The first quad of the search's board (the host form at 0.3): a seed."""
    quads, status, _ = A.find_board_tail(l, cap=1024)
    assert status == FOUND
    return [quads[0]]


def run(det, lists, seeds, q=Q, stride=5, point_status=None, fetch=True, **kw):
    """One batch: frame f = lists[f] (NaN behind its count) and seeds[f] ([k, 4]; the batch's seed rows behind a frame's own hold
    slot 0xFFFFFFF0, which no frame has) -> dict of the outputs before and after the fetch (sentinel-filled arrays)."""
    import torch
    n = len(lists)
    S = max(max(len(l) for l in lists), 1) + 3
    batch = np.full((n, S, stride), np.nan, np.float32)
    for f, l in enumerate(lists):
        batch[f, :len(l), :5] = l
    K = max(max(len(s) for s in seeds), 1)
    sq = np.full((n, K, 4), 0xFFFFFFF0, np.uint32)
    for f, s in enumerate(seeds):
        sq[f, :len(s)] = np.asarray(s, np.uint32).reshape(-1, 4)
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(quads=torch.full((n, q, 4), SENT, **i32), quad_points=torch.full((n, q, 4, 2), -7.0, dtype=torch.float32, device="cuda"),
               n_quads=torch.full((n,), SENT, **i32), status=torch.full((n,), SENT, **i32), seed_scores=torch.full((n, K), SENT, **i32),
               best_seed=torch.full((n,), SENT, **i32))
    ps = None
    if point_status is not None:
        ps = np.zeros((n, S), np.int32)
        for f, w in enumerate(point_status):
            ps[f, :len(w)] = w
        ps = dev(ps)
    det.grow_boards_enqueue(dev(batch), dev(sq.view(np.int32)), counts=dev(np.array([len(l) for l in lists], np.int32)),
                            seed_counts=dev(np.array([len(s) for s in seeds], np.int32)), point_status=ps, **out, **kw)
    det.sync()
    grab = lambda: {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.float32).copy() for k, v in out.items()}
    before = grab()
    if not fetch:
        return before, None
    det.grow_boards_fetch()
    assert det.get_option("last_grow_boards_frames") == n
    assert det.get_option("last_grow_boards_handed_back") == int((before["status"] == PENDING).sum())
    return before, grab()


def check_frame(what, l, seeds, res, f, q=Q, **kw):
    """Frame f of `res` against the host form, byte for byte; everything at or beyond the counts is untouched."""
    rq, rst, rn, rsc, rbest = host(l, seeds, **kw)
    if rst == FOUND and rn > q:
        rst, rq = CAPACITY, rq[:0]
    quads, pts = res["quads"][f], res["quad_points"][f]
    assert (int(res["status"][f]), int(res["n_quads"][f])) == (rst, rn), "%s: status %d count %d, host form %d %d" % (
        what, res["status"][f], res["n_quads"][f], rst, rn)
    rows = len(rq)
    assert quads[:rows].tobytes() == rq.tobytes(), what + ": rows"
    assert (quads[rows:] == SENT).all() and (pts[rows:] == np.float32(-7.0)).all(), what + ": a row at or beyond the count was written"
    if rows:
        assert bits_equal(pts[:rows], l[rq.astype(np.int64)][:, :, :2]), what + ": quad points"
    sc = res["seed_scores"][f]
    if rsc is None:
        assert (sc == SENT).all() and res["best_seed"][f] == SENT, what + ": scores of a frame without a board"
    else:
        assert sc[:len(rsc)].tobytes() == rsc.tobytes() and (sc[len(rsc):] == SENT).all(), "%s: seed scores %s, host form %s" % (what, sc, rsc)
        assert res["best_seed"][f] == rbest, what + ": best seed"


def check_all(names, lists, seeds, before, after, device=(), **kw):
    for f, name in enumerate(names):
        if before["status"][f] != PENDING:  # the kernel's own answer stands as it was written
            check_frame(name + " (before the fetch)", lists[f], seeds[f], before, f, **kw)
        check_frame(name, lists[f], seeds[f], after, f, **kw)
    late = [n for f, n in enumerate(names) if n in device and before["status"][f] == PENDING]
    assert not late, "handed back although the kernel must answer them: %s" % late
    assert not (after["status"] == PENDING).any()


# ---- 1: a mixed batch ------------------------------------------------------------------------------------------------------------
def test_mixed_batch_is_the_host_forms_answer_frame_by_frame(det):
    names, lists, seeds = [], [], []
    for name in ALL_IMAGES:
        l = as_list(golden_list(name))
        names.append(name), lists.append(l), seeds.append(first_quad(l))
    for name in ("lattice 7x7", "lattice 13x13", "lattice 7x7 perm 2"):
        l = BC.build(name)
        names.append(name), lists.append(l), seeds.append(first_quad(l))
    l7 = BC.lattice(7, 7)
    nan = l7.copy()
    nan[20, 0] = np.nan
    names += ["empty list", "no seed", "a saddle that is not finite", "a seed beyond the list"]
    lists += [l7[:0], l7, nan, l7]
    seeds += [np.zeros((0, 4), np.uint32), np.zeros((0, 4), np.uint32), first_quad(l7), [[0, 1, 49, 7]]]
    before, after = run(det, lists, seeds)
    device = [n for n in names if n in BC.BY_NAME and BC.BY_NAME[n].expect == "device"] + names[-4:]
    check_all(names, lists, seeds, before, after, device=device)
    assert list(after["status"][-4:]) == [NONE, NONE, INPUT, INPUT]
    answered = int((before["status"] != PENDING).sum())
    print("answered by the kernel: %d of %d" % (answered, len(names)))
    assert 4 * answered >= 3 * len(names)
    again = run(det, lists, seeds)[1]
    assert all(after[k].tobytes() == again[k].tobytes() for k in after)


# ---- 2: ratios -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lower", "upper"])
def test_ratio_thresholds_through_the_kernel(det, which):
    l = BC.lattice(7, 7)
    seed = first_quad(l)
    v, k = ratio_values(which), len(RATIO_STEPS)
    for r in (v[0], v[k], v[k - 1], v[-1]):  # both neighbours of the change, and 100 steps either side
        before, after = run(det, [l, l], [seed, seed], spacing_ratio=float(r))
        check_all(["ratio %r" % float(r)] * 2, [l, l], [seed, seed], before, after, spacing_ratio=float(r))
        assert not (before["status"] == PENDING).any()


@pytest.mark.parametrize("ratio", HUGE_RATIOS)
def test_a_huge_finite_ratio_is_answered_by_the_kernel(det, ratio):
    """The query point lies beyond 1e9 (at 3.2e38: at infinity): expand_one_w / probe4_w look at every saddle, not at grid cells."""
    lists = [BC.lattice(7, 7), BC.lattice(13, 13)]
    seeds = [first_quad(l) for l in lists]
    before, after = run(det, lists, seeds, spacing_ratio=ratio)
    check_all(["7x7", "13x13"], lists, seeds, before, after, spacing_ratio=ratio)
    assert not (before["status"] == PENDING).any() and list(after["n_quads"]) == [1, 1] and after["seed_scores"][:, 0].tolist() == [1, 1]


def test_gapped_lattice_at_both_ratios_in_one_process(det):
    lists = [gapped_lattice(2), gapped_lattice(3)]
    seeds = [first_tag_seed(lists[0], 2), first_tag_seed(lists[1], 3)]
    for ratio, counts in ((0.3, [1, 1]), (1.5, [4, 9]), (0.3, [1, 1])):
        before, after = run(det, lists, seeds, spacing_ratio=ratio)
        check_all(["gapped 2", "gapped 3"], lists, seeds, before, after, spacing_ratio=ratio)
        assert list(after["n_quads"]) == counts and not (before["status"] == PENDING).any()


# ---- 3: many seeds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 9, 20])
def test_many_seeds_and_the_stop_rule(det, k):
    l = BC.lattice(13, 13)
    board = A.find_board_tail(l, cap=1024)[0]
    far = np.concatenate([l, BC.lattice(3, 3, origin=(1500.0, 1500.0))])
    lone = A.find_board_tail(far[169:], cap=16)[0] + 169
    low_first = np.concatenate([np.repeat(lone[:1], max(k - 2, 0), axis=0), board[:2]])[:k]  # scores 1, ..., 1, 36, 36
    lists, seeds = [l, l, far, far], [board[:k], board[5:5 + k][::-1], low_first, low_first]
    for stop in (0, 36, 2, 1000):
        before, after = run(det, lists, seeds, stop_score=stop)
        check_all(["13x13 / %d seeds / stop %d" % (k, stop)] * 4, lists, seeds, before, after, stop_score=stop)
        assert not (before["status"] == PENDING).any()
        if stop == 36:
            assert after["seed_scores"][0][:k].tolist() == [36] + [0] * (k - 1)
    assert after["best_seed"][0] == 0 and after["best_seed"][2] == (max(k - 2, 0) if k > 1 else 0)


def test_fix_missing_flag_on_the_device(det):
    l, seed = fix_list()
    for flag in (True, False):
        before, after = run(det, [l, BC.lattice(7, 7)], [seed, first_quad(BC.lattice(7, 7))], fix_missing=flag)
        check_all(["fix list", "lattice 7x7"], [l, BC.lattice(7, 7)], [seed, first_quad(BC.lattice(7, 7))], before, after, fix_missing=flag)
    assert after["n_quads"][0] == 15


# ---- 4: hand-back ----------------------------------------------------------------------------------------------------------------
def test_a_wide_guard_band_hands_frames_back_and_changes_nothing(det):
    names = ["lattice 7x7 rot 30", "lattice 9x9 rot 45", "lattice 13x13"]
    lists = [BC.build(n) for n in names]
    seeds = [first_quad(l) for l in lists]
    det.set_option("tail_debug_band", 30000)  # 30 degrees (the most): the 90 degrees of every valid quad of a lattice lie in the band
    try:
        before, after = run(det, lists, seeds)
    finally:
        det.set_option("tail_debug_band", 0)
    assert (before["status"] == PENDING).all() and (before["quads"] == SENT).all()
    check_all(names, lists, seeds, before, after)
    assert (after["status"] == FOUND).all()


def test_pairs_that_straddle_the_kernels_sizes(det):
    names = ["strip 2x26", "strip 2x28", "lattice 20x20", "lattice 21x21", "7x7 and far saddles, 1024 in all", "7x7 and far saddles, 1025 in all"]
    lists = [BC.build(n) for n in names]
    seeds = [first_quad(l) for l in lists]
    before, after = run(det, lists, seeds)
    for f, n in enumerate(names):
        print("before the fetch: %-40s %s" % (n, "PENDING (handed back)" if before["status"][f] == PENDING else "answered by the kernel"))
    check_all(names, lists, seeds, before, after)
    assert before["status"][4] != PENDING and before["status"][5] == PENDING  # (TN follows from the constant)


def test_without_the_device_tail_every_frame_is_pending():
    d = A.TagDetector("t36h11", None, device=0)
    try:
        d.set_option("device_tail", 0)
        l = BC.lattice(7, 7)
        before, after = run(d, [l, l[:0]], [first_quad(l), np.zeros((0, 4), np.uint32)])
        assert (before["status"] == PENDING).all()
        check_all(["lattice 7x7", "empty"], [l, l[:0]], [first_quad(l), np.zeros((0, 4), np.uint32)], before, after)
    finally:
        d.close()


# ---- 5: layouts ----------------------------------------------------------------------------------------------------------------
def test_padded_stride_point_status_capacity_and_frame_table(det):
    import torch
    l = BC.lattice(7, 7)
    board = A.find_board_tail(l, cap=64)[0]
    seed = [board[0]]
    words = np.zeros(49, np.int32)
    words[board[4][1]] = 2  # a board saddle is not listed
    for stride in (5, 8):
        before, after = run(det, [l, l], [seed, seed], stride=stride, point_status=[words, np.zeros(49, np.int32)])
        check_frame("a board saddle removed", l, seed, after, 0, point_status=words.view(np.uint32))
        check_frame("all listed", l, seed, after, 1)
        assert after["n_quads"][0] < 9 and not (before["status"] == PENDING).any()
    words[board[0][2]] = 2  # the seed names a slot that is not listed
    before, after = run(det, [l], [seed], point_status=[words])
    assert before["status"][0] == INPUT and after["n_quads"][0] == 0
    before, after = run(det, [l, l], [seed, seed], q=8)  # one row short
    check_all(["cap 8"] * 2, [l, l], [seed, seed], before, after, q=8)
    assert list(after["status"]) == [CAPACITY, CAPACITY] and list(after["n_quads"]) == [9, 9] and list(after["best_seed"]) == [0, 0]
    # a frame table instead of counts: two lists back to back in one flat array, the second entry with an overflow bit in a third
    flat = np.concatenate([np.zeros((3, 5), np.float32), l, BC.lattice(9, 9)])
    table = np.array([[49, 3, 0, 0], [81, 52, 0, 0], [49, 3, 2, 0]], np.int32)
    l9 = BC.lattice(9, 9)
    sq = np.stack([np.asarray(seed, np.uint32), np.asarray(first_quad(l9), np.uint32), np.asarray(seed, np.uint32)]).reshape(3, 1, 4)
    i32 = dict(dtype=torch.int32, device="cuda")

    def table_pass(d, host_only):
        out = dict(quads=torch.full((3, Q, 4), SENT, **i32), quad_points=torch.full((3, Q, 4, 2), -7.0, dtype=torch.float32, device="cuda"),
                   n_quads=torch.full((3,), SENT, **i32), status=torch.full((3,), SENT, **i32), seed_scores=torch.full((3, 1), SENT, **i32),
                   best_seed=torch.full((3,), SENT, **i32))
        d.grow_boards_enqueue(dev(flat), dev(sq.view(np.int32)), frame_table=dev(table), **out)
        d.sync()
        if host_only:  # the kernel read no table: the overflow entry is the host form's to refuse
            assert (out["status"].cpu().numpy() == PENDING).all()
        d.grow_boards_fetch()
        res = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.float32).copy() for k, v in out.items()}
        quads, nq, st = res["quads"], res["n_quads"], res["status"]
        assert list(st) == [FOUND, FOUND, INPUT] and list(nq) == [9, 16, 0]
        assert quads[0, :9].tobytes() == host(l, seed)[0].tobytes() and quads[1, :16].tobytes() == host(l9, first_quad(l9))[0].tobytes()
        assert (quads[2] == SENT).all()
        assert (res["quad_points"][2] == np.float32(-7.0)).all() and res["seed_scores"][2, 0] == SENT and res["best_seed"][2] == SENT
        return res

    first = table_pass(det, False)
    # the same batch without the device tail: the fetch's host form answers all three, the overflow entry included
    d0 = A.TagDetector("t36h11", None, device=0)
    try:
        d0.set_option("device_tail", 0)
        second = table_pass(d0, True)
        assert d0.get_option("last_grow_boards_handed_back") == 3
    finally:
        d0.close()
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)


def test_frame_table_and_records_of_the_saddle_chain_for_one_rendered_frame(det):
    """d_frame_table instead of d_counts on agx_saddles_batch_enqueue_to's own outputs: its record layout, offsets and status words
    as they stand.  Three small frames, so that entries have offsets of their own, in whatever order the chain emitted them."""
    import torch
    from tests.test_find_boards_cpu import GPU_FIRST, GPU_SIZE
    n = 3
    frames, _ = synth_module().render_batch(GPU_FIRST, n, *GPU_SIZE, device="cuda")
    d_saddles = torch.zeros((n * 1024, 5), dtype=torch.float32, device="cuda")
    d_table = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    det.saddles_batch_enqueue_to(frames, d_saddles, d_table)
    det.sync()
    table, all_s = d_table.cpu().numpy(), d_saddles.cpu().numpy()
    assert not (table[:, 2] & 7).any() and len(set(table[:, 1].tolist())) == n  # (offsets in the order the chain emitted the frames)
    lists = [all_s[table[f, 1]:table[f, 1] + table[f, 0]].copy() for f in range(n)]
    boards = [A.find_board_tail(l, cap=1024) for l in lists]
    assert all(b[1] == FOUND and b[2] >= 4 for b in boards)
    seeds = np.stack([np.stack([b[0][0], b[0][b[2] // 2]]) for b in boards]).astype(np.uint32)  # two quads of the host form's board each
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(quads=torch.full((n, Q, 4), SENT, **i32), quad_points=torch.full((n, Q, 4, 2), -7.0, dtype=torch.float32, device="cuda"),
               n_quads=torch.full((n,), SENT, **i32), status=torch.full((n,), SENT, **i32), seed_scores=torch.full((n, 2), SENT, **i32),
               best_seed=torch.full((n,), SENT, **i32))
    det.grow_boards_enqueue(d_saddles, dev(seeds.view(np.int32)), frame_table=d_table, **out)
    det.sync()
    grab = lambda: {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.float32).copy() for k, v in out.items()}
    before = grab()
    det.grow_boards_fetch()
    after = grab()
    assert not (before["status"] == PENDING).any()
    for f in range(n):
        check_frame("frame %d (before the fetch)" % f, lists[f], seeds[f], before, f)
        check_frame("frame %d" % f, lists[f], seeds[f], after, f)
        assert after["status"][f] == FOUND and after["n_quads"][f] == boards[f][2]


# ---- 6: the whole chain on a rendered frame ----------------------------------------------------------------------------------------
def test_seeded_grow_completes_the_staged_chain_on_a_rendered_frame():
    import torch
    from tests.test_gpu_collect_tags import SH, SW, stages_for_the_host_loop
    from tests import board_grow_oracle as Y
    one = A.DetectorParams.default_params()
    one.max_num_of_boards = 1
    d = A.TagDetector("t36h11", one, device=0)
    try:
        frames, _ = synth_module().render_batch(40, 1, SW, SH, device="cuda")
        want = d.detect(frames[0].cpu().numpy())
        assert len(want) >= 4
        (records, pstatus, counts), h_records, h_words, h_counts = stages_for_the_host_loop(d, frames)
        c = int(h_counts[0])
        listed = np.flatnonzero(h_words[0, :c] == 0)
        corners = want[sorted(want)[0]]  # one returned tag: its corners as points, matched to the frame's listed slots
        nearest = [int(listed[np.argmin(((h_records[0, listed, :2] - p) ** 2).sum(axis=1))]) for p in corners]
        seed = np.array([nearest[::-1]], np.uint32)  # (detect reverses a quad's corners, detector.rs:469: back in init_quads' winding)
        # on the CPU first, with the yardstick: the seeded board has the search's quads
        grown = Y.grow(h_records[0, :c], seed, point_status=h_words[0, :c])
        search = A.find_board_tail(h_records[0, :c][h_words[0, :c] == 0], cap=1024)[0]
        as_sets = lambda qs, m=None: {frozenset(int(i) if m is None else int(m[i]) for i in q) for q in qs}
        assert grown[1] == FOUND and as_sets(grown[0]) == as_sets(search, listed)
        i32 = dict(dtype=torch.int32, device="cuda")
        quads, qpts = torch.zeros((1, Q, 4), **i32), torch.zeros((1, Q, 4, 2), dtype=torch.float32, device="cuda")
        nq, bst = torch.zeros(1, **i32), torch.zeros(1, **i32)
        qtags, qst = torch.zeros((1, Q, 9), **i32), torch.zeros((1, Q), **i32)
        tags, ntags, tst = torch.zeros((1, 587, 9), **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
        d.grow_boards_enqueue(records, dev(seed.view(np.int32).reshape(1, 1, 4)), quads, nq, bst, counts=counts, point_status=pstatus,
                              quad_points=qpts, spacing_ratio=0.3, fix_missing=True)
        d.grow_boards_fetch()
        d.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst)
        d.collect_tags_enqueue(quads, nq, bst, qtags, qst, None, tags, ntags, tst, reset=True, saddles_per_frame=records.shape[1])
        d.sync()
        assert int(bst.cpu()[0]) == FOUND and int(tst.cpu()[0]) == 0
        table = tags.cpu().numpy().view(np.uint32).reshape(587, 9)[:int(ntags.cpu()[0])]
        got = {int(r[0]): r[1:].view(np.float32).reshape(4, 2) for r in table}
        assert sorted(got) == sorted(want) and all(bits_equal(got[t], want[t]) for t in want)
    finally:
        d.close()


# ---- 7: batch state --------------------------------------------------------------------------------------------------------------
def test_batch_state_rules(det):
    import torch
    lib, h = det._lib, det._h
    l = BC.lattice(7, 7)
    seed = first_quad(l)
    assert lib.agx_grow_boards_fetch(h, 1) == AGX_ERR_STATE  # nothing in flight
    frames = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    pts = torch.full((1, 4, 2), 20.0, dtype=torch.float32, device="cuda")
    det.refine_points_enqueue(frames, pts)
    before, _ = run(det, [l], [seed], fetch=False)  # replaces the refine batch without waiting
    assert before["status"][0] == FOUND
    assert lib.agx_refine_points_fetch(h, None, None) == AGX_ERR_STATE
    assert lib.agx_find_boards_fetch(h, None, None, None, None, 1) == AGX_ERR_STATE
    # refused arguments leave the batch in flight
    i32 = dict(dtype=torch.int32, device="cuda")
    s, sq = dev(l[None]), dev(np.asarray(seed, np.uint32).view(np.int32).reshape(1, 1, 4))
    quads, nq, st = torch.zeros((1, Q, 4), **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
    for bad in (dict(spacing_ratio=float("nan")), dict(spacing_ratio=-1.0), dict(spacing_ratio=float("inf"))):
        with pytest.raises(A.AgxError) as e:
            det.grow_boards_enqueue(s, sq, quads, nq, st, **bad)
        assert e.value.status == AGX_ERR_ARG
    args = [h, s.data_ptr(), 20, 1, 49, None, None, None, sq.data_ptr(), 1, None, 0.3, 0, 1, Q, quads.data_ptr(), None, nq.data_ptr(), st.data_ptr(), None, None]
    for i, v in ((1, None), (2, 18), (3, 0), (4, 0), (8, None), (9, 0), (13, 2), (14, 0), (15, None), (17, None), (18, None), (5, nq.data_ptr())):
        a = list(args)
        a[i] = v
        if i == 5:
            a[6] = nq.data_ptr()  # both d_counts and d_frame_table
        assert lib.agx_grow_boards_enqueue(*a) == AGX_ERR_ARG, "argument %d" % i
    assert lib.agx_grow_boards_fetch(h, 1) == AGX_OK  # still there
    assert lib.agx_grow_boards_fetch(h, 1) == AGX_ERR_STATE
    # (no replay inside a captured graph here: agx_find_boards_enqueue has no such test to model it on)
