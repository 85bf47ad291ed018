"""agx_init_quads_enqueue / _fetch (k_init_quads): the candidate quads of caller-given seed saddles, or of the reference's own
seeds, on the device.  The reference is the host form agx_init_quads_tail per frame, which tests/test_init_quads_cpu.py holds to
the numpy yardstick on the same lists; what keeps this from comparing the host form with itself is the status BEFORE the fetch:
a frame the kernel handed back reads AGX_BOARD_PENDING there, and the lattice lists must not."""
import numpy as np
import pytest

from tests import board_cases as BC
from tests.test_find_boards_cpu import golden_list
from tests.test_grow_boards_cpu import as_list, gapped_lattice
from tests.util import ALL_IMAGES, bits_equal, synth_module

import aprilgrid_rs_amd as A

pytestmark = pytest.mark.gpu

FOUND, NONE, CAPACITY, INPUT, PENDING = 0, 1, 2, 3, 4
AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
SENT = 0x5A5A5A5A
Q = 1024


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(det, lists, seeds, spf=None, q=Q, k=50, stride=5, point_status=None, fetch=True):
    """One batch: frame f = lists[f] (NaN behind its count); seeds: None (the reference's own, at most spf) or a list of slot
    numbers per frame (the rows behind a frame's own hold slot 0xFFFFFFF0, which no frame has) -> (K, the outputs before the fetch,
    after it), sentinel-filled arrays."""
    import torch
    n = len(lists)
    S = max(max(len(l) for l in lists), 1) + 3
    batch = np.full((n, S, stride), np.nan, np.float32)
    for f, l in enumerate(lists):
        batch[f, :len(l), :5] = l
    sd = sc = None
    K = int(spf or 30)
    if seeds is not None:
        K = max(max(len(s) for s in seeds), 1)
        sq = np.full((n, K), 0xFFFFFFF0, np.uint32)
        for f, s in enumerate(seeds):
            sq[f, :len(s)] = np.asarray(s, np.uint32)
        sd, sc = dev(sq.view(np.int32)), dev(np.array([len(s) for s in seeds], np.int32))
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(quads=torch.full((n, q, 4), SENT, **i32), quad_points=torch.full((n, q, 4, 2), -7.0, dtype=torch.float32, device="cuda"),
               n_quads=torch.full((n,), SENT, **i32), status=torch.full((n,), SENT, **i32), seed_quad_counts=torch.full((n, K), SENT, **i32),
               seeds_out=torch.full((n, K), SENT, **i32), n_seeds_out=torch.full((n,), SENT, **i32))
    ps = None
    if point_status is not None:
        ps = np.zeros((n, S), np.int32)
        for f, w in enumerate(point_status):
            ps[f, :len(w)] = w
        ps = dev(ps)
    det.init_quads_enqueue(dev(batch), seed_saddles=sd, seed_counts=sc, seeds_per_frame=K, n_nearest=k,
                           counts=dev(np.array([len(l) for l in lists], np.int32)), point_status=ps, **out)
    det.sync()
    grab = lambda: {k_: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.float32).copy() for k_, v in out.items()}
    before = grab()
    if not fetch:
        return K, before, None
    det.init_quads_fetch()
    assert det.get_option("last_init_quads_frames") == n
    assert det.get_option("last_init_quads_handed_back") == int((before["status"] == PENDING).sum())
    return K, before, grab()


def check_frame(what, l, seeds, K, res, f, q=Q, k=50, point_status=None):
    """Frame f of `res` against the host form, byte for byte; everything at or beyond the counts is untouched."""
    rq, rst, rn, rper, rtaken = A.init_quads_tail(l, seeds, max_seeds=K, n_nearest=k, cap=q, point_status=point_status)
    quads, pts = res["quads"][f], res["quad_points"][f]
    assert (int(res["status"][f]), int(res["n_quads"][f])) == (rst, rn), "%s: status %d count %d, host form %d %d" % (
        what, res["status"][f], res["n_quads"][f], rst, rn)
    rows = len(rq)
    assert quads[:rows].tobytes() == rq.tobytes(), what + ": rows"
    assert (quads[rows:] == SENT).all() and (pts[rows:] == np.float32(-7.0)).all(), what + ": a row at or beyond the count was written"
    if rows:
        assert bits_equal(pts[:rows], l[rq.astype(np.int64)][:, :, :2]), what + ": quad points"
    per, taken = res["seed_quad_counts"][f], res["seeds_out"][f]
    if rper is None:
        assert (per == SENT).all() and (taken == SENT).all() and res["n_seeds_out"][f] == 0, what + ": per-seed outputs of an AGX_BOARD_INPUT frame"
    else:
        assert per.tobytes() == rper.tobytes(), "%s: quads per seed %s, host form %s" % (what, per, rper)
        assert res["n_seeds_out"][f] == len(rtaken) and taken[:len(rtaken)].tobytes() == rtaken.tobytes(), what + ": the seeds taken"
        assert (taken[len(rtaken):] == SENT).all(), what + ": a seed row beyond the count was written"


def check_all(names, lists, seeds, K, before, after, device=(), **kw):
    for f, name in enumerate(names):
        s = None if seeds is None else seeds[f]
        if before["status"][f] != PENDING:  # the kernel's own answer stands as it was written
            check_frame(name + " (before the fetch)", lists[f], s, K, before, f, **kw)
        check_frame(name, lists[f], s, K, after, f, **kw)
    late = [n for f, n in enumerate(names) if n in device and before["status"][f] == PENDING]
    assert not late, "handed back although the kernel must answer them: %s" % late
    assert not (after["status"] == PENDING).any()


def prune_count(l, s0, k):
    """The keys k_init_quads' first pass keeps of a list of more than 128 saddles: those at or below the k-th smallest of the 64
    lanes' minima (a lane holds every 64th saddle); up to 128 are sorted, more send the seed down the unpruned sort."""
    d = (l[s0, 0] - l[:, 0]).astype(np.float32)
    e = (l[s0, 1] - l[:, 1]).astype(np.float32)
    d2 = (d * d + e * e).astype(np.float32)
    key = d2.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.arange(len(l), dtype=np.uint64)
    mins = np.sort(np.array([key[lane::64].min() for lane in range(64)]))
    return int((key <= mins[k - 1]).sum())


# ---- 1: a mixed batch of the golden lists --------------------------------------------------------------------------------------
def test_mixed_batch_is_the_host_forms_answer_frame_by_frame(det):
    names, lists = [], []
    for name in ALL_IMAGES:
        names.append(name), lists.append(as_list(golden_list(name)))
    l7 = BC.lattice(7, 7)
    nan = l7.copy()
    nan[20, 0] = np.nan
    names += ["lattice 7x7", "empty list", "a saddle that is not finite"]
    lists += [l7, l7[:0], nan]
    seeds = [list(range(min(64, len(l)))) for l in lists]
    K, before, after = run(det, lists, seeds, q=2048)  # (the lattice's 49 seeds have more than 1024 quads)
    check_all(names, lists, seeds, K, before, after, device=names[-3:], q=2048)
    print("caller seeds: pending before the fetch: %d of %d frames" % (int((before["status"] == PENDING).sum()), len(names)))
    assert list(after["status"][-3:]) == [FOUND, NONE, INPUT]
    seeds[-3] = seeds[-3] + [49]  # a seed beyond the list
    K, before, after = run(det, lists[-3:], seeds[-3:])
    check_all(names[-3:], lists[-3:], seeds[-3:], K, before, after, device=names[-3:])
    assert list(before["status"]) == [INPUT, NONE, INPUT]
    K, before, after = run(det, lists, None, spf=30)
    check_all(names, lists, None, K, before, after, device=names[-3:])
    print("the reference's seeds: pending before the fetch: %d of %d frames" % (int((before["status"] == PENDING).sum()), len(names)))
    again = run(det, lists, None, spf=30)[2]
    assert all(after[k].tobytes() == again[k].tobytes() for k in after)


# ---- 2: list lengths at the edges of the three sort paths ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [50, 8, 64])
def test_lattice_prefixes_are_answered_by_the_kernel(det, k):
    full = BC.lattice(12, 12)
    lengths = (1, 2, 50, 51, 64, 65, 128, 129)
    lists = [full[:n].copy() for n in lengths]
    names = ["%d saddles" % n for n in lengths]
    seeds = [sorted({0, n // 2, n - 1}) for n in lengths]
    K, before, after = run(det, lists, seeds, k=k)
    assert not (before["status"] == PENDING).any(), "a lattice list was handed back: %s" % before["status"]
    check_all(names, lists, seeds, K, before, after, device=names, k=k)
    K, before, after = run(det, lists, None, spf=30, k=k, q=2048)  # (up to 1771 rows: beyond the 1024 the kernel keeps, too)
    assert not (before["status"] == PENDING).any()
    check_all(names, lists, None, K, before, after, device=names, k=k, q=2048)
    assert (after["status"][2:] == FOUND).all()


def test_1024_saddles_pruned_unpruned_and_1025(det):
    far = BC.far_saddles(1024, 5)
    # the pruned sort: the lattice's saddles 21 positions apart, one to a lane class
    l7 = BC.lattice(7, 7)
    at = (np.arange(49) * 21) % 1024
    spread = far.copy()
    spread[at] = l7
    # the unpruned sort: the 64 saddles of a lattice at the positions = 0 .. 3 (mod 64), so that 60 lanes' minima are far saddles
    l8 = BC.lattice(8, 8)
    pos = np.array([64 * r + c for r in range(16) for c in range(4)])
    packed = far.copy()
    packed[pos] = l8
    over = np.concatenate([spread, BC.far_saddles(1, 9)])
    seeds = [[int(at[24]), int(at[0]), 1], [int(pos[27]), int(pos[0]), 5], [int(at[24])]]
    assert all(prune_count(spread, s, 50) <= 128 for s in seeds[0]), "the premise of the pruned case"
    assert all(prune_count(packed, s, 50) > 128 for s in seeds[1][:2]), "the premise of the unpruned case"
    names, lists = ["1024, pruned", "1024, unpruned", "1025"], [spread, packed, over]
    K, before, after = run(det, lists, seeds)
    assert list(before["status"]) == [FOUND, FOUND, PENDING]
    check_all(names, lists, seeds, K, before, after, device=names[:2])
    assert after["n_quads"][0] > 0 and after["n_quads"][1] > 0 and after["status"][2] == FOUND
    K, before, after = run(det, lists, None, spf=9)
    assert list(before["status"]) == [FOUND, FOUND, PENDING]
    check_all(names, lists, None, K, before, after, device=names[:2])


# ---- 3: seeds per frame: one group, a full group, the group boundary, four groups -----------------------------------------------
@pytest.mark.parametrize("n_seeds", [1, 8, 9, 30])
def test_seed_groups_keep_the_order(det, n_seeds):
    g = as_list(golden_list(list(ALL_IMAGES)[0]))
    l9 = BC.lattice(9, 9)
    lists, names = [g, l9], ["golden list", "lattice 9x9"]
    seeds = [[(7 * i + 3) % len(l) for i in range(n_seeds)] for l in lists]
    K, before, after = run(det, lists, seeds)
    check_all(names, lists, seeds, K, before, after, device=names[1:])
    assert after["seed_quad_counts"][1].sum() == after["n_quads"][1] and after["status"][1] == FOUND
    rows = after["quads"][1][:after["n_quads"][1]]
    assert (rows[:, 0] == np.repeat(np.asarray(seeds[1], np.uint32), after["seed_quad_counts"][1])).all(), "column 0 is the row's seed, seed after seed"
    K, before, after = run(det, lists, None, spf=n_seeds)
    check_all(names, lists, None, K, before, after, device=names[1:])
    assert after["n_seeds_out"][1] == n_seeds


# ---- 4 .. 6: hand-back ---------------------------------------------------------------------------------------------------------
def test_a_seed_beyond_the_candidate_list_is_handed_back(det):
    # every saddle six times: 6^3 times the centre's two valid quads, 432 -- beyond the 256 of a seed's list; five times: 250
    l6, l5 = BC.repeated(BC.lattice(7, 7), 6), BC.repeated(BC.lattice(7, 7), 5)
    seeds = [[6 * 24, 0], [5 * 24, 0]]
    K, before, after = run(det, [l6, l5], seeds)
    assert list(before["status"]) == [PENDING, FOUND]
    check_all(["7x7 six times", "7x7 five times"], [l6, l5], seeds, K, before, after, device=["7x7 five times"])
    assert after["seed_quad_counts"][0][0] == 432 and after["seed_quad_counts"][1][0] == 250 and after["status"][0] == FOUND


def test_a_wide_guard_band_hands_frames_back_and_changes_nothing(det):
    names = ["lattice 7x7 rot 30", "lattice 9x9 rot 45", "lattice 13x13"]
    lists = [BC.build(n) for n in names]
    seeds = [[0, len(l) // 2] for l in lists]
    _, _, plain = run(det, lists, seeds)
    det.set_option("tail_debug_band", 30000)  # 30 degrees (the most): the 90 degrees of every valid quad of a lattice lie in the band
    try:
        K, before, after = run(det, lists, seeds)
    finally:
        det.set_option("tail_debug_band", 0)
    assert (before["status"] == PENDING).all() and (before["quads"] == SENT).all()
    check_all(names, lists, seeds, K, before, after)
    assert (after["status"] == FOUND).all() and all(plain[k].tobytes() == after[k].tobytes() for k in after)


def test_without_the_device_tail_every_frame_is_pending():
    d = A.TagDetector("t36h11", None, device=0)
    try:
        d.set_option("device_tail", 0)
        l = BC.lattice(7, 7)
        K, before, after = run(d, [l, l[:0]], [[24], []])
        assert (before["status"] == PENDING).all()
        check_all(["lattice 7x7", "empty"], [l, l[:0]], [[24], []], K, before, after)
        K, before, after = run(d, [l, l[:0]], None, spf=30)
        assert (before["status"] == PENDING).all()
        check_all(["lattice 7x7", "empty"], [l, l[:0]], None, K, before, after)
    finally:
        d.close()


# ---- 7: layouts ----------------------------------------------------------------------------------------------------------------
def test_padded_stride_point_status_capacity_and_frame_table(det):
    import torch
    l = BC.lattice(7, 7)
    words = np.zeros(49, np.int32)
    words[25] = 2  # a neighbour of the seed is not listed
    seeds = [[24, 8], [24, 8]]
    for stride in (5, 8):
        K, before, after = run(det, [l, l], seeds, stride=stride, point_status=[words, np.zeros(49, np.int32)])
        assert not (before["status"] == PENDING).any()
        check_frame("a saddle removed", l, seeds[0], K, before, 0, point_status=words.view(np.uint32))
        check_frame("all listed", l, seeds[1], K, before, 1)
        assert 0 < before["n_quads"][0] < before["n_quads"][1] and not (before["quads"][0][:before["n_quads"][0]] == 25).any()
    K, before, after = run(det, [l], [[24, 25]], point_status=[words])  # a seed names a slot that is not listed
    assert before["status"][0] == INPUT and before["n_quads"][0] == 0
    check_frame("an unlisted seed", l, [24, 25], K, before, 0, point_status=words.view(np.uint32))
    n = int(A.init_quads_tail(l, seeds[0])[2])
    K, before, after = run(det, [l, l], seeds, q=n)  # exactly the rows, then one row short
    assert list(before["status"]) == [FOUND, FOUND]
    check_all(["cap = the count"] * 2, [l, l], seeds, K, before, after, q=n)
    K, before, after = run(det, [l, l], seeds, q=n - 1)
    assert list(before["status"]) == [CAPACITY, CAPACITY] and list(before["n_quads"]) == [n, n] and (before["quads"] == SENT).all()
    check_all(["cap = the count - 1"] * 2, [l, l], seeds, K, before, after, q=n - 1)
    # a frame table instead of counts: two lists back to back in one flat array, the second entry with an overflow bit in a third
    l9 = BC.lattice(9, 9)
    flat = np.concatenate([np.zeros((3, 5), np.float32), l, l9])
    table = np.array([[49, 3, 0, 0], [81, 52, 0, 0], [49, 3, 2, 0]], np.int32)
    sd = np.array([[24], [40], [24]], np.int32)
    i32 = dict(dtype=torch.int32, device="cuda")
    w7, w9 = A.init_quads_tail(l, [24]), A.init_quads_tail(l9, [40])

    def table_pass(d, host_only):
        out = dict(quads=torch.full((3, Q, 4), SENT, **i32), quad_points=torch.full((3, Q, 4, 2), -7.0, dtype=torch.float32, device="cuda"),
                   n_quads=torch.full((3,), SENT, **i32), status=torch.full((3,), SENT, **i32), seed_quad_counts=torch.full((3, 1), SENT, **i32),
                   seeds_out=torch.full((3, 1), SENT, **i32), n_seeds_out=torch.full((3,), SENT, **i32))
        d.init_quads_enqueue(dev(flat), seed_saddles=dev(sd), frame_table=dev(table), **out)
        d.sync()
        pending = out["status"].cpu().numpy() == PENDING
        assert pending.all() if host_only else not pending.any()  # (without the device tail the kernel read no table)
        d.init_quads_fetch()
        res = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.float32).copy() for k, v in out.items()}
        quads, nq, st = res["quads"], res["n_quads"], res["status"]
        assert list(st) == [FOUND, FOUND, INPUT] and list(nq) == [w7[2], w9[2], 0]
        assert quads[0, :w7[2]].tobytes() == w7[0].tobytes() and quads[1, :w9[2]].tobytes() == w9[0].tobytes()
        assert (quads[2] == SENT).all() and (quads[0, w7[2]:] == SENT).all()
        assert (res["quad_points"][2] == np.float32(-7.0)).all() and res["seed_quad_counts"][2, 0] == SENT and res["seeds_out"][2, 0] == SENT
        assert res["n_seeds_out"][2] == 0
        return res

    first = table_pass(det, False)
    # the same batch without the device tail: the fetch's host form answers all three, the overflow entry included
    d0 = A.TagDetector("t36h11", None, device=0)
    try:
        d0.set_option("device_tail", 0)
        second = table_pass(d0, True)
        assert d0.get_option("last_init_quads_handed_back") == 3
    finally:
        d0.close()
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)


def test_more_rows_than_the_kernels_own_list(det):
    """More than 1024 rows of one frame (the kernel keeps that many until the count is known): listed a second time, straight to
    the caller's rows; one row short of the count is still AGX_BOARD_CAPACITY with no row."""
    l = BC.lattice(13, 13)
    seeds = [list(range(169))]
    n = int(A.init_quads_tail(l, seeds[0], cap=8192)[2])
    assert n > 1024
    for q in (n, n - 1):
        K, before, after = run(det, [l], seeds, q=q)
        assert before["status"][0] == (FOUND if q == n else CAPACITY) and before["n_quads"][0] == n
        check_all(["13x13, every saddle a seed"], [l], seeds, K, before, after, q=q)


# ---- 8: the rows go unfetched into agx_grow_boards_enqueue ---------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.3, 1.5])
def test_candidates_feed_grow_boards_on_the_same_stream(det, ratio):
    import torch
    tags = 4
    l = gapped_lattice(tags)
    m = 2 * tags
    seeds = np.array([[0, m + 1, 2 * m + 2]], np.int32)
    i32 = dict(dtype=torch.int32, device="cuda")
    s = dev(l[None])
    cand, ncand, cst = torch.full((1, Q, 4), SENT, **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
    quads, nq, bst = torch.full((1, 128, 4), SENT, **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
    scores, best = torch.zeros((1, Q), **i32), torch.zeros(1, **i32)
    det.init_quads_enqueue(s, cand, ncand, cst, seed_saddles=dev(seeds))
    det.grow_boards_enqueue(s, cand, quads, nq, bst, seed_counts=ncand, spacing_ratio=ratio, seed_scores=scores, best_seed=best)
    det.sync()
    assert int(cst.cpu()[0]) == FOUND and int(bst.cpu()[0]) == FOUND  # (neither kernel handed the lattice back)
    det.grow_boards_fetch()
    hq, hst, hn, _, _ = A.init_quads_tail(l, seeds[0])
    assert hst == FOUND and int(ncand.cpu()[0]) == hn and cand.cpu().numpy().view(np.uint32)[0, :hn].tobytes() == hq.tobytes()
    gq, gst, gn, gsc, gbest = A.grow_board_tail(l, hq, spacing_ratio=ratio, cap=128)
    assert gst == FOUND and int(nq.cpu()[0]) == gn and quads.cpu().numpy().view(np.uint32)[0, :gn].tobytes() == gq.tobytes()
    assert scores.cpu().numpy().view(np.uint32)[0, :hn].tobytes() == gsc.tobytes() and int(best.cpu()[0]) == gbest
    assert gn == tags * tags if ratio == 1.5 else gn < tags * tags  # (the whole board only at the ratio of its gaps)


# ---- 9: find_boards_staged -----------------------------------------------------------------------------------------------------
def test_find_boards_staged_is_find_boards_at_the_reference_ratio(det):
    import torch
    from tests.test_find_boards_cpu import GPU_FIRST, GPU_SIZE
    frames, _ = synth_module().render_batch(GPU_FIRST, 1, *GPU_SIZE, device="cuda")
    d_saddles = torch.zeros((2048, 5), dtype=torch.float32, device="cuda")
    d_table = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    det.saddles_batch_enqueue_to(frames, d_saddles, d_table)
    det.sync()
    table = d_table.cpu().numpy()
    assert not (table[:, 2] & 7).any()
    lists = [d_saddles.cpu().numpy()[table[0, 1]:table[0, 1] + table[0, 0]].copy()] + [as_list(golden_list(name)) for name in ALL_IMAGES]
    lists.append(BC.lattice(7, 7)[:0])
    S = max(len(l) for l in lists) + 1
    batch = np.full((len(lists), S, 5), np.nan, np.float32)
    for f, l in enumerate(lists):
        batch[f, :len(l)] = l
    s, counts = dev(batch), dev(np.array([len(l) for l in lists], np.int32))
    det.find_boards_enqueue(s, counts=counts)
    want = det.find_boards_fetch()
    got = det.find_boards_staged(s, 0.3, counts=counts)
    assert (want[3][:-1] == FOUND).all() and want[3][-1] == NONE
    for a, b, what in zip(got, want, ("quads", "quad points", "counts", "statuses")):
        assert a.tobytes() == b.tobytes(), what


def test_find_boards_staged_finds_the_widely_spaced_board(det):
    tags = 4
    l = gapped_lattice(tags)
    s = dev(l[None])
    det.find_boards_enqueue(s)
    fixed = det.find_boards_fetch()
    got = det.find_boards_staged(s, 1.5)
    assert fixed[3][0] == FOUND and fixed[2][0] < tags * tags  # the literal 0.3: a quad or a few, never the board
    assert got[3][0] == FOUND and got[2][0] == tags * tags
    m = 2 * tags
    cells = {frozenset(int(i) for i in q) for q in got[0][0, :got[2][0]]}
    assert cells == {frozenset((2 * r * m + 2 * c, 2 * r * m + 2 * c + 1, (2 * r + 1) * m + 2 * c, (2 * r + 1) * m + 2 * c + 1))
                     for r in range(tags) for c in range(tags)}


# ---- 10: batch state -----------------------------------------------------------------------------------------------------------
def test_batch_state_rules(det):
    import torch
    lib, h = det._lib, det._h
    l = BC.lattice(7, 7)
    assert lib.agx_init_quads_fetch(h, 1) == AGX_ERR_STATE  # nothing in flight
    frames = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    pts = torch.full((1, 4, 2), 20.0, dtype=torch.float32, device="cuda")
    det.refine_points_enqueue(frames, pts)
    K, before, _ = run(det, [l], [[24]], fetch=False)  # replaces the refine batch without waiting
    assert before["status"][0] == FOUND
    assert lib.agx_refine_points_fetch(h, None, None) == AGX_ERR_STATE
    assert lib.agx_find_boards_fetch(h, None, None, None, None, 1) == AGX_ERR_STATE
    assert lib.agx_grow_boards_fetch(h, 1) == AGX_ERR_STATE
    # refused arguments leave the batch in flight
    i32 = dict(dtype=torch.int32, device="cuda")
    s, sd = dev(l[None]), dev(np.array([[24]], np.int32))
    quads, nq, st = torch.zeros((1, Q, 4), **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
    for bad in (0, 1, 65):
        with pytest.raises(A.AgxError) as e:
            det.init_quads_enqueue(s, quads, nq, st, seed_saddles=sd, n_nearest=bad)
        assert e.value.status == AGX_ERR_ARG
    args = [h, s.data_ptr(), 20, 1, 49, None, None, None, sd.data_ptr(), 1, None, 50, Q, quads.data_ptr(), None, nq.data_ptr(), st.data_ptr(), None, None, None]
    assert lib.agx_init_quads_enqueue(*args) == AGX_OK and lib.agx_init_quads_fetch(h, 1) == AGX_OK
    K, before, _ = run(det, [l], [[24]], fetch=False)
    for i, v in ((1, None), (2, 18), (3, 0), (4, 0), (9, 0), (11, 1), (11, 65), (12, 0), (13, None), (15, None), (16, None), (5, nq.data_ptr()),
                 (8, None)):
        a = list(args)
        a[i] = v
        if i == 5:
            a[6] = nq.data_ptr()  # both d_counts and d_frame_table
        if i == 8:
            a[10] = nq.data_ptr()  # d_seed_counts without d_seed_saddles
        assert lib.agx_init_quads_enqueue(*a) == AGX_ERR_ARG, "argument %d" % i
    assert lib.agx_init_quads_fetch(h, 1) == AGX_OK  # still there
    assert lib.agx_init_quads_fetch(h, 1) == AGX_ERR_STATE
