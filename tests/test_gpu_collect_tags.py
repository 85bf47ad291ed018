"""agx_collect_tags_enqueue (k_collect_tags) and TagDetector.detect_staged on the GPU: the rounds of max_num_of_boards
(reference src/detector.rs:510-539) behind the staged chain.

The yardstick of the kernel is the host form, agx_collect_tags_tail, byte for byte (tests/test_collect_tags_cpu.py holds that
to a dict insert loop); of detect_staged the host loop find_board_tail -> decode_quads_tail -> collect_tags over the filtered
records and status words the device stages produced, and agx_detect_batch on the same pixels."""
import numpy as np
import pytest

from tests.test_collect_tags_cpu import (B_CAPACITY, B_INPUT, FOUND, NONE, PENDING, T_CAPACITY, T_INPUT, T_OK, T_PENDING, TAG, USED,
                                         host_rounds, make_round)
from tests.util import bits_equal, load_image, synth_module

import aprilgrid_rs_amd as A

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
SENT = 0x7E7E7E7E
MARGIN = 64  # sentinel words in front of and behind every output
N, Q, S, T = 9, 130, 600, 40
SW, SH = 320, 240


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(payload):
    """A device copy of an int32 / uint32 array between two sentinel margins -> (the whole tensor, the payload's view)."""
    import torch
    flat = np.full(payload.size + 2 * MARGIN, SENT, np.uint32)
    flat[MARGIN:MARGIN + payload.size] = payload.reshape(-1).view(np.uint32)
    whole = torch.from_numpy(flat.view(np.int32)).cuda()
    return whole, whole[MARGIN:MARGIN + payload.size].view(*payload.shape)


def margins_intact(whole):
    a = whole.cpu().numpy().view(np.uint32)
    return (a[:MARGIN] == SENT).all() and (a[-MARGIN:] == SENT).all()


# ---- 1. a synthetic batch against the host form ------------------------------------------------------------------------------
def synthetic_rounds():
    """Two rounds of a 9-frame batch -> per round (quads [N,Q,4], n_quads [N], board_status [N], quad_tags [N,Q], quad_status [N,Q])."""
    rng = np.random.default_rng(2024)

    def frame(n, pool, decoded=0.7):
        ids = rng.choice(pool, n) if n else np.zeros(0, np.int64)
        st = np.where(rng.random(n) < decoded, 0, rng.integers(1, 6, n))
        slots = rng.integers(0, S, (n, 4))
        return ids, st, slots

    pool = np.arange(50, 80)  # 30 ids: a frame of these never needs more than 30 rows
    rounds = []
    for r in range(2):
        quads = np.full((N, Q, 4), SENT, np.uint32)   # beyond a frame's count: slot numbers that are never looked at
        n_quads = np.zeros(N, np.uint32)
        bstatus = np.full(N, FOUND, np.uint32)
        qtags = np.zeros((N, Q), TAG)
        qtags.view(np.uint32)[:] = SENT
        qstatus = np.zeros((N, Q), np.uint32)         # ... and statuses that say "decoded"
        for f in range(N):
            if r == 0:
                n = [0, 1, 63, 64, 65, 129, 130, 50, 45][f]
                ids, st, slots = frame(n, pool)
                if f == 1:
                    st[:] = 0
                if f == 4:
                    st[7], slots[7, 2] = 0, S - 1          # slot 599 is accepted
                if f == 5:
                    st[100], ids[100] = 0, 586             # id 586 is accepted
                if f == 6:
                    st[[0, 63, 64, 129]] = 0
                    ids[63] = ids[64] = 301                # duplicates across the boundary of a pass of 64 ...
                    ids[0] = ids[129] = 302                # ... and as far apart as a frame allows
                if f == 7:                                 # reaches row 40 exactly
                    st[:] = 0
                    ids = np.concatenate([np.arange(400, 440), np.arange(400, 410)])
                    rng.shuffle(ids)
                if f == 8:                                 # needs row 41
                    st[:] = 0
                    ids = np.concatenate([np.arange(400, 441), np.arange(400, 404)])
                    rng.shuffle(ids)
            else:
                n = [5, 5, 200, 5, 20, 20, 90, 12, 30][f]
                ids, st, slots = frame(min(n, Q), pool)
                if f == 0:
                    bstatus[f] = NONE
                if f == 1:
                    bstatus[f] = PENDING
                if f == 2:
                    bstatus[f] = B_CAPACITY                # (the true count, above quads_per_frame, and no row)
                if f == 3:
                    bstatus[f] = B_INPUT
                if f == 4:
                    st[11], slots[11, 0] = 0, S            # slot 600 is refused
                if f == 5:
                    st[3], ids[3] = 0, 587                 # id 587 is refused
                if f == 6:                                 # ids of round 1 again, and new ones
                    ids[:45] = rng.choice(pool, 45)
                    ids[45:] = rng.choice(np.arange(500, 508), len(ids) - 45)
                    st[[0, 50, 89]] = 0
                    ids[89] = 301
                if f == 7:                                 # one new id on a full table
                    st[:] = 0
                    ids = np.concatenate([np.arange(405, 416), [7]])
            n_quads[f] = n
            k = len(ids)
            quads[f, :k], qstatus[f, :k] = slots, st
            qstatus[f, k:] = 0
            for q in range(k):
                if st[q] == 0:
                    qtags["id"][f, q] = ids[q]
                    qtags["xy"][f, q] = rng.uniform(0, 1000, 8).astype(np.float32)
                else:
                    qtags.view(np.uint32).reshape(N, Q, 9)[f, q] = 0  # as the decode leaves a quad that is not decoded
        rounds.append((quads, n_quads, bstatus, qtags, qstatus))
    return rounds


def expected(rounds, words0, mark=True):
    """The host form, frame by frame and round by round -> (rows [N,T] with sentinels beyond the counts, counts, statuses, words)."""
    rows = np.zeros((N, T), TAG)
    rows.view(np.uint32)[:] = SENT
    counts, status, words = np.zeros(N, np.uint32), np.zeros(N, np.uint32), words0.copy()
    for quads, n_quads, bstatus, qtags, qstatus in rounds:
        for f in range(N):
            k = int(n_quads[f]) if bstatus[f] == FOUND else 0
            assert k <= Q
            rows[f], counts[f], status[f], w = A.collect_tags("t36h11", quads[f, :k], bstatus[f], qtags[f, :k], qstatus[f, :k], S,
                                                              words[f] if mark else None, rows[f], counts[f], status[f], T)
            if mark:
                words[f] = w
    return rows, counts, status, words


def run_device(det, rounds, d_words, frame_table=None):
    tags_w, tags = guarded(np.full((N, T, 9), SENT, np.uint32))
    ntags_w, ntags = guarded(np.full(N, SENT, np.uint32))  # (reset: what the arrays hold before the first round does not matter)
    tst_w, tst = guarded(np.full(N, SENT, np.uint32))
    for r, (quads, n_quads, bstatus, qtags, qstatus) in enumerate(rounds):
        det.collect_tags_enqueue(dev(quads.view(np.int32)), dev(n_quads.view(np.int32)), dev(bstatus.view(np.int32)),
                                 dev(qtags.view(np.int32).reshape(N, Q, 9)), dev(qstatus.view(np.int32)), d_words, tags, ntags, tst,
                                 reset=r == 0, frame_table=frame_table, saddles_per_frame=S if d_words is None else None)
    det.sync()
    for w in (tags_w, ntags_w, tst_w):
        assert margins_intact(w)
    return (tags.cpu().numpy().view(np.uint32).reshape(N, T * 9).view(TAG).reshape(N, T), ntags.cpu().numpy().view(np.uint32),
            tst.cpu().numpy().view(np.uint32))


def words_before():
    return np.random.default_rng(7).integers(0, 5, (N, S)).astype(np.uint32)  # AGX_POINT_REFINED .. AGX_POINT_FILTERED


def test_synthetic_batch_equals_the_host_form(det):
    rounds = synthetic_rounds()
    words0 = words_before()
    want_rows, want_n, want_st, want_words = expected(rounds, words0)
    # the cases the batch is there for
    assert list(want_st) == [T_OK, T_PENDING, T_INPUT, T_INPUT, T_INPUT, T_INPUT, T_OK, T_CAPACITY, T_CAPACITY]
    assert want_n[7] == 41 and want_n[8] == 41 and want_n[6] > 30 and want_n[0] == 0 and want_n[1] == 1
    after_one = expected(rounds[:1], words0)
    assert list(after_one[2][:8]) == [T_OK] * 8 and after_one[1][7] == 40 and after_one[3][4, S - 1] == USED
    assert 586 in after_one[0]["id"][5, :after_one[1][5]]
    assert (want_words[8] == words0[8]).all()  # no word of a frame that never held a row
    words_w, words = guarded(words0)
    got_rows, got_n, got_st = run_device(det, rounds, words)
    assert margins_intact(words_w)
    assert np.array_equal(got_st, want_st) and np.array_equal(got_n, want_n)
    assert got_rows.tobytes() == want_rows.tobytes()  # rows below the counts, and the sentinels beyond them
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want_words)
    # the same batch through a frame table: offsets that are no multiple of 600, frames in shuffled order
    perm = np.random.default_rng(3).permutation(N)
    table = np.zeros((N, 4), np.uint32)
    table[:, 0], table[:, 1] = S, perm * 613 + 7
    flat = np.full(N * 613 + 20, SENT, np.uint32)
    for f in range(N):
        flat[table[f, 1]:table[f, 1] + S] = words0[f]
    flat_w, d_flat = guarded(flat)
    got = run_device(det, rounds, d_flat, frame_table=dev(table.view(np.int32)))
    assert margins_intact(flat_w)
    assert np.array_equal(got[2], want_st) and np.array_equal(got[1], want_n) and got[0].tobytes() == want_rows.tobytes()
    flat_after = d_flat.cpu().numpy().view(np.uint32)
    want_flat = flat.copy()
    for f in range(N):
        want_flat[table[f, 1]:table[f, 1] + S] = want_words[f]
    assert np.array_equal(flat_after, want_flat)  # the gaps between the frames' words included
    # a table entry bounds the slot numbers by its count: one short of the largest slot a frame uses
    table2 = table.copy()
    table2[6, 0] = int(max(rounds[0][0][6, q].max() for q in range(Q) if rounds[0][4][6, q] == 0))
    got = run_device(det, rounds[:1], dev(flat.view(np.int32)), frame_table=dev(table2.view(np.int32)))
    assert got[2][6] == T_INPUT and got[1][6] == 0 and list(got[2][:6]) == [T_OK] * 6
    # without point_status: the same tables, nothing marked
    want_rows, want_n, want_st, _ = expected(rounds, words0, mark=False)
    got = run_device(det, rounds, None)
    assert np.array_equal(got[2], want_st) and np.array_equal(got[1], want_n) and got[0].tobytes() == want_rows.tobytes()


def test_a_found_count_above_quads_per_frame_is_tags_input(det):
    """The one cause of AGX_TAGS_INPUT the host form cannot be given: its n_quads is the length of its arrays."""
    rng = np.random.default_rng(5)
    quads, qtags, qstatus = make_round(rng, [1, 2, 3, 4], n_slots=S)
    words_w, words = guarded(np.zeros((2, S), np.uint32))
    tags_w, tags = guarded(np.full((2, T, 9), SENT, np.uint32))
    ntags, tst = dev(np.zeros(2, np.int32)), dev(np.zeros(2, np.int32))
    two = lambda a: dev(np.stack([a, a]).view(np.int32))
    det.collect_tags_enqueue(two(quads), dev(np.array([5, 4], np.int32)), dev(np.zeros(2, np.int32)), two(qtags.view(np.uint32).reshape(4, 9)),
                             two(qstatus), words, tags, ntags, tst, reset=True)
    det.sync()
    assert list(tst.cpu().numpy()) == [T_INPUT, T_OK] and list(ntags.cpu().numpy()) == [0, 4]
    w = words.cpu().numpy()
    assert not w[0].any() and (w[1] == USED).sum() == len(np.unique(quads))
    t = tags.cpu().numpy().view(np.uint32)
    assert (t[0] == SENT).all() and (t[1, 4:] == SENT).all() and margins_intact(tags_w) and margins_intact(words_w)


# ---- 2. detect_staged ------------------------------------------------------------------------------------------------------
def stages_for_the_host_loop(d, frames, cpf=4096):
    """The stages in front of the rounds, as detect_staged runs them -> (records [n, cpf, 5], status words, counts) on the host."""
    import torch
    n, h, w = frames.shape[:3]
    blur = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    resp = torch.empty_like(blur)
    i32 = dict(dtype=torch.int32, device="cuda")
    rows, pts = torch.zeros((n, cpf, 4), **i32), torch.zeros((n, cpf, 2), dtype=torch.float32, device="cuda")
    counts, cstatus = torch.zeros(n, **i32), torch.zeros(n, **i32)
    records, pstatus = torch.zeros((n, cpf, 5), dtype=torch.float32, device="cuda"), torch.zeros((n, cpf), **i32)
    d.planes_enqueue(frames, d.blur_sigma, blur=blur, response=resp)
    d.clusters_enqueue(resp, clusters=rows, points=pts, counts=counts, status=cstatus)
    d.refine_points_enqueue(blur, pts, counts=counts, out=records, status=pstatus, image="plane", half_size_patch=d.half_size_patch)
    d.filter_saddles_enqueue(records, pstatus, counts=counts)
    d.sync()
    assert not cstatus.cpu().numpy().any()
    return (records, pstatus, counts), records.cpu().numpy(), pstatus.cpu().numpy().view(np.uint32), counts.cpu().numpy()


def check_staged(d, frames, what):
    """detect_staged against the host loop on the device's own filtered records (exact) and against detect_batch.
    -> (detect_staged's result, the frames that differ from detect_batch)."""
    got = d.detect_staged(frames)
    _, records, words, counts = stages_for_the_host_loop(d, frames)
    host = frames.cpu().numpy()
    rounds = d.detector_params.max_num_of_boards
    assert rounds == 2
    for f in range(len(host)):
        c = int(counts[f])
        rows, status, _ = host_rounds(records[f, :c], words[f, :c], A.TagDetector.luma8(host[f]), rounds)
        assert status == T_OK
        assert list(got[f]) == [int(t) for t in rows["id"]], "%s frame %d: ids or their order against the host loop" % (what, f)
        for i, t in enumerate(got[f]):
            assert bits_equal(got[f][t], rows["xy"][i].reshape(4, 2)), "%s frame %d: corners of tag %d" % (what, f, t)
    ref = d.detect_batch(host)
    differ = []
    for f in range(len(host)):
        same = sorted(got[f]) == sorted(ref[f]) and all(bits_equal(got[f][t], ref[f][t]) for t in got[f])
        if not same:
            differ.append(f)
            print("%s frame %d: detect_staged %d tags, detect_batch %d" % (what, f, len(got[f]), len(ref[f])))
    return got, differ


@pytest.fixture(scope="module")
def synthetic(det):
    frames, _ = synth_module().render_batch(40, 4, SW, SH, device="cuda")
    got, differ = check_staged(det, frames, "synthetic")
    return frames, got, differ


def test_detect_staged_on_two_boards(det):
    import torch
    img = load_image("two_boards.png")
    assert img.shape == (1080, 1920, 3) and img.dtype == np.uint8  # ImageRgb8: the stages take it as it is
    got, differ = check_staged(det, torch.from_numpy(img)[None].cuda(), "two_boards.png")
    assert len(got[0]) == 72 and not differ
    one = A.DetectorParams.default_params()
    one.max_num_of_boards = 1
    d1 = A.TagDetector("t36h11", one, device=0)
    try:
        assert len(d1.detect_staged(torch.from_numpy(img)[None].cuda())[0]) == 36  # what the staged chain gave without the rounds
    finally:
        d1.close()


def test_detect_staged_on_synthetic_frames(synthetic):
    frames, got, differ = synthetic
    assert len(got) == 4 and all(len(g) > 4 for g in got)
    assert not differ, "frames %s differ from detect_batch" % differ


def test_detect_staged_names_the_frame_it_cannot_hold(det, synthetic):
    frames = synthetic[0]
    with pytest.raises(A.AgxError, match=r"frame 0: tag status AGX_TAGS_CAPACITY"):
        det.detect_staged(frames, tags_per_frame=2)
    with pytest.raises(A.AgxError, match=r"frame 0: tag status AGX_TAGS_INPUT"):
        det.detect_staged(frames, quads_per_frame=1)


# ---- 3. the rounds with nothing but the stream between them ------------------------------------------------------------------
def test_rounds_without_a_host_sync_between_them(det, synthetic):
    import torch
    frames, want, _ = synthetic
    n = frames.shape[0]
    (records, pstatus, counts), _, _, _ = stages_for_the_host_loop(det, frames)
    i32 = dict(dtype=torch.int32, device="cuda")
    quads, qpts = torch.zeros((n, 128, 4), **i32), torch.zeros((n, 128, 4, 2), dtype=torch.float32, device="cuda")
    nq, bst = torch.zeros(n, **i32), torch.zeros(n, **i32)
    qtags, qst = torch.zeros((n, 128, 9), **i32), torch.zeros((n, 128), **i32)
    tags, ntags, tst = torch.full((n, 64, 9), SENT, **i32), torch.full((n,), SENT, **i32), torch.full((n,), SENT, **i32)
    for r in range(2):
        det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
        det.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst)
        det.collect_tags_enqueue(quads, nq, bst, qtags, qst, pstatus, tags, ntags, tst, reset=r == 0)
    det.sync()
    tst, ntags = tst.cpu().numpy(), ntags.cpu().numpy()
    ids, xy = A.TagDetector.split_device_tags(tags)
    ids, xy = ids.cpu().numpy(), xy.cpu().numpy()
    assert set(tst) <= {T_OK, T_PENDING} and (tst == T_OK).any()
    for f in range(n):
        if tst[f] != T_OK:
            continue
        assert list(ids[f, :ntags[f]]) == list(want[f]), "frame %d" % f
        for i, t in enumerate(want[f]):
            assert bits_equal(xy[f, i], want[f][t]), "frame %d: corners of tag %d" % (f, t)
        assert (ids[f, ntags[f]:] == SENT).all()


# ---- 4. state and arguments ----------------------------------------------------------------------------------------------------
def test_state_and_argument_rules(det):
    import torch
    lib, h = det._lib, det._h
    rng = np.random.default_rng(9)
    quads, qtags, qstatus = make_round(rng, [1, 2, 3], n_slots=S)
    n, q = 2, 3
    two = lambda a: dev(np.stack([a] * n).view(np.int32))
    d_quads, d_qtags, d_qst = two(quads), two(qtags.view(np.uint32).reshape(q, 9)), two(qstatus)
    d_nq, d_bst = dev(np.full(n, q, np.int32)), dev(np.zeros(n, np.int32))
    d_words = dev(np.zeros((n, S), np.int32))
    d_table = dev(np.array([[S, 0, 0, 0], [S, S, 0, 0]], np.int32))
    d_tags, d_nt, d_ts = dev(np.zeros((n, T, 9), np.int32)), dev(np.zeros(n, np.int32)), dev(np.zeros(n, np.int32))
    good = [n, q, d_quads.data_ptr(), d_nq.data_ptr(), d_bst.data_ptr(), d_qtags.data_ptr(), d_qst.data_ptr(), S, None, d_words.data_ptr(),
            T, d_tags.data_ptr(), d_nt.data_ptr(), d_ts.data_ptr(), 1]
    frames = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    det.saddles_batch_enqueue(frames)
    bad = {"no frames": {0: 0}, "negative frames": {0: -1}, "no quads per frame": {1: 0}, "null quads": {2: None}, "null n_quads": {3: None},
           "null board status": {4: None}, "null quad tags": {5: None}, "null quad status": {6: None}, "no slots and no table": {7: 0},
           "no tags per frame": {10: 0}, "null tags": {11: None}, "null n_tags": {12: None}, "null tag status": {13: None},
           "misaligned quads": {2: d_quads.data_ptr() + 2}, "misaligned quad tags": {5: d_qtags.data_ptr() + 1},
           "misaligned words": {9: d_words.data_ptr() + 2}, "misaligned table": {8: d_table.data_ptr() + 2},
           "misaligned tags": {11: d_tags.data_ptr() + 2}, "misaligned tag status": {13: d_ts.data_ptr() + 1},
           "2^31 slots": {7: 1 << 30}, "2^31 tag rows": {10: 1 << 30}, "2^31 quad rows": {1: 1 << 30}}
    cnt2, st2 = np.zeros(2, np.uint32), np.zeros(2, np.int32)
    sad = np.zeros((2, 8, 5), np.float32)
    for what, change in bad.items():
        a = list(good)
        for i, v in change.items():
            a[i] = v
        assert lib.agx_collect_tags_enqueue(h, *a) == AGX_ERR_ARG, what
    assert lib.agx_collect_tags_enqueue(None, *good) == AGX_ERR_ARG
    res, st = det.saddles_batch_fetch()  # the saddle batch is still in flight
    assert len(res) == 2 and (st == 0).all()
    # no slots per frame is fine with a table, and the words may be missing
    det.saddles_batch_enqueue(frames)
    a = list(good)
    a[7], a[8] = 0, d_table.data_ptr()
    assert lib.agx_collect_tags_enqueue(h, *a) == AGX_OK
    # a good call replaced the batch, has no fetch of its own, and every kind's fetch is AGX_ERR_STATE
    assert lib.agx_saddles_batch_fetch(h, sad.ctypes.data, 8, cnt2.ctypes.data, st2.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_refine_points_fetch(h, sad.ctypes.data, cnt2.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_detect_batch_fetch(h, None, cnt2.ctypes.data, st2.ctypes.data, 0) == AGX_ERR_STATE
    assert lib.agx_decode_quads_fetch(h, None, None, None) == AGX_ERR_STATE
    assert lib.agx_find_boards_fetch(h, None, None, None, None, 0) == AGX_ERR_STATE
    assert lib.agx_clusters_fetch(h, None, None, cnt2.ctypes.data, cnt2.ctypes.data) == AGX_ERR_STATE
    a = list(good)
    a[9] = None
    assert lib.agx_collect_tags_enqueue(h, *a) == AGX_OK
    det.sync()
    assert list(d_nt.cpu().numpy()) == [3, 3] and not d_ts.cpu().numpy().any()
    w = d_words.cpu().numpy()  # marked by the call with the table (frame 1's words start at S there too), not by the one without words
    assert (w[0] == USED).sum() == (w[1] == USED).sum() == len(np.unique(quads))
    # the bindings' own checks
    with pytest.raises(A.AgxError):
        det.collect_tags_enqueue(d_quads, d_nq, d_bst, d_qtags, d_qst, None, d_tags, d_nt, d_ts)  # no bound for the slot numbers
    with pytest.raises(A.AgxError):
        det.collect_tags_enqueue(d_quads, d_nq, d_bst, d_qtags, d_qst, d_words, d_tags.float(), d_nt, d_ts)
