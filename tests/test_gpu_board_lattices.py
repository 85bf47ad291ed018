"""k_find_boards on the hand-built lists of tests/board_cases.py: exact lattices, other index orders, coincident saddles,
saddles on a 3-NN query's radius, lattices at the white-block thresholds, lists around TN, BCELLS, BGR, TCAND and TA3.

The reference is the host form agx_find_board_tail on the same list -- status, count, every quad and the order --, which
tests/test_board_cases_cpu.py compares with the oracle on every one of these lists.  What keeps this from comparing the host form
with itself is read from the statuses BEFORE the fetch: a frame the kernel handed back is AGX_BOARD_PENDING there, and every
"device" case, the small side of every limit pair, three quarters of the whole table and all of families 1-4 must not be."""
import numpy as np
import pytest

from tests import board_cases as B
from tests.util import bits_equal

pytestmark = pytest.mark.gpu

FOUND, NONE, CAPACITY, INPUT, PENDING = 0, 1, 2, 3, 4
Q = 240  # rows per frame: the 32 x 32 lattice has 240 quads
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def table():
    """Every case's list and the host form's answer, computed once: name -> (list, (quads, status, n))."""
    import aprilgrid_rs_amd as A
    out = {}
    for c in B.CASES:
        l = B.build(c.name)
        out[c.name] = (l, A.find_board_tail(l, cap=1024))
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(det, lists, q=Q, slots=None):
    """One batch of the lists, padded with NaN behind each count, into caller-owned arrays filled with a sentinel ->
    (statuses before the fetch, handed back, quads, quad points, counts, statuses after it).  slots: the list's saddle i sits
    in slot slots[f][i] of a frame whose other slots hold decoys marked unused (point_status), without counts."""
    import torch
    n = len(lists)
    if slots is None:
        S = max(len(l) for l in lists) + 3
        batch = np.full((n, S, 5), np.nan, np.float32)
        for f, l in enumerate(lists):
            batch[f, :len(l)] = l
        kw = {"counts": dev(np.array([len(l) for l in lists], np.int32))}
    else:
        S = max(int(s.max()) for s in slots) + 2
        batch = np.zeros((n, S, 5), np.float32)
        pst = np.full((n, S), 2, np.int32)  # unused slots: decoys, copies of the list's own saddles (would tie with them if read)
        for f, (l, s) in enumerate(zip(lists, slots)):
            batch[f] = l[np.arange(S) % len(l)]
            batch[f, s] = l
            pst[f, s] = 0
        kw = {"point_status": dev(pst)}
    d_quads = torch.full((n, q, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d_pts = torch.full((n, q, 4, 2), -7.0, dtype=torch.float32, device="cuda")
    d_n = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    det.find_boards_enqueue(dev(batch), quads=d_quads, quad_points=d_pts, n_quads=d_n, status=d_st, **kw)
    det.sync()
    before = d_st.cpu().numpy().copy()
    det.find_boards_fetch()
    back = det.get_option("last_find_boards_handed_back")
    assert det.get_option("last_find_boards_frames") == n
    return before, back, d_quads.cpu().numpy().view(np.uint32), d_pts.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()


def check_frame(what, l, ref, quads, pts, n, st, q=Q, slots=None):
    rq, rst, rn = ref
    if rst == FOUND and rn > q:
        assert (int(st), int(n)) == (CAPACITY, rn), "%s: status %d count %d, host CAPACITY %d" % (what, st, n, rn)
        assert (quads == SENTINEL).all() and (pts == np.float32(-7.0)).all(), what + ": a row was written"
        return
    assert (int(st), int(n)) == (rst, rn), "%s: status %d count %d, host %d %d" % (what, st, n, rst, rn)
    want = rq.astype(np.int64) if slots is None else slots[rq.astype(np.int64)]
    assert np.array_equal(quads[:rn].astype(np.int64), want.reshape(-1, 4)), what + ": quads or their order"
    assert (quads[rn:] == SENTINEL).all() and (pts[rn:] == np.float32(-7.0)).all(), what + ": a row beyond the count was written"
    if rn:
        xy = l[rq.astype(np.int64)][:, :, :2]  # the list's x, y at the quad's indices
        assert bits_equal(pts[:rn], xy), what + ": quad points"


def check_all(names, table, res, q=Q, slots=None):
    before, back, quads, pts, n, st = res
    assert back == int((before == PENDING).sum())
    assert not (st == PENDING).any()
    for f, name in enumerate(names):
        check_frame(name, table[name][0], table[name][1], quads[f], pts[f], n[f], st[f], q, None if slots is None else slots[f])


NAMES = [c.name for c in B.CASES]


def test_every_list_is_answered_as_the_host_form_answers_and_mostly_by_the_kernel(det, table):
    res = run(det, [table[n][0] for n in NAMES])
    before = res[0]
    pending = {n: bool(before[f] == PENDING) for f, n in enumerate(NAMES)}
    for c in B.CASES:
        if c.expect != "device":
            print("before the fetch: %-50s %s" % (c.name, "PENDING (handed back)" if pending[c.name] else "answered by the kernel"))
    fam = {f: (sum(not pending[c.name] for c in B.CASES if c.family == f), sum(c.family == f for c in B.CASES)) for f in B.FAMILIES}
    total = sum(a for a, _ in fam.values())
    print("answered by the kernel: " + ", ".join("family %d: %d of %d" % (f, a, m) for f, (a, m) in fam.items()) + "; all: %d of %d" % (total, len(NAMES)))
    check_all(NAMES, table, res)
    late = [c.name for c in B.CASES if c.expect == "device" and pending[c.name]]
    assert not late, "handed back although the kernel must answer them: %s" % late
    for what, small, large in B.PAIRS:
        assert not any(pending[n] for n in small), (what, [n for n in small if pending[n]])
        assert all(pending[n] for n in large), (what, [n for n in large if not pending[n]])
    assert 4 * total >= 3 * len(NAMES)
    for f in (1, 2, 3, 4):
        assert fam[f][0] == fam[f][1], "family %d" % f
    # a second enqueue of the same batch, and the batch in reversed order: the same bytes per case (memo tables and the waves'
    # LDS are reused between the frames of a workgroup's lifetime)
    again = run(det, [table[n][0] for n in NAMES])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res[2:], again[2:])) and np.array_equal(res[0], again[0])
    rev = run(det, [table[n][0] for n in NAMES[::-1]])
    assert np.array_equal(rev[0][::-1], res[0])
    for a, b in zip(res[2:], rev[2:]):
        assert a.tobytes() == b[::-1].tobytes()


SHORT = ["lattice 13x13", "lattice 12x12", "lattice 32x32", "lattice 13x13 perm 3", "lattice 7x7", "lattice 2x2", "lattice 19x19"]


@pytest.mark.parametrize("q", [239, 35, 36])
def test_rows_one_short_is_capacity_with_the_true_count_and_no_row(det, table, q):
    """239: the 32 x 32 lattice's 240 quads (a frame the host form answers); 35: the 13 x 13 lattice's 36, from the kernel."""
    res = run(det, [table[n][0] for n in SHORT], q=q)
    check_all(SHORT, table, res, q=q)
    st, n = res[5], res[4]
    assert st[2] == CAPACITY and n[2] == 240
    assert (st[0], n[0], st[3], n[3]) == ((CAPACITY, 36, CAPACITY, 36) if q == 35 else (FOUND, 36, FOUND, 36))
    assert res[0][0] != PENDING and res[0][3] != PENDING  # (the 13 x 13 lattices' answer, CAPACITY included, is the kernel's)
    assert st[1] == FOUND and st[5] == NONE


def test_through_slot_maps_ties_follow_the_list_not_the_slots(det, table):
    """Every other slot unused and holding a copy of a listed saddle; the listed ones at scattered slots in the list's order.
    The answer is the host form's on the compacted list, mapped back through the slots."""
    names = [c.name for c in B.CASES if c.family in (2, 3, 4)] + ["lattice 7x7 doubled", "lattice 9x9 rot 30", "lattice 12x12", "lattice 2x2"]
    rng = np.random.default_rng(9)
    lists = [table[n][0] for n in names]
    P = 2 * max(len(l) for l in lists) + 8
    slots = []
    for i, l in enumerate(lists):
        s = 2 * np.arange(len(l)) + 1 if i % 2 else np.sort(rng.choice(P - 2, len(l), replace=False))  # (ascending: slot order is list order)
        slots.append(s.astype(np.int64))
    res = run(det, lists, slots=slots)
    check_all(names, table, res, slots=slots)
    assert not (res[0] == PENDING).any()
