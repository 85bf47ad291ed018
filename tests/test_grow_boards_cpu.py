"""agx_grow_board_tail -- boards grown from caller-given seed quads at any spacing ratio (reference src/board.rs:26-112), the host
form -- against tests/board_grow_oracle.py, a numpy restatement of the crate's text that is itself pinned here against the
oracle's orc_try_find_best_board.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import board_cases as BC
from tests import board_grow_oracle as Y
from tests.test_find_boards_cpu import golden_list, yardstick as orc_find
from tests.util import ALL_IMAGES

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

F32 = np.float32
FAMILY_12 = [c.name for c in BC.CASES if c.family in (1, 2)]
FAMILY_1_BOARDS = [c.name for c in BC.CASES if c.family == 1 and c.quads is not None]

# The 7 x 7 lattice grown from the first quad of its board: the neighbour's corner is predicted at a + (b - a)(1 + ratio) and
# accepted within sqrt(0.5)|b - a| of the corner two spacings on, so the board is whole for 1 - sqrt(0.5) <= ratio <= 1 +
# sqrt(0.5) up to rounding.  Bisected with the yardstick (bisect_ratio below), never with the library: the float32 bits of the
# last ratio that still gives one quad at the lower end, and of the last that still gives nine at the upper end.
RATIO_THRESHOLDS = {"lower": 0x3E95F60D, "upper": 0x3FDA827A}
RATIO_STEPS = (0, 1, 10, 100)
# try_fix_missing changes the count: the 9 x 9 lattice with the theta of saddle 12 eight degrees off, grown from the first quad
# of the undisturbed lattice's board (found by a search with the yardstick over every interior saddle and 6 .. 10 degrees)
FIX_SADDLE, FIX_DTHETA = 12, 8.0


def as_list(s):
    return np.ascontiguousarray(np.ascontiguousarray(s).view(np.float32).reshape(-1, 5)) if s.dtype.names else np.ascontiguousarray(s, F32)


def ratio_values(which):
    lo = np.array([RATIO_THRESHOLDS[which]], np.uint32).view(np.float32)[0]
    hi = BC.f32_steps(lo, 1)
    return [BC.f32_steps(lo, -k) for k in RATIO_STEPS] + [BC.f32_steps(hi, k) for k in RATIO_STEPS]


def bisect_ratio(lo, hi):
    """-> the last float32 ratio with lo's quad count on lattice(7, 7) and its upper neighbour, by the yardstick."""
    l, seed = BC.lattice(7, 7), [Y.try_find_best_board(BC.lattice(7, 7))[0]]
    count = lambda r: Y.grow(l, seed, spacing_ratio=r)[2]
    lo, hi = F32(lo), F32(hi)
    want = count(lo)
    assert count(hi) != want
    while BC.f32_steps(lo, 1) != hi:
        mid = F32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = BC.f32_steps(lo, 1)
        lo, hi = (mid, hi) if count(mid) == want else (lo, mid)
    return lo, hi


def gapped_lattice(tags, side=24.0, gap=36.0, origin=(100.0, 60.0)):
    """tags x tags tags of `side` with true gaps of `gap` = 1.5 side between them: 2 tags x 2 tags saddles, row-major."""
    m = 2 * tags
    i = np.arange(m)
    p = (i // 2) * (side + gap) + (i % 2) * side
    r, c = np.mgrid[0:m, 0:m]
    out = np.zeros((m * m, 5), F32)
    out[:, 0] = (p[c] + origin[0]).ravel()
    out[:, 1] = (p[r] + origin[1]).ravel()
    out[:, 3] = np.where((r + c) % 2 == 0, F32(-45.0), F32(45.0)).ravel()
    return out


def first_tag_seed(l, tags):
    """The quad of the tag in the first row and column, in init_quads' corner order (from the yardstick's init_quads)."""
    m = 2 * tags
    return [q for q in Y.init_quads(Y.Yard(l), 0) if set(q) == {0, 1, m, m + 1}][:1]


def fix_list():
    l = BC.lattice(9, 9)
    seed = [Y.try_find_best_board(l)[0]]
    l[FIX_SADDLE, 3] += F32(FIX_DTHETA)
    return l, seed


def check(l, seeds, what="", **kw):
    """agx_grow_board_tail == the yardstick, byte for byte: rows, count, status, seed scores, best seed."""
    kw.setdefault("cap", 1024)
    want = Y.grow(l, seeds, **kw)
    got = A.grow_board_tail(l, seeds, **kw)
    assert got[1] == want[1] and got[2] == want[2], "%s: status %d count %d, yardstick %d %d" % (what, got[1], got[2], want[1], want[2])
    assert got[0].tobytes() == want[0].tobytes(), what + ": rows"
    assert (got[3] is None) == (want[3] is None) and (got[3] is None or got[3].tobytes() == want[3].tobytes()), what + ": seed scores"
    assert got[4] == want[4], what + ": best seed"
    return got


# ---- 1: the yardstick is the oracle's search ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL_IMAGES) + FAMILY_12)
def test_the_yardsticks_search_is_the_oracles(name):
    l = as_list(golden_list(name)) if name in ALL_IMAGES else BC.build(name)
    mine, ref = Y.try_find_best_board(l, 0.3), orc_find(l)
    if ref is None:
        assert mine is None
    else:
        assert mine is not None and np.array_equal(np.array(mine, np.int64).reshape(-1, 4), ref.astype(np.int64)), "quads or their order"


# ---- 2: every quad of the oracle's board as a seed --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL_IMAGES) + FAMILY_1_BOARDS)
def test_seeds_from_the_oracles_board(name):
    l = as_list(golden_list(name)) if name in ALL_IMAGES else BC.build(name)
    board = orc_find(l)
    assert board is not None and len(board)
    for i, q in enumerate(board):
        got = check(l, [q], "seed %d" % i, spacing_ratio=0.3)
        assert got[1] == _ffi.AGX_BOARD_FOUND and got[3][0] >= 1 and got[4] == 0
    check(l, board, "all seeds", spacing_ratio=0.3)
    check(l, board, "all seeds, stop 2", spacing_ratio=0.3, stop_score=2)
    got = check(l, board, "all seeds, stop at the board", spacing_ratio=0.3, stop_score=len(board), fix_missing=False)
    assert (got[3][got[4] + 1:] == 0).all()


# ---- 3: the ratio decides the board ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lower", "upper"])
def test_ratio_thresholds_of_the_7x7_lattice(which):
    l = BC.lattice(7, 7)
    seed = [Y.try_find_best_board(l)[0]]
    counts = [check(l, seed, "ratio %r" % float(r), spacing_ratio=r)[2] for r in ratio_values(which)]
    k = len(RATIO_STEPS)
    if which == "lower":
        assert counts[:k] == [1] * k and all(c > 1 for c in counts[k:]) and counts[-1] == 9, counts
    else:
        assert counts[:k] == [9] * k and all(c < 9 for c in counts[k:]) and counts[-1] == 1, counts


def test_the_recorded_thresholds_are_the_yardsticks():
    for which, (lo, hi) in (("lower", (0.2, 0.5)), ("upper", (1.5, 1.9))):
        last, _ = bisect_ratio(lo, hi)
        assert np.array([last], np.float32).view(np.uint32)[0] == RATIO_THRESHOLDS[which], which
    assert abs(float(ratio_values("lower")[0]) - (1 - np.sqrt(0.5))) < 1e-6 and abs(float(ratio_values("upper")[0]) - (1 + np.sqrt(0.5))) < 1e-6


def test_a_lattice_with_true_gaps_needs_its_own_ratio():
    # two by two tags: the search at 0.3 finds a lone quad (the prediction lands 28.8 from the next tag's corner, allowed 17)
    l = gapped_lattice(2)
    quads, status, n = A.find_board_tail(l)
    assert status == _ffi.AGX_BOARD_NONE or n == 1
    seed = first_tag_seed(l, 2)
    assert len(seed) == 1
    assert check(l, seed, "0.3", spacing_ratio=0.3)[2] == 1
    got = check(l, seed, "1.5", spacing_ratio=1.5)
    assert got[2] == 4 and got[3][0] == 4
    # three by three: with more saddles the search at 0.3 does chain a few quads (larger squares among them), but never the
    # nine tags; those are found at 1.5 only
    l = gapped_lattice(3)
    tags = {(2 * r * 6 + 2 * c) for r in range(3) for c in range(3)}
    quads, status, n = A.find_board_tail(l)
    assert n < 9 and set(quads.min(axis=1).tolist()) != tags
    seed = first_tag_seed(l, 3)
    assert check(l, seed, "0.3", spacing_ratio=0.3)[2] == 1
    got = check(l, seed, "1.5", spacing_ratio=1.5)
    assert got[2] == 9 and set(got[0].min(axis=1).tolist()) == tags


HUGE_RATIOS = (1e12, 3.2e38)  # the query point beyond any grid (the kernel then looks at every saddle), and beyond binary32


@pytest.mark.parametrize("ratio", HUGE_RATIOS)
def test_a_huge_finite_ratio_finds_nothing_beyond_the_seed(ratio):
    l = BC.lattice(7, 7)
    seed = [Y.try_find_best_board(l)[0]]
    with np.errstate(over="ignore", invalid="ignore"):  # (the yardstick's query point overflows to infinity at 3.2e38, as the library's)
        got = check(l, seed, "ratio %g" % ratio, spacing_ratio=ratio)
    assert got[1] == _ffi.AGX_BOARD_FOUND and got[2] == 1 and got[3].tolist() == [1]


# ---- 4: order rules ------------------------------------------------------------------------------------------------------------
def test_order_rules():
    l = BC.lattice(7, 7)
    board = Y.try_find_best_board(l)
    got = check(l, [board[3], board[5]], "equal scores")
    assert got[3].tolist() == [9, 9] and got[4] == 0
    got = check(l, board[:3], "stop at seed 0", stop_score=9)
    assert got[3].tolist() == [9, 0, 0] and got[4] == 0
    a, b = check(l, board[:3], "stop above every score", stop_score=10), check(l, board[:3], "no stop", stop_score=0)
    assert a[0].tobytes() == b[0].tobytes() and a[3].tolist() == b[3].tolist() == [9, 9, 9] and a[4] == b[4] == 0
    # a later seed wins only with a strictly higher score: a quad of the far 3 x 3 lattice first (score 1), then the board's
    both = np.concatenate([l, BC.lattice(3, 3, origin=(1500.0, 1500.0))])
    lone = orc_find(both[49:]) + 49
    got = check(both, [lone[0], board[0], board[1]], "a higher score later")
    assert got[3].tolist() == [1, 9, 9] and got[4] == 1 and got[2] == 9


# ---- 5: AGX_GROW_FIX_MISSING -----------------------------------------------------------------------------------------------------
def test_fix_missing_changes_the_board():
    l, seed = fix_list()
    on, off = Y.grow(l, seed, fix_missing=True), Y.grow(l, seed, fix_missing=False)
    assert on[5] >= 1 and on[2] == off[2] + 1  # (the yardstick: the fix list is not empty and one cell is mended)
    assert check(l, seed, "fix", fix_missing=True)[2] == on[2]
    assert check(l, seed, "no fix", fix_missing=False)[2] == off[2]
    for name in ("lattice 7x7", "lattice 9x9 rot 30"):
        l = BC.build(name)
        seed = [Y.try_find_best_board(l)[0]]
        assert check(l, seed, name, fix_missing=True)[0].tobytes() == check(l, seed, name, fix_missing=False)[0].tobytes()


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------
def raw(l, seeds, ratio=0.3, stop=0, flags=1, cap=64, point_status=None, guard=0xDEADBEEF, **null):
    """agx_grow_board_tail with guard words around every output -> (rc, quads, n, status, scores, best); asserts the guards."""
    l = np.ascontiguousarray(l, F32).reshape(-1, 5)
    s = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 4)
    quads = np.full((cap + 2) * 4, guard, np.uint32)
    scores = np.full(len(s) + 2, guard, np.uint32)
    one = np.full((3, 3), guard, np.uint32)  # rows: n_quads, status, best_seed, each between two guard words
    ps = None if point_status is None else np.ascontiguousarray(point_status, np.uint32)
    p = lambda a, off: a.ctypes.data + 4 * off
    rc = _ffi.lib().agx_grow_board_tail(None if null.get("no_saddles") else l.ctypes.data, len(l), None if ps is None else ps.ctypes.data,
                                        None if null.get("no_seeds") else s.ctypes.data, len(s), float(ratio), stop, flags,
                                        None if null.get("no_quads") else p(quads, 4), cap,
                                        None if null.get("no_n_quads") else C.cast(p(one[0], 1), C.POINTER(C.c_uint32)),
                                        None if null.get("no_status") else C.cast(p(one[1], 1), C.POINTER(C.c_uint32)),
                                        None if null.get("no_scores") else p(scores, 1),
                                        None if null.get("no_best") else C.cast(p(one[2], 1), C.POINTER(C.c_uint32)))
    assert (quads[:4] == guard).all() and (quads[-4:] == guard).all() and scores[0] == guard and scores[-1] == guard
    assert (one[:, 0] == guard).all() and (one[:, 2] == guard).all()
    return rc, quads[4:-4].reshape(cap, 4), one[0, 1], one[1, 1], scores[1:-1], one[2, 1]


def test_refused_arguments():
    l = BC.lattice(7, 7)
    seed = [Y.try_find_best_board(l)[0]]
    assert raw(l, seed)[0] == _ffi.AGX_OK
    for ratio in (np.nan, np.inf, -np.inf, -1.0, -1.5, float(BC.f32_steps(-1.0, -1))):
        assert raw(l, seed, ratio=ratio)[0] == _ffi.AGX_ERR_ARG, ratio
    assert raw(l, seed, ratio=float(BC.f32_steps(-1.0, 1)))[0] == _ffi.AGX_OK  # (1 + ratio > 0: the last one allowed)
    for flags in (2, 3, -1):
        assert raw(l, seed, flags=flags)[0] == _ffi.AGX_ERR_ARG
    for what in ("no_saddles", "no_seeds", "no_quads", "no_n_quads", "no_status"):
        assert raw(l, seed, **{what: True})[0] == _ffi.AGX_ERR_ARG, what
    assert raw(l, seed, no_scores=True, no_best=True)[0] == _ffi.AGX_OK  # optional on their own


def test_input_none_and_capacity():
    guard = 0xDEADBEEF
    l = BC.lattice(7, 7)
    board = Y.try_find_best_board(l)
    seed = [board[0]]
    for bad in (49, 0xFFFFFFFF):  # a slot at or beyond the list
        rc, quads, n, status, scores, best = raw(l, [[board[0][0], bad, board[0][2], board[0][3]]])
        assert (rc, n, status) == (_ffi.AGX_OK, 0, _ffi.AGX_BOARD_INPUT) and (quads == guard).all() and (scores == guard).all() and best == guard
    ps = np.zeros(49, np.uint32)
    ps[board[0][2]] = 1  # the seed names a slot that is not listed
    assert raw(l, seed, point_status=ps)[2:4] == (0, _ffi.AGX_BOARD_INPUT)
    assert raw(l, [board[1], board[0]], point_status=ps)[2:4] == (0, _ffi.AGX_BOARD_INPUT)  # (every seed is looked at first)
    rc, quads, n, status, scores, best = raw(l, np.zeros((0, 4), np.uint32))  # no seed
    assert (rc, n, status) == (_ffi.AGX_OK, 0, _ffi.AGX_BOARD_NONE) and best == guard
    nan = l.copy()
    nan[30, 1] = np.nan
    assert raw(nan, seed)[2:4] == (0, _ffi.AGX_BOARD_INPUT)
    rc, quads, n, status, scores, best = raw(l, seed, cap=8)  # one row short: the true count, no row
    assert (rc, n, status) == (_ffi.AGX_OK, 9, _ffi.AGX_BOARD_CAPACITY) and (quads == guard).all() and scores.tolist() == [9] and best == 0
    rc, quads, n, status, scores, best = raw(l, seed, cap=9)
    assert (n, status) == (9, _ffi.AGX_BOARD_FOUND) and quads.tobytes() == np.array(board, np.uint32).tobytes()
    # point_status words removing a board saddle: the yardstick's smaller board, slot numbers of the whole list
    ps = np.zeros(49, np.uint32)
    ps[board[4][1]] = 7
    got = check(l, seed, "a board saddle removed", point_status=ps)
    assert got[1] == _ffi.AGX_BOARD_FOUND and got[2] < 9 and board[4][1] not in got[0]
