"""agx_init_quads_tail -- the candidate quads of caller-given seed saddles (reference src/detector.rs:543-586), the host form --
against tests/board_grow_oracle.py's init_quads (tests/init_quads_cases.py states the contract with it).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import board_cases as BC
from tests import init_quads_cases as IQ
from tests.test_find_boards_cpu import golden_list
from tests.test_grow_boards_cpu import as_list
from tests.util import ALL_IMAGES

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

F32 = np.float32
NEAREST = (2, 3, 8, 49, 50, 51, 64)


def check(l, seeds=None, what="", **kw):
    """agx_init_quads_tail == the yardstick, byte for byte: rows, count, status, quads per seed, the seeds taken."""
    kw.setdefault("cap", 1024)
    want = IQ.yardstick(l, seeds, **kw)
    got = A.init_quads_tail(l, seeds, **kw)
    IQ.same(got, want, what)
    return got


# ---- 1: the golden lists, the reference's seeds and saddles 0 .. 63 ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL_IMAGES))
def test_golden_lists_reference_and_caller_seeds(name):
    l = as_list(golden_list(name))
    got = check(l, None, "the reference's seeds", max_seeds=30)
    assert got[1] == _ffi.AGX_BOARD_FOUND and got[2] <= 385 and got[3].max() <= 40
    # the pop order: the fullest round(theta) bin from the back, as the yardstick's try_find_best_board takes them
    yd = IQ.Y.Yard(l)
    assert got[4].tolist() == IQ.reference_seeds(yd, 30)
    assert (got[0][:, 0] == np.repeat(got[4], got[3][:len(got[4])])).all(), "column 0 of a row is its seed"
    seeds = list(range(min(64, len(l))))
    got = check(l, seeds, "saddles 0 .. 63")
    assert got[2] <= 729 and got[3].sum() == got[2]


# ---- 2: n_nearest, and lists shorter than it ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", NEAREST)
def test_n_nearest(k):
    l = as_list(golden_list(list(ALL_IMAGES)[0]))
    check(l, None, "golden list, k = %d" % k, max_seeds=8, n_nearest=k)
    l = BC.lattice(7, 7)
    check(l, None, "7 x 7 lattice, the reference's seeds, k = %d" % k, max_seeds=30, n_nearest=k)
    check(l, [0, 24, 48], "7 x 7 lattice, corner / centre / corner, k = %d" % k, n_nearest=k)
    for n in (1, 2, 49, 50, 51):
        sub = BC.lattice(8, 8)[:n]
        check(sub, list(range(0, n, 7)), "%d saddles, k = %d" % (n, k), n_nearest=k)
        check(sub, None, "%d saddles, k = %d, the reference's seeds" % (n, k), max_seeds=4, n_nearest=k)


def test_n_nearest_changes_the_answer():
    """Fewer neighbours, fewer quads; the whole list at 64 where 50 stops short."""
    l = BC.lattice(9, 9)
    counts = [A.init_quads_tail(l, [40], n_nearest=k)[2] for k in (2, 8, 50, 64)]
    assert counts[0] == 0 and 0 < counts[1] < counts[2] <= counts[3], counts


# ---- 3: statuses ------------------------------------------------------------------------------------------------------------------
def test_capacity_true_count_and_no_row():
    l = BC.lattice(7, 7)
    full = check(l, None, "everything", max_seeds=30)
    n = full[2]
    assert full[1] == _ffi.AGX_BOARD_FOUND and n > 1
    check(l, None, "cap = the count", max_seeds=30, cap=n)
    check(l, None, "cap = the count - 1", max_seeds=30, cap=n - 1)
    # through the C ABI, rows filled with a sentinel: CAPACITY leaves every row as it was
    lib = _ffi.lib()
    rows = np.full((n - 1, 4), 0xABCDEF01, np.uint32)
    per_seed, taken = np.full(30, 0xABCDEF01, np.uint32), np.full(30, 0xABCDEF01, np.uint32)
    nq, st, nt = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    rc = lib.agx_init_quads_tail(l.ctypes.data, len(l), None, None, 0, 30, 50, rows.ctypes.data, n - 1, C.byref(nq), C.byref(st),
                                 per_seed.ctypes.data, taken.ctypes.data, C.byref(nt))
    assert rc == _ffi.AGX_OK and st.value == _ffi.AGX_BOARD_CAPACITY and nq.value == n
    assert (rows == 0xABCDEF01).all()
    assert per_seed.tobytes() == full[3].tobytes() and nt.value == len(full[4]) and taken[:nt.value].tobytes() == full[4].tobytes()
    assert (taken[nt.value:] == 0xABCDEF01).all()


def test_bad_seeds_are_input():
    l = BC.lattice(7, 7)
    got = check(l, [3, len(l)], "a seed at n_saddles")
    assert got[1] == _ffi.AGX_BOARD_INPUT and got[3] is None
    ps = np.zeros(len(l), np.uint32)
    ps[10] = 5
    got = check(l, [3, 10], "a seed that is not listed", point_status=ps)
    assert got[1] == _ffi.AGX_BOARD_INPUT
    got = check(l, [3, 11], "the list without saddle 10", point_status=ps)
    assert got[1] == _ffi.AGX_BOARD_FOUND and not (got[0] == 10).any()
    check(l, None, "the list without saddle 10, the reference's seeds", point_status=ps, max_seeds=30)
    # a seed behind max_seeds is not looked at
    got = check(l, [3, len(l)], "one seed taken", max_seeds=1)
    assert got[1] == _ffi.AGX_BOARD_FOUND and len(got[4]) == 1


def test_nan_theta_is_input():
    l = BC.lattice(7, 7)
    l[20, 3] = np.nan
    for seeds in (None, [3]):
        got = check(l, seeds, "NaN theta")
        assert got[1] == _ffi.AGX_BOARD_INPUT
    ps = np.zeros(len(l), np.uint32)
    ps[20] = 1
    assert check(l, [3], "NaN theta, unlisted", point_status=ps)[1] == _ffi.AGX_BOARD_FOUND


def test_no_seed_and_empty_list_are_none():
    l = BC.lattice(7, 7)
    got = check(l, [], "zero seeds", max_seeds=4)
    assert got[1] == _ffi.AGX_BOARD_NONE and (got[3] == 0).all() and len(got[3]) == 4 and len(got[4]) == 0
    got = check(l[:0], None, "an empty list")
    assert got[1] == _ffi.AGX_BOARD_NONE and len(got[4]) == 0
    got = check(BC.far_saddles(20, 3), None, "no valid quad", max_seeds=5)
    assert got[1] == _ffi.AGX_BOARD_NONE and (got[3] == 0).all() and len(got[4]) >= 1


def test_duplicate_seed_yields_its_quads_twice():
    l = BC.lattice(7, 7)
    one = check(l, [24], "once")
    two = check(l, [24, 8, 24], "twice")
    assert one[2] > 0 and two[3][0] == two[3][2] == one[2]
    assert two[0][:one[2]].tobytes() == one[0].tobytes() == two[0][-one[2]:].tobytes()


# ---- 4: the chain's stop rule on host forms is the search -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL_IMAGES))
def test_init_quads_then_grow_is_find_board(name):
    l = as_list(golden_list(name))
    want = A.find_board_tail(l, cap=1024)
    got = IQ.staged_board(lambda l, s, m: A.init_quads_tail(l, s, max_seeds=m), A.grow_board_tail, l, 0.3)
    assert got[1] == want[1] == _ffi.AGX_BOARD_FOUND and got[2] == want[2]
    assert got[0].tobytes() == want[0].tobytes()


# ---- 5: argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _ffi.lib()
    l = BC.lattice(3, 3)
    rows = np.zeros((64, 4), np.uint32)
    seeds = np.array([4], np.uint32)
    nq, st = C.c_uint32(0), C.c_uint32(0)

    def call(saddles=l.ctypes.data, n=len(l), sd=seeds.ctypes.data, n_seeds=1, max_seeds=1, k=50, quads=rows.ctypes.data, cap=64,
             p_n=C.byref(nq), p_st=C.byref(st)):
        return lib.agx_init_quads_tail(saddles, n, None, sd, n_seeds, max_seeds, k, quads, cap, p_n, p_st, None, None, None)

    assert call() == _ffi.AGX_OK and st.value == _ffi.AGX_BOARD_FOUND
    for k in (0, 1, 65, 0xFFFFFFFF):
        assert call(k=k) == _ffi.AGX_ERR_ARG
    for k in (2, 64):
        assert call(k=k) == _ffi.AGX_OK
    assert call(max_seeds=0) == _ffi.AGX_ERR_ARG
    assert call(sd=None, n_seeds=1) == _ffi.AGX_ERR_ARG  # seeds counted but not given
    assert call(sd=None, n_seeds=0) == _ffi.AGX_OK       # the reference's own
    assert call(saddles=None) == _ffi.AGX_ERR_ARG
    assert call(quads=None) == _ffi.AGX_ERR_ARG
    assert call(quads=None, cap=0) == _ffi.AGX_OK and st.value == _ffi.AGX_BOARD_CAPACITY
    assert call(p_n=None) == _ffi.AGX_ERR_ARG and call(p_st=None) == _ffi.AGX_ERR_ARG
    assert lib.agx_abi_version() == 1


# ---- 6: the order of the list does not matter where no two distances tie ------------------------------------------------------------
def test_permuted_list():
    l = as_list(golden_list(list(ALL_IMAGES)[0]))
    seeds = list(range(0, min(64, len(l)), 3))
    want = A.init_quads_tail(l, seeds)
    p, perm = BC.permuted(l, 11)
    inv = np.argsort(perm)  # saddle i of l is saddle inv[i] of p
    yd = IQ.Y.Yard(l)
    for s in seeds:  # (the premise: no exact tie among a seed's distances)
        d2 = np.array([d for d, _ in yd.nearest(yd.x[s], yd.y[s], 64)])
        assert len(np.unique(d2)) == len(d2)
    got = check(p, [int(inv[s]) for s in seeds], "permuted")
    assert got[2] == want[2] and got[3].tobytes() == want[3].tobytes()
    assert perm[got[0].astype(np.int64)].astype(np.uint32).tobytes() == want[0].tobytes()
