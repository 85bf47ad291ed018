"""rochade_refine's constants at half_size_patch 1 .. 4 (agx_debug_refine_constants; reference src/detector.rs:208-254) against
the oracle's orc_refine_pmat, without a device.  The cone kernel is the oracle's bit for bit at every size.  The pseudo-inverse
is the exact one of the quadratic design matrix rounded to binary32: the oracle's Gauss-Jordan gives the same bits at 1, 2 and
4; at 3 it leaves 28 of its 294 entries at 2^-60 or 2^-59 where the exact value is 0 (all in columns 0 and 2), and every other
entry is bit-equal there too."""
import ctypes as C

import numpy as np
import pytest

from tests.util import bits_equal

AGX_OK, AGX_ERR_ARG, AGX_ERR_CAPACITY = 0, -1, -3
HALVES = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


@pytest.fixture(scope="module")
def lib():
    from aprilgrid_rs_amd import _ffi
    return _ffi.lib()


def constants(lib, half, cap=81):
    cone = np.full(81, np.float32(-7.0), np.float32)
    pmat = np.full(81 * 6, np.float32(-7.0), np.float32)
    n = C.c_int(-1)
    st = lib.agx_debug_refine_constants(half, cone.ctypes.data, pmat.ctypes.data, cap, C.byref(n))
    return st, n.value, cone, pmat


@pytest.mark.parametrize("half", HALVES)
def test_cone_is_the_oracles_bit_for_bit(lib, oracle, half):
    st, n, cone, pmat = constants(lib, half)
    ks = 2 * half + 1
    assert st == AGX_OK and n == ks * ks
    op, ok = oracle.refine_constants(half)
    assert bits_equal(cone[:n], np.asarray(ok, np.float32).reshape(-1))
    assert (cone[n:] == np.float32(-7.0)).all() and (pmat[n * 6:] == np.float32(-7.0)).all()  # nothing written past n_points


@pytest.mark.parametrize("half", (1, 2, 4))
def test_pmat_is_the_oracles_bit_for_bit(lib, oracle, half):
    st, n, _, pmat = constants(lib, half)
    assert st == AGX_OK
    op, _ = oracle.refine_constants(half)
    assert bits_equal(pmat[:n * 6], np.asarray(op, np.float32).reshape(-1))


def test_pmat_at_3_is_the_oracles_wherever_the_exact_value_is_not_zero(lib, oracle):
    st, n, _, pmat = constants(lib, 3)
    assert st == AGX_OK and n == 49
    got = pmat[:n * 6].reshape(n, 6)
    op = np.asarray(oracle.refine_constants(3)[0], np.float32).reshape(n, 6)
    big = np.abs(op) > 2.0 ** -50
    assert bits_equal(got[big], op[big])
    rest = ~big  # (the exact zeros: where the oracle has 0.0 as well, and where its elimination left a residue)
    assert (got[rest].view(np.uint32) == 0).all(), "an exact zero is not +0.0"
    assert (np.abs(op[rest]) <= 2.0 ** -59).all()
    residue = rest & (op != 0)
    assert int(residue.sum()) == 28
    assert set(np.nonzero(residue)[1]) <= {0, 2}


@pytest.mark.parametrize("half", HALVES)
def test_no_negative_zero(lib, half):
    st, n, cone, pmat = constants(lib, half)
    assert st == AGX_OK
    for a in (cone[:n], pmat[:n * 6]):
        assert not (a.view(np.uint32) == 0x80000000).any()


def test_half_2_is_what_the_handle_less_constants_call_gives(lib):
    cone25 = np.zeros(25, np.float32)
    pmat150 = np.zeros(150, np.float32)
    assert lib.agx_detector_constants(None, None, cone25.ctypes.data, pmat150.ctypes.data) == AGX_OK
    st, n, cone, pmat = constants(lib, 2)
    assert st == AGX_OK and n == 25
    assert bits_equal(cone[:25], cone25) and bits_equal(pmat[:150], pmat150)


def test_python_wrapper(lib):
    import aprilgrid_rs_amd as A
    for half in HALVES:
        cone, pmat = A.refine_constants(half)
        st, n, c, p = constants(lib, half)
        assert cone.shape == (n,) and pmat.shape == (n, 6)
        assert bits_equal(cone, c[:n]) and bits_equal(pmat.reshape(-1), p[:n * 6])
    with pytest.raises(A.AgxError) as e:
        A.refine_constants(5)
    assert e.value.status == AGX_ERR_ARG


def test_argument_rules(lib):
    for half in (0, 5, -1):
        assert constants(lib, half)[0] == AGX_ERR_ARG, half
    buf = np.zeros(81 * 6, np.float32)
    n = C.c_int(0)
    assert lib.agx_debug_refine_constants(2, None, buf.ctypes.data, 81, C.byref(n)) == AGX_ERR_ARG
    assert lib.agx_debug_refine_constants(2, buf.ctypes.data, None, 81, C.byref(n)) == AGX_ERR_ARG
    assert lib.agx_debug_refine_constants(2, buf.ctypes.data, buf.ctypes.data, 81, None) == AGX_ERR_ARG
    for half in HALVES:
        ks2 = (2 * half + 1) ** 2
        st, n_pts, cone, pmat = constants(lib, half, cap=ks2 - 1)
        assert st == AGX_ERR_CAPACITY and n_pts == ks2
        assert (cone == np.float32(-7.0)).all() and (pmat == np.float32(-7.0)).all()  # nothing written
        assert constants(lib, half, cap=ks2)[0] == AGX_OK
