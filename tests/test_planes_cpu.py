"""agx_debug_blur_weights without a GPU: the taps of gaussian_blur_f32 (src/image_util.rs:111-124) at any sigma the new
blur kernel takes are the oracle's, bit for bit, and the sigma rules of agx_planes_enqueue hold."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.util import bits_equal

SIGMAS = [0.05, 0.3, 0.5, 1.5, 2.0, 2.0000002, 2.25, 3.3, 7.75, 8.0]


@pytest.fixture(scope="module")
def lib():
    from aprilgrid_rs_amd import _ffi
    return _ffi.lib()


def weights(lib, sigma, cap=33):
    w = np.full(max(cap, 1), np.nan, np.float32)
    radius = C.c_int(-1)
    st = lib.agx_debug_blur_weights(sigma, w.ctypes.data, cap, C.byref(radius))
    return st, w, radius.value


@pytest.mark.parametrize("sigma", SIGMAS)
def test_weights_are_the_oracles_bit_for_bit(lib, sigma):
    ref = O.blur_weights(sigma)
    st, w, radius = weights(lib, sigma)
    assert st == 0
    assert 2 * radius + 1 == len(ref) and radius == int(np.ceil(np.float32(sigma) * np.float32(2.0)))
    assert bits_equal(w[: len(ref)], ref)
    assert np.isnan(w[len(ref):]).all()  # nothing behind the taps is written
    import aprilgrid_rs_amd as A
    assert bits_equal(A.blur_weights(sigma), ref)


def test_sigma_one_and_a_half_is_the_detectors_seven_taps(lib):
    """What tests/test_oracle_pins.py pins of the seven taps, and the handle's stored constants (agx_detector_constants)."""
    st, w, radius = weights(lib, 1.5)
    assert st == 0 and radius == 3
    w = w[:7]
    assert bits_equal(w, O.blur_weights(1.5))
    assert abs(float(w.sum()) - 1.0) < 1e-6 and bits_equal(w, w[::-1])
    stored = np.zeros(7, np.float32)
    assert lib.agx_detector_constants(None, stored.ctypes.data, None, None) == 0
    assert bits_equal(stored, w)


@pytest.mark.parametrize("sigma", [0.0, -1.0, float("nan"), float("inf"), 8.01])
def test_sigmas_the_blur_does_not_take(lib, sigma):
    from aprilgrid_rs_amd import _ffi
    st, w, _ = weights(lib, sigma)
    assert st == _ffi.AGX_ERR_ARG
    assert np.isnan(w).all()
    import aprilgrid_rs_amd as A
    with pytest.raises(A.AgxError) as e:
        A.blur_weights(sigma)
    assert e.value.status == _ffi.AGX_ERR_ARG


def test_short_capacity_and_null_arguments(lib):
    from aprilgrid_rs_amd import _ffi
    for sigma, cap in ((1.5, 6), (1.5, 0), (8.0, 32), (0.3, 2)):
        st, w, radius = weights(lib, sigma, cap)
        assert st == _ffi.AGX_ERR_CAPACITY and np.isnan(w).all()
        assert cap < 2 * radius + 1  # the radius is reported: the caller can size the array
    assert weights(lib, 1.5, 7)[0] == 0 and weights(lib, 8.0, 33)[0] == 0
    r = C.c_int(0)
    assert lib.agx_debug_blur_weights(1.5, None, 7, C.byref(r)) == _ffi.AGX_ERR_ARG
    w = np.zeros(7, np.float32)
    assert lib.agx_debug_blur_weights(1.5, w.ctypes.data, 7, None) == _ffi.AGX_ERR_ARG
