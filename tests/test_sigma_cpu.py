"""The any-sigma chain without a GPU: the yardstick of tests/test_gpu_sigma.py (tests/sigma_oracle.py, the reference's
refined_saddle_points composed from the oracle's exported pieces with a sigma in place of the 1.5 of src/detector.rs:410) is
the oracle's own refined_saddle_points at sigma 1.5 -- every plane, table and record, bit for bit -- and the two new entries
of the C ABI refuse a NULL handle."""
import ctypes as C

import numpy as np
import pytest

from tests import sigma_oracle
from tests.util import ALL_IMAGES, load_image, synth_module

AGX_ERR_ARG = -1


def synthetic_frames():
    synth = synth_module()
    return [("synthetic %d" % f, synth.render_frame(f, 320, 240)[0].numpy()) for f in range(3)]


@pytest.mark.parametrize("name", ALL_IMAGES + ["synthetic"])
def test_the_helper_at_sigma_1_5_is_the_oracle(name):
    from oracle import oracle as O
    images = synthetic_frames() if name == "synthetic" else [(name, load_image(name))]
    for what, img in images:
        ref, d = O.refined_saddle_points(img, debug=True)
        got, g = sigma_oracle.refined_saddle_points(img, 1.5)
        for key in ("blur", "resp", "min_resp", "centers", "refined"):
            a, b = np.ascontiguousarray(g[key]), np.ascontiguousarray(d[key])
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %s" % (what, key)
        for key in ("first_index", "sizes"):
            assert np.array_equal(g[key], d[key]), "%s: %s" % (what, key)
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), "%s: saddles after the filter" % what
        assert len(ref) >= 2, what


def test_the_helper_follows_sigma():
    """Another sigma is another blur plane (the oracle's gaussian_blur_f32 at that sigma) and another list."""
    from oracle import oracle as O
    img = synthetic_frames()[0][1]
    s15, _ = sigma_oracle.refined_saddle_points(img, 1.5)
    s25, d = sigma_oracle.refined_saddle_points(img, 2.5)
    assert d["blur"].tobytes() == O.gaussian_blur_f32(O.luma_f32(img), 2.5).tobytes()
    assert len(s25) >= 2 and s25.tobytes() != s15.tobytes()


def test_null_handle_is_refused():
    from aprilgrid_rs_amd import _ffi
    lib = _ffi.lib()
    v = C.c_float(-7.0)
    assert lib.agx_detector_set_blur_sigma(None, 2.0) == AGX_ERR_ARG
    assert lib.agx_detector_get_blur_sigma(None, C.byref(v)) == AGX_ERR_ARG
    assert v.value == -7.0
