"""The chain at any half_size_patch without a GPU: the yardstick of tests/test_gpu_patch.py (tests/patch_oracle.py, the
reference's refined_saddle_points composed from the oracle's exported pieces with a sigma in place of the 1.5 of
src/detector.rs:410 and a half_size_patch in place of the 2 of :430) is the oracle's own refined_saddle_points at (1.5, 2) --
every plane, table and record, bit for bit; the counts it gives at the other sizes are pinned; no record of a case the GPU file
uses sits close enough to the phi limits for the angle tolerance to hide a difference behind the filter; and the two new
entries of the C ABI are declared, bound and refuse a NULL handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import patch_oracle
from tests.util import ANGLE_TOL_DEG, ROOT, load_image, synth_module

AGX_ERR_ARG = -1
# (sigma, half) of every case tests/test_gpu_patch.py runs on the three 320 x 240 frames
GPU_CASES = [(s, h) for s in (1.5, 3.0) for h in (1, 2, 3, 4)] + [(6.0, 4)]
COUNTS_AT_1_5 = {1: (202, 173, 192), 2: (177, 157, 178), 3: (161, 137, 151), 4: (151, 96, 147)}


@pytest.fixture(scope="module")
def boards():
    return synth_module().render_batch(0, 3, 320, 240)[0].numpy()


@pytest.fixture(scope="module")
def helper(boards):
    """The helper's answer for every (sigma, half, frame) the GPU file uses, computed once."""
    return {(s, h, i): patch_oracle.refined_saddle_points(boards[i], s, h) for s, h in GPU_CASES for i in range(3)}


def same_products(got, g, ref, d, what):
    for key in ("blur", "resp", "min_resp", "centers", "refined"):
        a, b = np.ascontiguousarray(g[key]), np.ascontiguousarray(d[key])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %s" % (what, key)
    for key in ("first_index", "sizes"):
        assert np.array_equal(g[key], d[key]), "%s: %s" % (what, key)
    assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), "%s: saddles after the filter" % what


def test_the_helper_at_1_5_and_2_is_the_oracle(boards, helper):
    from oracle import oracle as O
    for i in range(3):
        ref, d = O.refined_saddle_points(boards[i], debug=True)
        got, g = helper[(1.5, 2, i)]
        same_products(got, g, ref, d, "frame %d" % i)
        assert len(ref) == COUNTS_AT_1_5[2][i]
    img = load_image("EuRoC.png")
    ref, d = O.refined_saddle_points(img, debug=True)
    got, g = patch_oracle.refined_saddle_points(img, 1.5, 2)
    same_products(got, g, ref, d, "EuRoC.png")
    assert len(ref) >= 2


@pytest.mark.parametrize("half", [1, 3, 4])
def test_counts_at_sigma_1_5(helper, half):
    assert tuple(len(helper[(1.5, half, i)][0]) for i in range(3)) == COUNTS_AT_1_5[half]


def test_lists_at_2_and_3_differ(helper):
    assert helper[(1.5, 2, 0)][0].tobytes() != helper[(1.5, 3, 0)][0].tobytes()


def test_the_large_component_at_sigma_6(helper):
    out, d = helper[(6.0, 4, 0)]
    assert int(d["sizes"].max()) == 7756 and len(out) == 1
    assert len(helper[(6.0, 4, 2)][0]) == 0


def test_no_record_sits_at_the_phi_limits(helper):
    """The k / phi filter keeps phi in [30, 60] (the default parameters): a record within the angle tolerance of a limit could
    be kept by one side and dropped by the other without the comparison of the angles noticing."""
    tightest = (np.inf, None)
    for key, (_, d) in helper.items():
        phi = d["refined"]["phi"].astype(np.float64)
        if not len(phi):
            continue
        m = float(min(np.abs(phi - 30.0).min(), np.abs(phi - 60.0).min()))
        assert m > 2 * ANGLE_TOL_DEG, (key, m)
        tightest = min(tightest, (m, key))
    assert tightest[1] == (1.5, 3, 0) and abs(tightest[0] - 0.00243) < 1e-5, tightest


def test_the_abi_declares_and_binds_both_functions():
    header = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    assert re.search(r"int\s+agx_detector_set_half_size_patch\s*\(\s*agx_detector\s*\*\s*det\s*,\s*int\s+half_size_patch\s*\)\s*;", header)
    assert re.search(r"int\s+agx_detector_get_half_size_patch\s*\(\s*const\s+agx_detector\s*\*\s*det\s*,\s*int\s*\*\s*half_size_patch\s*\)\s*;", header)
    ffi_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub fn agx_detector_set_half_size_patch(det: *mut agx_detector, half_size_patch: c_int) -> c_int;" in ffi_rs
    assert "pub fn agx_detector_get_half_size_patch(det: *const agx_detector, half_size_patch: *mut c_int) -> c_int;" in ffi_rs
    assert "with_half_size_patch" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    from aprilgrid_rs_amd import _ffi
    lib = _ffi.lib()
    v = C.c_int(-7)
    assert lib.agx_detector_set_half_size_patch(None, 3) == AGX_ERR_ARG
    assert lib.agx_detector_get_half_size_patch(None, C.byref(v)) == AGX_ERR_ARG
    assert v.value == -7
    assert lib.agx_abi_version() == 1
