"""The Python and Rust surfaces of the calibration exist and the wrappers check their arguments (tests/test_rust_binding.py holds
ffi.rs to the header declaration for declaration; this file only pins the new names)."""
import os

import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import calibrate_cases as CC
from tests.util import ROOT


def test_the_surfaces_exist():
    for name in ("calibrate", "calibrate_seed", "calib_report", "calib_param_jacobian"):
        assert callable(getattr(A, name)) and name in A.__all__
    for name in ("calibrate", "calibrate_seed", "calibrate_enqueue", "calibrate_batch"):
        assert callable(getattr(A.TagDetector, name))
    for sym in ("agx_calibrate_enqueue", "agx_calibrate_tail", "agx_calibrate_seed_tail", "agx_debug_calib_param_jacobian"):
        assert sym in _ffi.SYMBOLS and hasattr(_ffi.lib(), sym)
    assert (_ffi.AGX_CALIB_OK, _ffi.AGX_CALIB_FEW, _ffi.AGX_CALIB_SINGULAR, _ffi.AGX_CALIB_ACCEPT_LOOSE) == (0, 1, 2, 1)
    assert np.dtype(_ffi.CALIB_REPORT_DTYPE).itemsize == 552
    rust = os.path.join(ROOT, "bindings", "rust", "src")
    ffi, lib = open(os.path.join(rust, "ffi.rs")).read(), open(os.path.join(rust, "lib.rs")).read()
    for text in ("pub fn agx_calibrate_enqueue(", "pub fn agx_calibrate_tail(", "pub fn agx_calibrate_seed_tail(", "pub fn agx_debug_calib_param_jacobian("):
        assert text in ffi, text
    for text in ("pub fn calibrate_tail(", "pub fn calibrate_seed_tail(", "pub struct CalibReport", "ffi::agx_calibrate_tail(", "ffi::agx_calibrate_seed_tail("):
        assert text in lib, text


def test_the_wrappers_check_their_arguments():
    b = CC.exact_batch("radtan", noise=0.1).subset([0, 1, 2])
    ok = dict(tags=b.tags, n_tags=b.counts, cols=6, rows=6, camera=b.seed, poses=b.pose, row_status=b.row_status, fit_status=b.fit_status,
              tag_size=CC.TAG_SIZE, iterations=1)
    assert A.calibrate(**ok)["status"] == CC.OK
    for kw in (dict(damping=-1.0), dict(damping=float("inf")), dict(iterations=65), dict(min_tags=0), dict(min_frames=0), dict(tag_size=-1.0),
               dict(cols=0), dict(spacing_ratio=float("nan")), dict(camera=A.Camera(400.0, -1.0, 0.0, 0.0)), dict(camera=None), dict(fixed=512),
               dict(fixed=["fz"]), dict(fixed=[9]), dict(n_tags=b.counts[:2]), dict(poses=b.pose[:2]), dict(fit_status=b.fit_status[:2]),
               dict(tags=b.tags.view(np.uint8)), dict(camera=A.Camera.equidistant(400.0, 400.0, 0.0, 0.0)._replace(k3=1.0))):
        with pytest.raises(A.AgxError) as e:
            A.calibrate(**dict(ok, **kw))
        assert e.value.status == _ffi.AGX_ERR_ARG, kw
    assert A.detector._fixed_mask(["fx", "k3", 2]) == 0x105 and A.detector._fixed_mask(0x1ff) == 0x1ff
    with pytest.raises(A.AgxError):
        A.calibrate_seed(np.zeros((2, 9)), [0], (800, 600))
    with pytest.raises(A.AgxError):
        A.calibrate_seed(np.zeros((1, 9)), [0], (0, 600))
    with pytest.raises(A.AgxError):
        A.calibrate_seed(np.zeros((0, 9)), [], (800, 600))
    with pytest.raises(A.AgxError):
        A.calib_report(np.zeros(68))
    with pytest.raises(A.AgxError):
        A.calib_param_jacobian(A.Camera.double_sphere(250.0, 250.0, 0.0, 0.0, 0.0, 1.5), [[0.0, 0.0, 1.0]])
    lib = _ffi.lib()
    assert lib.agx_calibrate_tail(3, None, 1, None, None, 6, 6, 0, 0.3, 1.0, 0, b.seed.as_doubles(), 0, 0.0, 1, 1, 1, 0, *([None] * 8)) == _ffi.AGX_ERR_ARG
    assert lib.agx_debug_calib_param_jacobian(3, b.seed.as_doubles(), None, 0, None) == _ffi.AGX_ERR_ARG
