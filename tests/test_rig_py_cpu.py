"""The Python and Rust surfaces of the rig calibration exist and the wrappers check their arguments (tests/test_rust_binding.py
holds ffi.rs to the header declaration for declaration; this file only pins the new names)."""
import os

import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import calibrate_cases as CC
from tests import rig_cases as RC
from tests.util import ROOT


def test_the_surfaces_exist():
    for name in ("rig_calibrate", "rig_seed", "rig_report", "rig_jacobian"):
        assert callable(getattr(A, name)) and name in A.__all__
    for name in ("rig_calibrate", "rig_seed", "rig_calibrate_enqueue", "rig_calibrate_batch"):
        assert callable(getattr(A.TagDetector, name))
    for sym in ("agx_rig_calibrate_enqueue", "agx_rig_calibrate_tail", "agx_rig_seed_tail", "agx_debug_rig_jacobian"):
        assert sym in _ffi.SYMBOLS and hasattr(_ffi.lib(), sym)
    assert (_ffi.AGX_RIG_OK, _ffi.AGX_RIG_FEW, _ffi.AGX_RIG_SINGULAR, _ffi.AGX_RIG_CAM_ATTACHED, _ffi.AGX_RIG_CAM_DETACHED) == (0, 1, 2, 0, 1)
    assert np.dtype(_ffi.RIG_REPORT_DTYPE).itemsize == 560
    rust = os.path.join(ROOT, "bindings", "rust", "src")
    ffi, lib = open(os.path.join(rust, "ffi.rs")).read(), open(os.path.join(rust, "lib.rs")).read()
    for text in ("pub fn agx_rig_calibrate_enqueue(", "pub fn agx_rig_calibrate_tail(", "pub fn agx_rig_seed_tail(", "pub fn agx_debug_rig_jacobian("):
        assert text in ffi, text
    for text in ("pub fn rig_calibrate_tail(", "pub fn rig_seed_tail(", "pub struct RigReport", "ffi::agx_rig_calibrate_tail(", "ffi::agx_rig_seed_tail("):
        assert text in lib, text


def test_the_wrappers_check_their_arguments():
    b = RC.stereo_rig(noise=0.1).subset(instants=[0, 1, 2])
    seed = RC.off_extrinsics(b.E)
    ok = dict(tags=b.tags, n_tags=b.counts, cols=6, rows=6, cameras=b.cams, poses=b.pose, row_status=b.row_status, fit_status=b.fit_status,
              extrinsics=seed, tag_size=CC.TAG_SIZE, iterations=1)
    assert A.rig_calibrate(**ok)["status"] == RC.OK
    nan_seed = seed.copy()
    nan_seed[1, 0] = np.nan
    for kw in (dict(damping=-1.0), dict(damping=float("inf")), dict(iterations=65), dict(min_tags=0), dict(min_cams=0), dict(min_instants=0),
               dict(tag_size=-1.0), dict(cols=0), dict(spacing_ratio=float("nan")), dict(cameras=[b.cams[0], A.Camera(400.0, -1.0, 0.0, 0.0)]),
               dict(cameras=b.cams[:1]), dict(cameras=[b.cams[0], None]), dict(n_tags=b.counts[:, :2]), dict(poses=b.pose[:, :2]),
               dict(fit_status=b.fit_status[:1]), dict(extrinsics=seed[:1]), dict(extrinsics=nan_seed), dict(tags=b.tags.view(np.uint8)),
               dict(tags=b.tags[0]), dict(cameras=[b.cams[0], A.Camera.equidistant(400.0, 400.0, 0.0, 0.0)._replace(k3=1.0)])):
        with pytest.raises(A.AgxError) as e:
            A.rig_calibrate(**dict(ok, **kw))
        assert e.value.status == _ffi.AGX_ERR_ARG, kw
    with pytest.raises(A.AgxError):  # one camera is no rig
        A.rig_calibrate(**dict(ok, tags=b.tags[:1], n_tags=b.counts[:1], poses=b.pose[:1], row_status=b.row_status[:1], fit_status=b.fit_status[:1],
                               cameras=b.cams[:1], extrinsics=seed[:1]))
    with pytest.raises(A.AgxError):
        A.rig_seed(np.zeros((2, 3, 12)), [0] * 5)
    with pytest.raises(A.AgxError):
        A.rig_seed(np.zeros((2, 3, 12)), [0] * 6, [1] * 5)
    with pytest.raises(A.AgxError):
        A.rig_seed(np.zeros((1, 3, 12)), [0] * 3)
    with pytest.raises(A.AgxError):
        A.rig_seed(np.zeros((6, 12)), [0] * 6)
    with pytest.raises(A.AgxError):
        A.rig_report(np.zeros(69))
    with pytest.raises(A.AgxError):
        A.rig_jacobian(A.Camera.double_sphere(250.0, 250.0, 0.0, 0.0, 0.0, 1.5), None, RC.IDENT, [[0.0, 0.0]])
    lib = _ffi.lib()
    from aprilgrid_rs_amd.detector import _rig_cameras
    models, cams = _rig_cameras(b.cams, 2)
    assert lib.agx_rig_calibrate_tail(2, 3, None, 1, None, None, 6, 6, 0, 0.3, 1.0, models, cams, 0.0, 1, 1, 2, 1, 0, *([None] * 10)) == _ffi.AGX_ERR_ARG
    assert lib.agx_rig_seed_tail(2, 3, None, None, None, None, None) == _ffi.AGX_ERR_ARG
    assert lib.agx_debug_rig_jacobian(3, b.cams[0].as_doubles(), None, None, None, 0, None) == _ffi.AGX_ERR_ARG
