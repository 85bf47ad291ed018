"""agx_board_pose_enqueue_m at AGX_LENS_DOUBLE_SPHERE (k_board_pose<AGX_LENS_DOUBLE_SPHERE>) on the GPU: every output array against
the host form agx_board_pose_tail_m byte for byte, FILL bytes beyond and between what a frame may write included
(tests/test_board_pose_ds_cpu.py holds the host form to numpy and scipy).  The model is + - * / and the binary64 square root, so
this is the test that the two compilers keep its order of operations.  The launches are board_pose_cases.gpu_batches' construction
under the four (xi, alpha) cameras (tests/board_pose_ds_cases.py) -- every frame status in a launch, 1 .. 587 rows a frame, layouts
1 x 1 and 6 x 6, 64 x 64 once -- and one 6 x 6 launch of three frames under the alpha = 0.8 camera whose tables hold a corner on the
principal point, corners with Zc < 0 inside the cone (which the seed clamps), a corner clamped by its angle and a corner outside
the unprojection's domain.  Then the refusals through the device entry."""
import ctypes as C

import numpy as np
import pytest

from tests import board_fit_cases as BC
from tests import board_pose_cases as PC
from tests import board_pose_ds_cases as DC
from tests.board_pose_cases import FEW, INPUT, KEYS, LOOSE, OK, SINGULAR

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_arrays(b):
    d = {k: dev(v.view(np.int32).reshape(v.shape[0], -1, 9) if k == "pred" else v) for k, v in b.empty_outputs().items()}
    table = dev(b.table().view(np.int32).reshape(b.n, b.tpf, 9))
    counts = dev(np.array(b.counts, np.int32))
    st = None if b.tag_status is None else dev(np.array(b.tag_status, np.int32))
    return d, table, counts, st


def enqueue(det, b, d, table, counts, st):
    """The model reaches the kernel through the Camera object."""
    assert b.cam.model == DC.DS
    n = b.n
    det.board_pose_enqueue(table, counts, b.cols, b.rows, b.cam, *[d[k][:n] for k in KEYS], tag_size=b.tag_size, first_id=b.first_id,
                           spacing_ratio=b.s, max_err_sq=b.max_err_sq, max_drop=b.max_drop, min_tags=b.min_tags, iterations=b.iterations,
                           predict_missing=bool(b.flags & PC.MISSING), tag_status=st)


def run(det, b):
    import torch
    want = b.host()
    d, table, counts, st = device_arrays(b)
    enqueue(det, b, d, table, counts, st)
    det.sync()
    torch.cuda.synchronize()
    for k in KEYS:
        assert d[k].cpu().numpy().tobytes() == want[k].tobytes(), "%s: %s differs from the host form" % (b.name, k)
    return want


@pytest.mark.parametrize("name", sorted(DC.gpu_batches()))
def test_the_kernel_gives_the_host_forms_bytes(det, name):
    b, status = DC.gpu_batches()[name]
    want = run(det, b)
    seen = want["status"][:b.n].tolist()
    assert seen == status, (name, seen)
    if b.n > 3:
        assert set(seen) == {OK, LOOSE, FEW, SINGULAR, INPUT}, (name, seen)
    assert BC.untouched(want["status"][b.n:]) and BC.untouched(want["pose"][b.n:])
    for f in range(b.n):
        if seen[f] in (FEW, SINGULAR, INPUT):  # refused: its three words and nothing else
            assert want["n_inliers"][f] == 0 and want["n_pred"][f] == 0
            assert all(BC.untouched(want[k][f]) for k in ("pose", "err_sq", "row_status", "rms", "best_iter", "pred"))
        else:
            cnt = b.counts[f]
            assert BC.untouched(want["err_sq"][f, cnt:]) and BC.untouched(want["row_status"][f, cnt:])
            assert BC.untouched(want["pred"][f, int(want["n_pred"][f]):])


@pytest.mark.parametrize("iterations", [0, 10])
def test_the_corners_only_this_model_has(det, iterations):
    """board_pose_ds_cases.special_tables under the alpha = 0.8 camera, at the seed alone and after ten steps."""
    cam = DC.CAMERAS["high"]
    tables = DC.special_tables(cam)
    xy = [t["xy"].reshape(-1, 4, 2).astype(np.float64) for t in tables]
    assert (tables[0]["xy"].reshape(-1, 2) == np.float32([cam.cx, cam.cy])).all(axis=-1).any()
    ray = DC.unproject(cam, xy[1][..., 0], xy[1][..., 1])
    assert (ray[..., 2] <= 0.0).any() and DC.in_domain(cam, xy[1][..., 0], xy[1][..., 1]).all()
    assert (~DC.in_domain(cam, xy[2][..., 0], xy[2][..., 1])).sum() == 1
    ray = DC.unproject(cam, xy[2][0, 0, 0], xy[2][0, 0, 1])
    assert ray[2] > 0.0 and np.arctan2(np.hypot(ray[0], ray[1]), ray[2]) > DC.THETA_MAX
    b = DC.Batch("special_it%d" % iterations, tables, 6, 6, cam, max_err_sq=1e30, iterations=iterations, flags=PC.MISSING, tpf=40)
    want = run(det, b)
    assert want["status"][:3].tolist() == [OK, OK, OK] and np.isfinite(want["pose"][:3]).all() and np.isfinite(want["rms"][:3]).all()
    if iterations:
        assert want["rms"][0] < 1e-3 and want["rms"][1] < 1e-3
        k = int(want["n_pred"][1])
        assert want["pred"]["id"][1, :k].tolist() == list(DC.BEHIND_MISSING) and np.isfinite(want["pred"]["xy"][1, :k]).all()
        Z = (PC.board_points(6, 6, tag_size=PC.TAG_SIZE) @ want["pose"][1, :9].reshape(3, 3).T + want["pose"][1, 9:])[list(DC.BEHIND_MISSING), :, 2]
        assert (Z < 0.0).any()  # predicted rows of tags behind the image plane


def test_refused_arguments_leave_the_batch_in_flight(det):
    import torch
    b, _ = DC.gpu_batches()["1x1"]
    d, table, counts, st = device_arrays(b)
    det.saddles_batch_enqueue(torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda"))
    good = PC.camera_args(b.cam)

    def call(model, cam):
        return det._lib.agx_board_pose_enqueue_m(det._h, 1, table.data_ptr(), b.tpf, counts.data_ptr(), None, 1, 1, 7, 0.3, 0.05, model, (C.c_double * 9)(*cam),
                                                 4.0, 0, 1, 10, 0, *[d[k].data_ptr() for k in KEYS])

    def put(i, v):
        return good[:i] + [v] + good[i + 1:]

    cases = [(DC.DS, put(5, v)) for v in (-1e-9, 1.0 + 1e-9, np.nan)] + [(DC.DS, put(4, v)) for v in (-1.0, 1.0 + 1e-9, np.inf)]
    cases += [(DC.DS, put(i, 5e-324)) for i in (6, 7, 8)] + [(3, good), (-1, good)]
    for model, cam in cases:
        assert call(model, cam) == _ffi.AGX_ERR_ARG, (model, cam)
    res, _ = det.saddles_batch_fetch()  # still there
    assert len(res) == 1 and all(BC.untouched(d[k].cpu().numpy()) for k in KEYS)
    assert call(DC.DS, good) == _ffi.AGX_OK  # the same six-number camera passes
    det.sync()
    with pytest.raises(A.AgxError) as e:
        det.saddles_batch_fetch()
    assert e.value.status == _ffi.AGX_ERR_STATE
    assert int(d["status"][0]) == OK
