"""agx_board_pose_enqueue_m at AGX_LENS_EQUIDISTANT (k_board_pose<AGX_LENS_EQUIDISTANT>) on the GPU: every output array against the
host form agx_board_pose_tail_m byte for byte, FILL bytes beyond and between what a frame may write included
(tests/test_board_pose_equi_cpu.py holds the host form to numpy and scipy).  This is the test that decides whether pose_atan, the
seed's tangent and the products of D and D' agree between the two compilers.  The launches are board_pose_cases.gpu_batches'
construction under four equidistant cameras (tests/board_pose_equi_cases.py: gpu_batches) -- at most 16 frames each, every frame
status, 1 .. 587 rows a frame, layouts 1 x 1 .. 64 x 64, iterations 0 / 5 / 10, max_drop 0 and > 0, both flags -- and one launch
with a corner exactly on the optical axis and just either side of the small-r threshold.  Then the predicted rows snapped on the
caller's stream, the refused arguments, and the recovery on a frame seen through a fisheye."""
import ctypes as C

import numpy as np
import pytest

from tests import board_fit_cases as BC
from tests import board_pose_cases as PC
from tests import board_pose_equi_cases as EC
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
    assert b.cam.model == _ffi.AGX_LENS_EQUIDISTANT
    n = b.n
    det.board_pose_enqueue(table, counts, b.cols, b.rows, b.cam, *[d[k][:n] for k in KEYS], tag_size=b.tag_size, first_id=b.first_id,
                           spacing_ratio=b.s, max_err_sq=b.max_err_sq, max_drop=b.max_drop, min_tags=b.min_tags, iterations=b.iterations,
                           predict_missing=bool(b.flags & PC.MISSING), tag_status=st)


@pytest.mark.parametrize("name", sorted(EC.gpu_batches()))
def test_the_kernel_gives_the_host_forms_bytes(det, name):
    import torch
    b, status = EC.gpu_batches()[name]
    want = b.host()
    d, table, counts, st = device_arrays(b)
    enqueue(det, b, d, table, counts, st)
    det.sync()
    torch.cuda.synchronize()
    for k in KEYS:
        got = d[k].cpu().numpy()
        assert got.tobytes() == want[k].tobytes(), "%s: %s differs from the host form" % (name, k)
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


def test_predicted_rows_feed_the_snap_on_the_callers_stream(det):
    """A launch on the caller's stream under the wide camera: the pose's rows of the missing tags go to snap_points_enqueue as
    they stand."""
    import torch
    cam = EC.CAMERAS["wide"]
    R, t = PC.pose("near", 6, 6)
    full = EC.exact_table(6, 6, range(36), cam, R, t, noise=0.1)
    keep = np.array([i for i in range(36) if i not in (0, 5, 17, 30, 35)])
    b = EC.EquiBatch("snap", [full[keep], full[keep][::-1]], 6, 6, cam, max_drop=1, flags=PC.MISSING, tpf=36)
    want = b.host()
    saddles = np.zeros((2, 144, 5), np.float32)  # the true corners of every tag as the frame's saddle list
    saddles[:, :, :2] = full["xy"].reshape(144, 2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d, table, counts, st = device_arrays(b)
        d_saddles, d_counts = dev(saddles), dev(np.full(2, 144, np.int32))
        i32 = dict(dtype=torch.int32, device="cuda")
        slots, kept, nkept, sst = torch.zeros((2, 36, 4), **i32), torch.zeros((2, 36, 4), **i32), torch.zeros(2, **i32), torch.zeros(2, **i32)
        enqueue(det, b, d, table, counts, st)
        det.snap_points_enqueue(d_saddles, d["pred"][:2], slots, kept, nkept, sst, 1.0, counts=d_counts, row_counts=d["n_pred"][:2], reverse=True)
        assert det._stream_ptr == s.cuda_stream
    s.synchronize()
    for k in KEYS:
        assert d[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    rec = np.zeros(144, A.SADDLE_DTYPE)
    rec["x"], rec["y"] = saddles[0, :, 0], saddles[0, :, 1]
    for f in range(2):
        k = int(want["n_pred"][f])
        assert want["status"][f] == OK and k == 5
        s_slots, _d, s_rows, _i, s_st = A.snap_points(rec, want["pred"][f, :k], 1.0, reverse=True)
        assert s_st == _ffi.AGX_SNAP_OK and int(sst[f]) == _ffi.AGX_SNAP_OK and int(nkept[f]) == len(s_rows) == 5
        assert np.array_equal(slots[f, :k].cpu().numpy().view(np.uint32), s_slots)
        assert np.array_equal(kept[f, :5].cpu().numpy().view(np.uint32), s_rows)


def test_refused_arguments_leave_the_batch_in_flight(det):
    import torch
    b, _ = EC.gpu_batches()["1x1"]
    d, table, counts, st = device_arrays(b)
    det.saddles_batch_enqueue(torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda"))
    good = PC.camera_args(b.cam)

    def call(cam=good, model=EC.EQUI, tag_size=0.05, iterations=10, null_cam=False, **ptr):
        p = {k: d[k].data_ptr() for k in KEYS}
        p.update(ptr)
        c = None if null_cam else (C.c_double * 9)(*cam)
        return det._lib.agx_board_pose_enqueue_m(det._h, 1, table.data_ptr(), b.tpf, counts.data_ptr(), None, 1, 1, 7, 0.3, float(tag_size), model, c,
                                                 4.0, 0, 1, iterations, 0, *[p[k] for k in KEYS])

    cases = [dict(model=2), dict(model=-1), dict(cam=good[:8] + [1e-300]), dict(cam=good[:8] + [-0.02]), dict(null_cam=True), dict(tag_size=0.0),
             dict(tag_size=np.nan), dict(iterations=65), dict(pose=d["pose"].data_ptr() + 4), dict(best_iter=None), dict(pose=None)]
    for i in range(9):
        for v in (np.nan, np.inf):
            cases.append(dict(cam=good[:i] + [v] + good[i + 1:]))
    cases += [dict(cam=[0.0] + good[1:]), dict(cam=good[:1] + [-1.0] + good[2:])]
    for kw in cases:
        assert call(**kw) == _ffi.AGX_ERR_ARG, kw
    res, _ = det.saddles_batch_fetch()  # still there
    assert len(res) == 1 and all(BC.untouched(d[k].cpu().numpy()) for k in KEYS)
    assert call(iterations=64) == _ffi.AGX_OK
    det.sync()
    with pytest.raises(A.AgxError) as e:
        det.saddles_batch_fetch()
    assert e.value.status == _ffi.AGX_ERR_STATE
    assert int(d["status"][0]) == OK
    # a non-zero ninth double is read as k3 by the radial-tangential model: the same nine doubles pass at AGX_LENS_RADTAN
    assert call(model=EC.RADTAN, cam=good[:8] + [-0.02]) == _ffi.AGX_OK
    det.sync()


def test_recovery_with_an_equidistant_camera_on_a_frame_seen_through_a_fisheye(det):
    """recover_tags_enqueue(camera=Camera.equidistant(...)) on board_pose_equi_cases.warped_frame with four outer-ring tags taken
    out of the table: the table and the pose equal the composition of the host forms byte for byte, and all four come back -- the
    count tests/test_board_pose_equi_cpu.py pins (36), against 34 without a camera."""
    import torch
    luma, cam, _radtan, saddles, tags, (w, h, rows, cols) = EC.warped_frame()
    less = {t: xy for t, xy in tags.items() if t not in EC.WARP_MISSING}
    tpf = 40
    rec = np.ascontiguousarray(saddles).view(np.float32).reshape(-1, 5)

    def run(**kw):
        table = np.zeros((1, tpf), BC.TAG)
        table[0, :len(less)] = BC.tag_rows(less)
        d_tags, d_n = dev(table.view(np.int32).reshape(1, tpf, 9)), dev(np.array([len(less)], np.int32))
        d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        fit = det.recover_tags_enqueue(dev(luma[None]), dev(rec[None]), dev(np.array([len(rec)], np.int32)), None, d_tags, d_n, d_st, cols, rows, **kw)
        det.sync()
        out = d_tags.cpu().numpy().view(BC.TAG).reshape(1, tpf)[0, :int(d_n[0])]
        return {int(r["id"]): r["xy"].reshape(4, 2).copy() for r in out}, fit

    for camera, count in ((cam, 36), (None, 34)):
        got, fit = run(**({} if camera is None else dict(camera=camera)))
        want, hfit = PC.recovered_host(luma, saddles, less, cols, rows, camera=camera)
        assert list(got) == list(want) and len(got) == count
        for t in want:
            assert np.array_equal(np.asarray(got[t], np.float32).view(np.uint32), want[t].view(np.uint32)), t
        if camera is not None:
            assert "pose" in fit and fit["pose"][0].cpu().numpy().tobytes() == hfit["pose"].tobytes() and int(fit["recovered"][0]) == 4
