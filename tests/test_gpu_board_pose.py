"""agx_board_pose_enqueue (k_board_pose) on the GPU: every output array against the host form agx_board_pose_tail byte for byte,
FILL bytes beyond and between what a frame may write included (tests/test_board_pose_cpu.py holds the host form to a scipy
least-squares pose).  This is also the test that decides whether the binary64 square root of the two compilers agrees
(csrc/board_pose_math.h: pose_sqrt).  The layout, the camera, iterations, max_drop and the flag are scalars of a call, so their
combinations are a handful of launches of at most 16 frames, each with every frame status (tests/board_pose_cases.py:
gpu_batches); the launches under the cameras "full" and "k3" decide the same for the k3 and tangential products, which under the
other cameras are products with 0 or 1e-3, and the _wrap launches run spacing ratios 1, -0.5 and 0 on an id window that passes
2^32.  Then the pose's predicted rows snapped on the caller's stream, the refused arguments, the recovery without a
camera pinned to the bytes of board_fit's path, and the recovery with a camera on a frame seen through a barrel lens."""
import numpy as np
import pytest

from tests import board_fit_cases as BC
from tests import board_pose_cases as PC
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
    n = b.n
    det.board_pose_enqueue(table, counts, b.cols, b.rows, b.cam, *[d[k][:n] for k in KEYS], tag_size=b.tag_size, first_id=b.first_id,
                           spacing_ratio=b.s, max_err_sq=b.max_err_sq, max_drop=b.max_drop, min_tags=b.min_tags, iterations=b.iterations,
                           predict_missing=bool(b.flags & PC.MISSING), tag_status=st)


@pytest.mark.parametrize("name", sorted(PC.gpu_batches()))
def test_the_kernel_gives_the_host_forms_bytes(det, name):
    import torch
    b, status = PC.gpu_batches()[name]
    want = b.host()
    d, table, counts, st = device_arrays(b)
    enqueue(det, b, d, table, counts, st)
    det.sync()
    torch.cuda.synchronize()
    for k in KEYS:
        got = d[k].cpu().numpy()
        assert got.tobytes() == want[k].tobytes(), "%s: %s differs from the host form" % (name, k)
    # what the launch covers, read from the host form's answer (the bytes above are the device's too)
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
    """A second launch, on the caller's stream: the pose's rows of the missing tags go to snap_points_enqueue as they stand."""
    pose_then_snap(det, "barrel", 0)


def test_predicted_rows_with_wrapped_ids_feed_the_snap(det):
    """The same chain under camera "full" with the layout from 0xFFFFFFF0: the missing tags 0, 5, 17, 30, 35 have the ids
    0xFFFFFFF0, 0xFFFFFFF5, 1, 14, 19, which a second kernel reads in place."""
    want = pose_then_snap(det, "full", PC.WRAP_FIRST_ID)
    for f in range(2):
        assert want["pred"][f, :5]["id"].tolist() == [0xFFFFFFF0, 0xFFFFFFF5, 1, 14, 19]


def pose_then_snap(det, camera, first_id):
    import torch
    cam = PC.CAMERAS[camera]
    R, t = PC.pose("near", 6, 6)
    full = PC.exact_table(6, 6, range(36), cam, R, t, first_id=first_id, noise=0.1)
    keep = np.array([i for i in range(36) if i not in (0, 5, 17, 30, 35)])
    b = PC.PoseBatch("snap", [full[keep], full[keep][::-1]], 6, 6, cam, first_id=first_id, max_drop=1, flags=PC.MISSING, tpf=36)
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
    return want


def test_refused_arguments_leave_the_batch_in_flight(det):
    import ctypes as C
    import torch
    b, _ = PC.gpu_batches()["1x1"]
    d, table, counts, st = device_arrays(b)
    det.saddles_batch_enqueue(torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda"))
    good = PC.camera_args(b.cam)

    def call(cam=good, tag_size=0.05, iterations=10, null_cam=False, **ptr):
        p = {k: d[k].data_ptr() for k in KEYS}
        p.update(ptr)
        c = None if null_cam else (C.c_double * 9)(*cam)
        return det._lib.agx_board_pose_enqueue(det._h, 1, table.data_ptr(), b.tpf, counts.data_ptr(), None, 1, 1, 7, 0.3, float(tag_size), c, 4.0, 0, 1,
                                               iterations, 0, *[p[k] for k in KEYS])

    cases = [dict(null_cam=True), dict(tag_size=0.0), dict(tag_size=-1.0), dict(tag_size=np.nan), dict(tag_size=np.inf), dict(iterations=65),
             dict(pose=d["pose"].data_ptr() + 4), dict(best_iter=None), dict(pose=None)]
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


def test_recovery_without_a_camera_returns_todays_bytes(det):
    """camera=None is the path of the parent commit: recover_tags_enqueue and detect_recovered on the 4 x 7 frame equal the
    restatement over board_fit's host form, and the fit dict carries h, not pose."""
    import torch
    from oracle import oracle as O
    img, gt, tags, (w, h, rows, cols) = BC.frame(0)
    s = O.refined_saddle_points(img)
    table = np.zeros((1, 40), BC.TAG)
    less = {t: xy for t, xy in tags.items() if t not in (9, 17)}
    table[0, :len(less)] = BC.tag_rows(less)
    d_tags, d_n, d_st = dev(table.view(np.int32).reshape(1, 40, 9)), dev(np.array([len(less)], np.int32)), torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = np.ascontiguousarray(s).view(np.float32).reshape(-1, 5)
    fit = det.recover_tags_enqueue(dev(img[None]), dev(rec[None]), dev(np.array([len(rec)], np.int32)), None, d_tags, d_n, d_st, cols, rows)
    det.sync()
    want, hfit = BC.recovered_host(img, s, less, cols, rows)
    assert "h" in fit and "pose" not in fit and fit["h"][0].cpu().numpy().tobytes() == hfit["H"].tobytes()
    out = d_tags.cpu().numpy().view(BC.TAG).reshape(1, 40)[0, :int(d_n[0])]
    assert [int(r["id"]) for r in out] == list(want) and all(np.array_equal(r["xy"].reshape(4, 2).view(np.uint32), want[int(r["id"])].view(np.uint32)) for r in out)
    got, fits = det.detect_recovered(dev(img[None]), cols, rows, return_fit=True)
    want, hfit = BC.recovered_host(img, s, tags, cols, rows)
    assert list(got[0]) == list(want) and fits[0]["H"].tobytes() == hfit["H"].tobytes() and "pose" not in fits[0]
    for t in want:
        assert np.array_equal(np.asarray(got[0][t], np.float32).view(np.uint32), want[t].view(np.uint32))


def test_detect_recovered_on_a_board_whose_ids_start_at_100(det):
    """first_id through detect_recovered, with and without a camera, on a rendered 6 x 6 frame printed with the ids 100 .. 135:
    the tags and the fit equal the restatement over the host forms bit for bit."""
    luma, saddles, tags, cam = PC.frame_from_100()
    for camera in (None, cam):
        got, fits = det.detect_recovered(dev(luma[None]), 6, 6, first_id=PC.FRAME_FIRST_ID, camera=camera, return_fit=True)
        want, hfit = PC.recovered_host(luma, saddles, tags, 6, 6, camera=camera, first_id=PC.FRAME_FIRST_ID)
        assert list(got[0]) == list(want) and sorted(want) == list(range(100, 136))
        for t in want:
            assert np.array_equal(np.asarray(got[0][t], np.float32).view(np.uint32), want[t].view(np.uint32)), t
        assert fits[0]["status"] == hfit["status"] == OK and fits[0]["n_inliers"] == 36
        key = "H" if camera is None else "pose"
        assert fits[0][key].tobytes() == hfit[key].tobytes() and fits[0]["err_sq"].tobytes() == hfit["err_sq"].tobytes()


def test_on_a_warped_frame_the_camera_recovers_strictly_more_tags(det):
    """The rendered 6 x 6 frame seen through the strong barrel (board_pose_cases.warped_frame), four outer-ring tags taken out of
    detect_staged's table: recover_tags_enqueue(camera=) brings back all four, without a camera two -- the counts
    tests/test_board_pose_cpu.py establishes on the host forms from the oracle's saddle list -- and both tables, the pose and
    detect_recovered(camera=) equal the composition of the host forms byte for byte."""
    import torch
    luma, cam, saddles, tags, (w, h, rows, cols) = PC.warped_frame()
    staged = det.detect_staged(dev(luma[None]))[0]
    assert list(staged) == list(tags) and all(np.array_equal(np.asarray(staged[t], np.float32).view(np.uint32), tags[t].view(np.uint32)) for t in tags)
    less = {t: xy for t, xy in staged.items() if t not in PC.WARP_MISSING}
    assert len(less) == 32
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

    def same(got, want):
        assert list(got) == list(want)
        for t in want:
            assert np.array_equal(np.asarray(got[t], np.float32).view(np.uint32), want[t].view(np.uint32)), t

    with_cam, fit = run(camera=cam)
    without, plain_fit = run()
    want_cam, hfit = PC.recovered_host(luma, saddles, less, cols, rows, camera=cam)
    want_plain, _ = PC.recovered_host(luma, saddles, less, cols, rows)
    same(with_cam, want_cam)
    same(without, want_plain)
    assert len(with_cam) == 36 and len(without) == 34 and len(with_cam) > len(without)
    assert "pose" in fit and "h" not in fit and "h" in plain_fit and fit["pose"][0].cpu().numpy().tobytes() == hfit["pose"].tobytes()
    assert int(fit["best_iter"][0]) == hfit["best_iter"] and int(fit["recovered"][0]) == 4 and int(plain_fit["recovered"][0]) == 2
    # detect_recovered: nothing is missing from detect_staged's own table, so the camera only changes the fit that is returned
    got, fits = det.detect_recovered(dev(luma[None]), cols, rows, camera=cam, return_fit=True)
    full, hfull = PC.recovered_host(luma, saddles, tags, cols, rows, camera=cam)
    same(got[0], full)
    assert fits[0]["status"] == OK and fits[0]["pose"].tobytes() == hfull["pose"].tobytes() and fits[0]["best_iter"] == hfull["best_iter"] and "H" not in fits[0]
