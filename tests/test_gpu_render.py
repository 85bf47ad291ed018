"""k_render_boards<LENS> on the GPU against its host form, byte for byte -- frames with their guard bytes, truth rows, counts and
statuses (tests/test_render_cpu.py holds the host form to a numpy restatement) -- and the chain without a host step:
render_boards_enqueue -> detect -> board_pose_enqueue -> render again from the returned pose, all on one device batch."""
import numpy as np
import pytest

from tests import render_cases as RC
from tests.test_render_cpu import TRIP_BOUND_PX

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

pytestmark = pytest.mark.gpu

TAG = A.TagDetector.TAG_DTYPE


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def synced(det):
    import torch
    det.sync()
    torch.cuda.synchronize()


def batch_poses(name, layout, n):
    """n poses of the case: the case's own, then the same seen from other sides; with five of them frame 1 is wholly behind the
    camera (AGX_RENDER_EMPTY) and frame 3 has an entry that is not a number (AGX_RENDER_INPUT)"""
    d, tx, ty, rz, off = RC.SMALL_POSES[(name, layout)]
    poses = [A.board_pose_looking_at(d * (1.0 + 0.07 * k), tx + 5.0 * k, ty - 4.0 * k, rz + 31.0 * k, off) for k in range(n)]
    if n == 5:
        poses[1] = (poses[1][0], np.array([0.0, 0.0, -50.0]))  # (beyond the widest cone, 158 degrees)
        poses[3][0][1, 2] = np.nan
    return A.pose_rows(poses)


def both_forms(det, cam, layout, poses, w, h, dtype, S, keep, row_pad, frame_pad, edge_pad, seed, **kw):
    """The same random padded buffer through the host form and through the kernel -> ((buffer, truth, n_truth, status) of each)"""
    import torch
    n, px = len(poses), np.dtype(dtype).itemsize
    rng = np.random.default_rng(seed)
    row, frame = w + row_pad, (w + row_pad) * h + frame_pad
    buf = rng.integers(0, np.iinfo(dtype).max + 1, edge_pad + n * frame + edge_pad, dtype=dtype)
    n_board = layout[0] * layout[1]
    black, white, bg = RC.colours(dtype)
    args = dict(supersample=S, black=black, white=white, background=bg, keep_background=keep, **kw)
    # the host form
    hbuf = buf.copy()
    hview = np.lib.stride_tricks.as_strided(hbuf[edge_pad:], (n, h, w), (frame * px, row * px, px))
    _, htruth, hn, hst = A.render_boards((w, h), layout[0], layout[1], cam, poses, out=hview, **args)
    # the kernel: rows the frame does not write keep the pattern on both sides
    dbuf = torch.from_numpy(buf.view(np.int16) if px == 2 else buf.copy()).cuda()
    dview = dbuf.as_strided((n, h, w), (frame, row, 1), edge_pad)
    truth = torch.zeros((n, n_board, 9), dtype=torch.int32, device="cuda:0")
    n_truth = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    det.render_boards_enqueue(dview, layout[0], layout[1], cam, torch.from_numpy(poses).cuda(), truth, n_truth, status, **args)
    synced(det)
    got = dbuf.cpu().numpy().view(dtype)
    gtruth = truth.cpu().numpy().view(np.uint32).reshape(n, n_board, 9)
    want_truth = np.zeros((n, n_board, 9), np.uint32)
    for f in range(n):
        want_truth[f, :hn[f]] = htruth[f][:hn[f]].view(np.uint32).reshape(-1, 9)
    return (got, gtruth, n_truth.cpu().numpy().astype(np.uint32), status.cpu().numpy().astype(np.uint32)), (hbuf, want_truth, hn, hst)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("name", sorted(RC.SMALL_CAMERAS))
def test_kernel_gives_the_host_forms_bytes(det, name, dtype):
    """Widths 1, 3, 4, 5 and 67, heights 1 and 45, S = 1 .. 4, AGX_RENDER_KEEP_BACKGROUND on and off, batches of 1 and of 5 frames
    with different poses (one AGX_RENDER_EMPTY, one AGX_RENDER_INPUT), tight rows (whole-dword stores where the width allows) and
    padded rows behind an odd offset with guard bytes between rows, between frames and around the batch."""
    cam, layout = RC.SMALL_CAMERAS[name], (2, 3)
    k = 0
    for w in (1, 3, 4, 5, 67):
        for h in (1, 45):
            for keep in (False, True):
                k += 1
                n = 5 if (w, h) == (67, 45) or (w, h, keep) == (4, 1, True) else 1
                aligned = k % 3 == 0  # (a third of the launches takes the whole-dword path where the width is a multiple of 4)
                pads = (0, 0, 0) if aligned and w % 4 == 0 else (4 - w % 4 if aligned else 3, 8 if aligned else 5, 8 if aligned else 11)
                S = 1 + k % 4
                # (the small frames look at the middle of the picture: the principal point moves with the size)
                c = cam._replace(cx=cam.cx - 48.0 + w / 2.0, cy=cam.cy - 40.0 + h / 2.0)
                got, want = both_forms(det, c, layout, batch_poses(name, layout, n), w, h, dtype, S, keep, *pads, seed=k)
                tag = (name, np.dtype(dtype).name, w, h, keep, n, S, pads)
                assert list(want[3]) == ([0, 1, 0, 2, 0] if n == 5 else [0]), tag
                assert np.array_equal(got[3], want[3]) and np.array_equal(got[2], want[2]), tag
                assert np.array_equal(got[1], want[1]), tag
                assert np.array_equal(got[0], want[0]), (tag, int((got[0] != want[0]).sum()))


@pytest.mark.parametrize("layout,first_id", [((1, 1), 586), ((24, 24), 11)])
def test_layouts_up_to_the_code_tables_length(det, layout, first_id):
    """One tag (the family's last code) and the largest square layout T36H11's 587 codes admit, 24 x 24 from id 11 up to the last code.  A 64 x 64 layout asks for 4096 codes, which no family has: AGX_ERR_ARG on both forms."""
    import torch
    cam = A.Camera.equidistant(40.0, 40.0, 33.0, 22.0, -0.013, 0.021, -0.013, 0.0026)
    ext = max(layout) * 1.3
    poses = A.pose_rows([A.board_pose_looking_at(0.9 * ext, 12.0, -9.0, 17.0), A.board_pose_looking_at(0.5 * ext, -20.0, 15.0, 80.0)])
    got, want = both_forms(det, cam, layout, poses, 67, 45, np.uint8, 2, False, 1, 3, 5, seed=9, first_id=first_id)
    assert list(want[3]) == [0, 0] and list(want[2]) == [layout[0] * layout[1]] * 2
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert (want[0] != RC.colours(np.uint8)[2]).sum() > 1000
    frames = torch.zeros((1, 45, 67), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(A.AgxError) as e:
        det.render_boards_enqueue(frames, 64, 64, cam, torch.from_numpy(poses[:1]).cuda(), torch.zeros((1, 4096, 9), dtype=torch.int32, device="cuda:0"),
                                  torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0"))
    assert e.value.status == _ffi.AGX_ERR_ARG
    with pytest.raises(A.AgxError):
        A.render_boards((67, 45), 64, 64, cam, poses[:1])


@pytest.mark.parametrize("name", sorted(RC.TRIP_CAMERAS))
def test_render_detect_pose_render_without_a_host_step(det, name):
    """render_boards_enqueue -> detect_batch_enqueue(out=) -> board_pose_enqueue -> render_boards_enqueue from the returned poses,
    read in place, on one device batch of two frames at the round trip's size: the detected ids are the layout's, the corners and
    the pose's predictions lie within tests/test_render_cpu.py's bound of d_truth, and the second rendering detects the same ids."""
    import torch
    cam = RC.TRIP_CAMERAS[name]
    w, h = RC.TRIP_SIZE
    d, tx, ty, rz, off = RC.TRIP_POSE
    poses = torch.from_numpy(A.pose_rows([RC.looking_at(RC.TRIP_POSE), A.board_pose_looking_at(d * 1.08, -tx, ty + 6.0, rz - 50.0, off)])).cuda()
    n, cap = 2, 64
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda:0")
    frames = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
    truth, n_truth, status = i32(n, 36, 9), i32(n), i32(n)
    det.render_boards_enqueue(frames, 6, 6, cam, poses, truth, n_truth, status, supersample=4)
    tags, counts, tstatus = i32(n, cap, 9), i32(n), i32(n)
    det.detect_batch_enqueue(frames, cap, out=(tags, counts, tstatus))
    det.detect_batch_fetch()
    pose, err_sq, row_status = torch.zeros((n, 12), dtype=torch.float64, device="cuda:0"), torch.zeros((n, cap), device="cuda:0"), i32(n, cap)
    n_inl, rms, best, pred, n_pred, pstatus = i32(n), torch.zeros(n, device="cuda:0"), i32(n), i32(n, 36, 9), i32(n), i32(n)
    det.board_pose_enqueue(tags, counts, 6, 6, cam, pose, err_sq, row_status, n_inl, rms, best, pred, n_pred, pstatus)
    frames2 = torch.zeros_like(frames)
    truth2, n_truth2, status2 = i32(n, 36, 9), i32(n), i32(n)
    det.render_boards_enqueue(frames2, 6, 6, cam, pose, truth2, n_truth2, status2, supersample=4)
    again = det.detect_batch_device(frames2, cap=cap)
    synced(det)
    assert status.tolist() == [0, 0] and n_truth.tolist() == [36, 36] and status2.tolist() == [0, 0] and pstatus.tolist() == [0, 0]
    assert counts.tolist() == [36, 36] and n_pred.tolist() == [36, 36]
    want = truth.cpu().numpy().view(TAG).reshape(n, 36)
    got = tags.cpu().numpy().view(TAG).reshape(n, cap)
    pr = pred.cpu().numpy().view(TAG).reshape(n, 36)
    for f in range(n):
        by_id = {int(r["id"]): r["xy"] for r in got[f][:36]}
        assert sorted(by_id) == list(range(36)) and list(want[f]["id"]) == list(range(36)) and list(pr[f]["id"]) == list(range(36))
        corner = max(float(np.abs(by_id[i].astype(np.float64) - want[f][i]["xy"]).max()) for i in range(36))
        reproj = float(np.abs(pr[f]["xy"].astype(np.float64) - want[f]["xy"]).max())
        print(name, f, "corner error", corner, "reprojection", reproj)
        assert corner < TRIP_BOUND_PX and reproj < TRIP_BOUND_PX
        assert sorted(again[f]) == list(range(36))
    assert np.abs(pose.cpu().numpy() - poses.cpu().numpy()).max() < 0.02 * d
