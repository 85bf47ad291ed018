"""k_rectify_map<AGX_LENS_DOUBLE_SPHERE> and k_rectified_points<AGX_LENS_DOUBLE_SPHERE> on the GPU against their host forms, byte for
byte, padding and guard bytes included (tests/test_rectify_ds_cpu.py holds the host forms to the numpy restatement), with and
without the 60 degree turn that sends the target's far columns past the image plane; and remap -> detect on the device through
the double-sphere map against detect_batch of the host form's rectified frames."""
import functools

import numpy as np
import pytest

from tests import board_pose_cases as PC
from tests import board_pose_ds_cases as DC
from tests import rectify_cases as RC
from tests.rectify_cases import NEW_CAMERA, NONE, SRC
from tests.test_rectify_ds_cpu import CAMERAS, TURN

import aprilgrid_rs_amd as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def synced(det):
    import torch
    det.sync()
    torch.cuda.synchronize()


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("dst", [(97, 61), (5, 3)])
@pytest.mark.parametrize("lens", ["wide", "tele"])
def test_map_kernel_gives_the_host_forms_bytes(det, lens, dst, rotated):
    import torch
    cam, R = CAMERAS[lens], TURN if rotated else None
    stride = 8 * dst[0] + 24
    want = A.rectify_map(cam, SRC, dst, NEW_CAMERA, R, row_stride=stride)
    buf = torch.full((dst[1], stride // 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
    out = buf[:, :2 * dst[0]].unflatten(1, (dst[0], 2))
    got = det.rectify_map_enqueue(cam, SRC, dst, NEW_CAMERA, R, out=out)
    synced(det)
    assert got is out
    assert buf.cpu().numpy().tobytes() == want.base.tobytes()
    if rotated and lens == "wide" and dst == (97, 61):  # the far columns: rays with Z <= 0, and entries all the same
        i, j = np.meshgrid(np.arange(dst[0]), np.arange(dst[1]))
        behind = RC.rays(NEW_CAMERA, R, i, j)[..., 2] <= 0.0
        assert behind.sum() > 1000 and (want[behind] != NONE).all()


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("n", [1, 63, 130])
def test_points_kernel_gives_the_host_forms_bytes(det, n, rotated):
    """A list between guard points on both sides: points across and beyond the target, a NaN and an infinite one."""
    import torch
    cam, R = CAMERAS["wide"], TURN if rotated else PC.rotation(0.0, 150.0, 0.0)  # (the second: many rays outside the cone)
    rng = np.random.RandomState(n)
    pts = (rng.rand(n, 2) * [97 * 3, 61] - [97, 0]).astype(np.float32)
    if n > 10:
        pts[5], pts[6] = (np.nan, 3.0), (2.0, np.inf)
    want = A.rectified_points(pts, cam, NEW_CAMERA, R)
    if n > 10:
        assert np.isnan(want[5]).all() and np.isfinite(want).any()
    src = np.full((n + 2, 2), np.float32(-7.5), np.float32)  # a guard point at each end of both lists
    src[1:-1] = pts
    dst = np.full((n + 2, 2), np.float32(-9.25), np.float32)
    s_d, d_d = dev(src), dev(dst)
    got = det.rectified_points_enqueue(s_d[1:-1], cam, NEW_CAMERA, R, out=d_d[1:-1])
    synced(det)
    dst[1:-1] = want
    assert d_d.cpu().numpy().tobytes() == dst.tobytes() and s_d.cpu().numpy().tobytes() == src.tobytes()
    assert got.cpu().numpy().tobytes() == want.tobytes()


def warp(img, pinhole, cam):
    """The frame `pinhole` (fx, fy, cx, cy) rendered as the double-sphere `cam` would have seen it: every output pixel goes to its
    ray by the restated unprojection and samples the pinhole frame there, order 1."""
    from scipy.ndimage import map_coordinates
    v, u = np.mgrid[0:img.shape[0], 0:img.shape[1]].astype(np.float64)
    ray = DC.unproject(cam, u, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(ray[..., 2] > 1e-3, ray[..., 2], np.nan)
        ui, vi = pinhole[0] * ray[..., 0] / z + pinhole[2], pinhole[1] * ray[..., 1] / z + pinhole[3]
    out = map_coordinates(img.astype(np.float64), [np.nan_to_num(vi, nan=-1e6), np.nan_to_num(ui, nan=-1e6)], order=1, mode="constant", cval=128.0)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


WARP_FOCAL = 0.6  # the lens's focal length near the axis, fx / (1 + xi), as a fraction of the rendered pinhole's


@functools.lru_cache(maxsize=None)
def ds_frames():
    from tests import board_fit_cases as BC
    img, gt, tags, (w, h, rows, cols) = BC.frame(1)
    K = PC.camera_of(A.board_fit(BC.tag_rows(tags), cols, rows, (w, h))["H"], w, h)
    xi, alpha = DC.XI_ALPHA["mid"]
    cam = A.Camera.double_sphere(K[0] * WARP_FOCAL * (1.0 + xi), K[1] * WARP_FOCAL * (1.0 + xi), K[2], K[3], xi, alpha)
    luma = warp(img, K, cam)
    return np.stack([luma, np.roll(luma, 3, axis=1)]), cam, K, (w, h)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for t in x:
            assert np.asarray(x[t]).tobytes() == np.asarray(y[t]).tobytes()


def test_remap_then_detect_on_the_device(det):
    """Two L8 frames behind a double-sphere lens, rectified to the rendered pinhole: the device's map is the host form's,
    remap_enqueue followed by detect_batch_enqueue equals detect_batch of the host form's rectified frames, and so does
    detect_rectified."""
    frames, cam, K, (w, h) = ds_frames()
    m = A.rectify_map(cam, (w, h), new_camera=K)
    rect = A.remap(frames, m)
    want = det.detect_batch(rect)
    assert min(len(f) for f in want) >= 15
    m_d = det.rectify_map_enqueue(cam, (w, h), new_camera=K)
    rect_d = det.remap_enqueue(dev(frames), m_d)
    det.detect_batch_enqueue(rect_d)
    got = det.detect_batch_fetch()
    assert m_d.cpu().numpy().tobytes() == m.tobytes() and rect_d.cpu().numpy().tobytes() == rect.tobytes()
    _same(got, want)
    _same(det.detect_rectified(dev(frames), cam, new_camera=K), want)
