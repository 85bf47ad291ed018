"""What tests/test_rectify_cpu.py and tests/test_gpu_rectify.py share: small cameras of both lens models, a numpy float64 statement
of the rectification map (np.arctan / np.sqrt, written independently of csrc/rectify_math.h), a numpy integer statement of the
remap, the caller's maps with entries at and beyond the source's limits, and board_pose_equi_cases' rendered frame rebuilt behind
fisheyes of other focal lengths."""
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import board_pose_cases as PC
from tests import board_pose_equi_cases as PE

NONE = _ffi.AGX_MAP_NONE
SRC = (83, 59)  # (w, h): odd, no multiple of the remap's four pixels a lane
DST = (97, 61)
# the target pinhole of the small cases: its corners look past the 83 x 59 source, so every map has entries without a source pixel
NEW_CAMERA = (50.0, 50.0, 47.5, 30.2)
ROTATION = PC.rotation(3.0, -2.0, 4.0)
# radtan: |r| reaches 1.03 in the target's corners, where d(r rad)/dr = 1 - 0.36 r^2 + 0.15 r^4 = 0.77 > 0: inside the monotone radius
CAMERAS = {
    "radtan": A.Camera(60.0, 62.0, 41.3, 28.7, -0.12, 0.03, 0.001, -0.0007, 0.0),
    "equi": A.Camera.equidistant(62.0, 63.0, 40.6, 29.2, -0.013, 0.021, -0.013, 0.0026),
}
PINHOLE = A.Camera(70.0, 70.0, 41.0, 29.0)


def rays(new_camera, rotation, x, y):
    """Rectified positions (x, y) -> camera-frame points [..., 3]: ((x - cx') / fx', (y - cy') / fy', 1) turned by rotation."""
    fx, fy, cx, cy = [float(v) for v in new_camera]
    d = np.stack([(np.asarray(x, np.float64) - cx) / fx, (np.asarray(y, np.float64) - cy) / fy, np.ones(np.shape(x))], axis=-1)
    return d if rotation is None else d @ np.asarray(rotation, np.float64).reshape(3, 3).T


def numpy_points(cam, new_camera, rotation, x, y):
    """-> (uv [..., 2] float64 with NaN where Z is not > 0, Z) under the camera's model, numpy float64."""
    Q = rays(new_camera, rotation, x, y)
    with np.errstate(invalid="ignore", divide="ignore"):
        uv = PE.project_rays(cam, Q) if cam.model == PE.EQUI else PC.project(cam, np.eye(3), np.zeros(3), Q)
    return uv, Q[..., 2]


def numpy_map(cam, src, dst, new_camera, rotation):
    """-> (uv [dst_h, dst_w, 2] float64, valid bool, near bool: within 1e-9 px of a validity boundary (or Z within 1e-9 of 0))."""
    i, j = np.meshgrid(np.arange(dst[0]), np.arange(dst[1]))
    uv, z = numpy_points(cam, new_camera, rotation, i, j)
    lim = np.array([src[0] - 1, src[1] - 1], np.float64) + 1.0 / 64.0
    fin = np.isfinite(uv).all(-1)
    with np.errstate(invalid="ignore"):
        valid = fin & (uv >= -1.0 / 64.0).all(-1) & (uv < lim).all(-1)
        near = (fin & ((np.abs(uv + 1.0 / 64.0) < 1e-9).any(-1) | (np.abs(uv - lim) < 1e-9).any(-1))) | (np.abs(z) < 1e-9)
    return uv, valid, near


def numpy_remap(img, m, border):
    """The remap in numpy integers: img [N, H, W] uint8 / uint16, m int32 [dh, dw, 2] -> [N, dh, dw] of img's dtype."""
    n, h, w = img.shape
    mx, my = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    ok = (mx >= 0) & (my >= 0) & (mx <= 32 * (w - 1)) & (my <= 32 * (h - 1))
    mx, my = np.where(ok, mx, 0), np.where(ok, my, 0)
    x0, y0, ax, ay = mx >> 5, my >> 5, mx & 31, my & 31
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    p = img.astype(np.int64)
    v = ((32 - ax) * (32 - ay) * p[:, y0, x0] + ax * (32 - ay) * p[:, y0, x1] + (32 - ax) * ay * p[:, y1, x0] + ax * ay * p[:, y1, x1] + 512) >> 10
    return np.where(ok, v, border).astype(img.dtype)


def image(n, size, dtype, seed=3):
    """n frames of smooth structure plus noise, with the extremes 0 and the dtype's maximum present."""
    w, h = size
    rng = np.random.RandomState(seed)
    top = np.iinfo(dtype).max
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w), dtype)
    for f in range(n):
        v = 0.5 + 0.5 * np.sin(x * (0.21 + 0.03 * f) + y * 0.13) * np.cos(y * 0.17 - f)
        out[f] = np.clip(v * top + rng.randint(-top // 16, top // 16 + 1, (h, w)), 0, top).astype(dtype)
        out[f, f % h, :4] = (0, top, 0, top)
    return out


def padded(a, row_pad, frame_pad, fill=0xA5):
    """A copy of a [N, H, W] as a view into a buffer with row_pad extra bytes a row and frame_pad a frame, the rest `fill`
    -> (view, the whole buffer as bytes)."""
    n, h, w = a.shape
    px = a.itemsize
    row, frame = w * px + row_pad, (w * px + row_pad) * h + frame_pad
    buf = np.full(n * frame, fill, np.uint8)
    assert row % px == 0 and frame % px == 0
    view = np.lib.stride_tricks.as_strided(buf.view(a.dtype), a.shape, (frame, row, px))
    view[...] = a
    return view, buf


def callers_map(src, dst):
    """A caller's own map: entries exactly at 32 (src - 1) in x, in y and in both, one past them, negative ones, one word
    AGX_MAP_NONE and the other valid, INT32_MAX -- over a smooth shear of the source -- and the entry kinds it holds."""
    (sw, sh), (dw, dh) = src, dst
    i, j = np.meshgrid(np.arange(dw), np.arange(dh))
    m = np.stack([(i * 32 * (sw - 1)) // max(dw - 1, 1) + (j % 7), (j * 32 * (sh - 1)) // max(dh - 1, 1) + (i % 5)], axis=-1).astype(np.int32)
    m[..., 0] = np.minimum(m[..., 0], 32 * (sw - 1))
    m[..., 1] = np.minimum(m[..., 1], 32 * (sh - 1))
    ex, ey = 32 * (sw - 1), 32 * (sh - 1)
    special = [(ex, 40), (40, ey), (ex, ey), (ex + 1, 40), (40, ey + 1), (-1, 40), (40, -1), (NONE, 40), (40, NONE), (NONE, NONE),
               (2 ** 31 - 1, 2 ** 31 - 1), (ex - 1, ey - 1), (0, 0), (31, 31)]
    flat = m.reshape(-1, 2)
    for k, e in enumerate(special):
        if k * 3 + 1 < len(flat):
            flat[k * 3 + 1] = e
    return m


@functools.lru_cache(maxsize=None)
def fisheye_frame(ratio):
    """board_pose_equi_cases.warped_frame's rendered 6 x 6 frame behind an equidistant lens of `ratio` times the rendered pinhole's
    focal length (0.62 is that case itself) -> (luma, the equidistant camera, ground truth {id: 4x2 float64} in the fisheye
    frame's pixels, (w, h))."""
    from tests import board_fit_cases as BC
    img, gt, tags, (w, h, rows, cols) = BC.frame(1)
    K = PC.camera_of(A.board_fit(BC.tag_rows(tags), cols, rows, (w, h))["H"], w, h)
    cam = A.Camera.equidistant(K[0] * ratio, K[1] * ratio, K[2], K[3], -0.013, 0.021, -0.013, 0.0026)
    luma = PE.warp(img, K, cam)
    truth = {}
    for t, xy in gt.items():
        xy = np.asarray(xy, np.float64).reshape(4, 2)[::-1]  # (the renderer lists a tag's corners in the reverse of detect's order)
        Q =np.stack([(xy[:, 0] - K[2]) / K[0], (xy[:, 1] - K[3]) / K[1], np.ones(4)], axis=-1)
        truth[int(t)] = PE.project_rays(cam, Q)
    return luma, cam, truth, (w, h)


def numpy_rectified(luma, cam):
    """The frame rectified with numpy at the camera's own focal length and size: positions quantised to 1/32 px, then
    scipy's map_coordinates(order=1), rounded to nearest (the table of the feature's issue)."""
    from scipy.ndimage import map_coordinates
    h, w = luma.shape
    uv, valid, _ = numpy_map(cam, (w, h), (w, h), cam[:4], None)
    q = np.floor(np.where(valid[..., None], uv, 0.0) * 32.0 + 0.5) / 32.0
    out = np.rint(map_coordinates(luma.astype(np.float64), [q[..., 1], q[..., 0]], order=1, mode="nearest"))
    return np.where(valid, np.clip(out, 0, 255), 0).astype(np.uint8)


def corner_errors(found, truth):
    """{id: 4x2} against the ground truth -> the corner distances of the ids in both, one array."""
    ids = sorted(set(found) & set(truth))
    return np.concatenate([np.linalg.norm(np.asarray(found[t], np.float64).reshape(4, 2) - truth[t], axis=1) for t in ids]) if ids else np.zeros(0)
