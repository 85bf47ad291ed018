"""What tests/test_board_pose_equi_cpu.py and tests/test_gpu_board_pose_equi.py share: the equidistant cameras, a numpy float64
statement of the pinhole-equidistant projection (np.arctan, np.sqrt) written independently of csrc/board_pose_math.h, tables and
the scipy yardstick through it, a batch answered by agx_board_pose_tail_m, the launches of the GPU suite (board_pose_cases's
construction under the equidistant cameras, and the frames on the optical axis and at the small-r threshold), and a rendered frame
warped through a fisheye with its inverse model."""
import ctypes as C
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import board_pose_cases as PC
from tests.board_pose_cases import FEW, INPUT, LOOSE, MISSING, OK, SINGULAR, TAG, TAG_SIZE

RADTAN, EQUI = _ffi.AGX_LENS_RADTAN, _ffi.AGX_LENS_EQUIDISTANT
SMALL_R2 = 2.0 ** -13  # csrc/board_pose_math.h: POSE_EQUI_SMALL_R2
THETA_MAX = 1.5        # POSE_EQUI_THETA_MAX
# 800 x 600 as board_pose_cases.  "zero": the pure equidistant map.  "kalibr": coefficients of the size Kalibr reports for a
# pinhole-equi camera.  "four": four coefficients of distinct magnitudes, so each product of D and D' shows in the bytes.
# "wide": fx = 0.3 of the width -- the image's corner lies at theta_d = 2.08 rad and a near board's corners pass 70 degrees.
CAMERAS = {
    "zero": A.Camera.equidistant(400.0, 400.0, 400.0, 300.0),
    "kalibr": A.Camera.equidistant(400.0, 410.0, 395.0, 305.0, -0.013, 0.021, -0.013, 0.0026),
    "four": A.Camera.equidistant(380.0, 420.0, 410.0, 290.0, -0.04, 0.012, -0.003, 0.0007),
    "wide": A.Camera.equidistant(240.0, 240.0, 400.0, 300.0, -0.01, 0.002, -0.0005, 0.0001),
}
# a board so near that its outer corners lie beyond 70 degrees off the axis (t in units of the board's larger extent)
VNEAR = ((4.0, -5.0, 2.0), (0.0, 0.0, 0.24))


def project(cam, R, t, P):
    """Points P [..., 3] of the board -> pixels [..., 2] under cam.model; NaN where Z is not > 0."""
    if getattr(cam, "model", RADTAN) != EQUI:
        return PC.project(cam, R, t, P)
    Q = P @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    return project_rays(cam, Q)


def project_rays(cam, Q):
    """Camera-frame points Q [..., 3] -> pixels, the equidistant model with np.arctan / np.sqrt."""
    fx, fy, cx, cy, k1, k2, k3, k4, _ = [float(v) for v in cam]
    z = np.where(Q[..., 2] > 0.0, Q[..., 2], np.nan)
    x, y = Q[..., 0] / z, Q[..., 1] / z
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    thd = th * (1.0 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r > 0.0, thd / np.where(r > 0.0, r, 1.0), 1.0)
    return np.stack([fx * s * x + cx, fy * s * y + cy], axis=-1)


def library_project(cam, Q, model=None):
    """agx_debug_pose_project: the host form's pose_project of camera-frame points Q [n, 3] -> [n, 2] float64."""
    Q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    uv = np.zeros((len(Q), 2), np.float64)
    rc = _ffi.lib().agx_debug_pose_project(cam.model if model is None else model, (C.c_double * 9)(*[float(v) for v in cam]), Q.ctypes.data, len(Q),
                                           uv.ctypes.data)
    assert rc == _ffi.AGX_OK, rc
    return uv


def pose_of(spec, cols, rows, tag_size=TAG_SIZE, s=0.3):
    ang, t = spec
    return PC.rotation(*ang), np.asarray(t, np.float64) * PC.extent(cols, rows, s, tag_size)


def exact_table(cols, rows, ids, cam, R, t, tag_size=TAG_SIZE, first_id=0, s=0.3, noise=0.0, seed=1):
    """board_pose_cases.exact_table through `project` (either model)."""
    ids = np.asarray(ids, np.int64)
    uv = project(cam, R, t, PC.board_points(cols, rows, s, tag_size)[ids])
    if noise:
        uv = uv + noise * PC.splitmix64(uv.size, seed).reshape(uv.shape)
    out = np.zeros(len(ids), TAG)
    out["id"] = PC.wrapped_ids(first_id, ids)
    out["xy"] = uv.reshape(len(ids), 8).astype(np.float32)
    return out


def yardstick(table, cols, rows, cam, R0, t0, tag_size=TAG_SIZE, first_id=0, s=0.3):
    """board_pose_cases.yardstick through `project`: scipy's least-squares pose from (R0, t0) -> (R, t, sum of |e|^2)."""
    from scipy.optimize import least_squares
    P = PC.board_points(cols, rows, s, tag_size)[PC.layout_index(table["id"], first_id)]
    obs = table["xy"].astype(np.float64).reshape(-1, 4, 2)

    def res(p):
        return (project(cam, PC.rodrigues(p[:3]) @ R0, p[3:], P) - obs).ravel()

    sol = least_squares(res, np.concatenate([np.zeros(3), t0]), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return PC.rodrigues(sol.x[:3]) @ R0, sol.x[3:], float(np.sum(res(sol.x) ** 2))


def field_angle(R, t, P):
    """The largest angle off the optical axis of the board points P under the pose, degrees."""
    Q = P @ np.asarray(R).T + np.asarray(t)
    return float(np.degrees(np.arctan2(np.hypot(Q[..., 0], Q[..., 1]), Q[..., 2])).max())


class EquiBatch(PC.PoseBatch):
    """board_pose_cases.PoseBatch answered by agx_board_pose_tail_m under the camera's model."""

    def host(self, model=None):
        out, table = self.empty_outputs(), self.table()
        u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        cam = (C.c_double * 9)(*PC.camera_args(self.cam))
        model = getattr(self.cam, "model", RADTAN) if model is None else model
        for f in range(self.n):
            st = _ffi.AGX_TAGS_OK if self.tag_status is None else self.tag_status[f]
            rc = _ffi.lib().agx_board_pose_tail_m(
                table[f].ctypes.data, self.tpf, self.counts[f], st, self.cols, self.rows, self.first_id, float(self.s), float(self.tag_size), model, cam,
                float(self.max_err_sq), self.max_drop, self.min_tags, self.iterations, self.flags, out["pose"][f].ctypes.data,
                out["err_sq"][f].ctypes.data, out["row_status"][f].ctypes.data, C.cast(out["n_inliers"][f:].ctypes.data, u32),
                C.cast(out["rms"][f:].ctypes.data, f32), C.cast(out["best_iter"][f:].ctypes.data, u32), out["pred"][f].ctypes.data,
                C.cast(out["n_pred"][f:].ctypes.data, u32), C.cast(out["status"][f:].ctypes.data, u32))
            assert rc == _ffi.AGX_OK, (self.name, f, rc)
        return out


# the launches whose statuses are not the construction's nominal ones, as the host form gives them, pinned: at iterations = 0 the
# answer is the seed (board_pose_cases.SEED_ONLY_STATUS says why a lone far tag is LOOSE there)
PINNED_STATUS = {
    "64x64_zero_it0_drop0_all": [LOOSE] + [OK] * 8 + [LOOSE, FEW, SINGULAR, INPUT, INPUT, INPUT],
    "6x6_zero_it0_drop2_missing": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT, LOOSE],
}


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """board_pose_cases.gpu_batches under the four equidistant cameras: name -> (EquiBatch, the statuses its frames must have)."""
    out = {}
    rng = np.random.RandomState(7)
    R, t = PC.pose("tilt40", 64, 64, 0.01)
    ids = rng.permutation(4096)[:587]
    for cam, it, drop, flags in (("kalibr", 10, 2, MISSING), ("zero", 0, 0, 0), ("four", 10, 2, MISSING), ("wide", 5, 1, 0)):
        full = exact_table(64, 64, ids, CAMERAS[cam], R, t, 0.01, first_id=5, noise=0.05)
        off = full[:3].copy()
        off["id"] = [4, 5 + 4096, 0xFFFFFFFF]
        tables = [full[:n] for n in (1, 4, 36, 63, 64, 65, 129, 587)]
        status = [OK] * 8
        tables.append(np.concatenate([off[:2], full[:40], off[2:]]))
        status.append(OK)
        tables.append(PC._wrong(full[:36], drop + 1))
        status.append(LOOSE)
        if drop:
            tables.append(PC._wrong(full[:70], 1))
            status.append(OK)
        tables += [full[:0], PC.flat_row(full), PC.nan_row(full[:20])]
        status += [FEW, SINGULAR, INPUT]
        counts = [len(x) for x in tables] + [601, 10]
        tables += [full[:10], full[:10]]
        status += [INPUT, INPUT]
        tag_status = [0] * (len(tables) - 1) + [_ffi.AGX_TAGS_CAPACITY]
        name = "64x64_%s_it%d_drop%d_%s" % (cam, it, drop, "missing" if flags else "all")
        out[name] = (EquiBatch(name, tables, 64, 64, CAMERAS[cam], 0.01, first_id=5, max_drop=drop, iterations=it, flags=flags, counts=counts,
                               tag_status=tag_status, tpf=600), PINNED_STATUS.get(name, status))
    for cam, it, drop, flags in (("zero", 10, 0, MISSING), ("zero", 0, 2, MISSING), ("kalibr", 10, 2, 0), ("kalibr", 5, 0, MISSING),
                                 ("four", 10, 2, MISSING), ("four", 0, 0, 0), ("wide", 10, 0, 0), ("wide", 5, 2, MISSING)):
        tables, status = [], []
        poses = [PC.POSES[p] for p in sorted(PC.POSES)] + ([VNEAR] if cam == "wide" else [])
        for k, spec in enumerate(poses):
            R, t = pose_of(spec, 6, 6)
            full = exact_table(6, 6, range(36), CAMERAS[cam], R, t, noise=0.1, seed=k + 1)
            tables.append(full[rng.permutation(36)[:36 - 5 * min(k, 4)]])
            status.append(OK)
        base = tables[0]
        tables += [PC._wrong(base, drop + 1), base[:0], PC.flat_row(base), PC.nan_row(base)]
        status += [LOOSE, FEW, SINGULAR, INPUT]
        if drop:
            tables.append(PC._wrong(base, 1))
            status.append(OK)
        name = "6x6_%s_it%d_drop%d_%s" % (cam, it, drop, "missing" if flags else "all")
        out[name] = (EquiBatch(name, tables, 6, 6, CAMERAS[cam], max_drop=drop, iterations=it, flags=flags, tpf=40), PINNED_STATUS.get(name, status))
    R, t = PC.pose("tilt40", 1, 1)
    one = exact_table(1, 1, [0], CAMERAS["kalibr"], R, t, first_id=7)
    out["1x1"] = (EquiBatch("1x1", [one, one[:0], PC.flat_row(one)], 1, 1, CAMERAS["kalibr"], first_id=7, flags=MISSING, tpf=3), [OK, FEW, SINGULAR])
    out["6x6_kalibr_axis_and_threshold"] = (EquiBatch("axis", axis_tables(CAMERAS["kalibr"]), 6, 6, CAMERAS["kalibr"], flags=MISSING, tpf=40), [OK] * 3)
    return out


def axis_pose(r, corner=(14, 2), rz=3.0, z=0.28):
    """A fronto-parallel pose (turned by rz degrees about the axis) under which the 6 x 6 board's corner `corner` (tag, corner:
    tag 14's corner 2 is the inner corner nearest the board's centre) lies at the normalised radius r from the optical axis."""
    R = PC.rotation(0.0, 0.0, rz)
    P0 = PC.board_points(6, 6, tag_size=TAG_SIZE)[corner[0], corner[1]]
    return R, np.array([r * z, 0.0, z]) - R @ P0


def axis_tables(cam):
    """Exact tables of three frames: a corner observed exactly on the optical axis (its pixel is (cx, cy): the seed's
    theta_d = 0), and the same corner just inside and just outside the small-r threshold r^2 = 2^-13."""
    out = []
    for r in (0.0, np.sqrt(SMALL_R2) * (1.0 - 1e-3), np.sqrt(SMALL_R2) * (1.0 + 1e-3)):
        R, t = axis_pose(r)
        tab = exact_table(6, 6, range(36), cam, R, t)
        if r == 0.0:
            tab["xy"][14, 4:6] = [cam.cx, cam.cy]
        out.append(tab)
    return out


# ---- a rendered frame seen through a fisheye ----------------------------------------------------------------------------------
def fisheye_rays(cam, u, v, steps=60):
    """Pixels of the equidistant camera -> pinhole coordinates (x, y) of their rays: theta from theta_d by Newton run long, then
    np.tan (numpy float64)."""
    fx, fy, cx, cy, k1, k2, k3, k4, _ = [float(c) for c in cam]
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    thd = np.sqrt(x0 * x0 + y0 * y0)
    th = thd.copy()
    for _ in range(steps):
        t2 = th * th
        th = th - (th * (1 + k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4) - thd) / (1 + 3 * k1 * t2 + 5 * k2 * t2 ** 2 + 7 * k3 * t2 ** 3 + 9 * k4 * t2 ** 4)
    k = np.where(thd > 0.0, np.tan(th) / np.where(thd > 0.0, thd, 1.0), 1.0)
    return x0 * k, y0 * k


def warp(img, pinhole, cam):
    """The frame `pinhole` (fx, fy, cx, cy) rendered as the equidistant `cam` would have seen it: every output pixel goes to its
    ray by the inverse model and samples the pinhole frame there, order 1."""
    from scipy.ndimage import map_coordinates
    v, u = np.mgrid[0:img.shape[0], 0:img.shape[1]].astype(np.float64)
    x, y = fisheye_rays(cam, u, v)
    ui, vi = pinhole[0] * x + pinhole[2], pinhole[1] * y + pinhole[3]
    return np.clip(np.rint(map_coordinates(img.astype(np.float64), [vi, ui], order=1, mode="nearest")), 0, 255).astype(np.uint8)


WARP_MISSING = PC.WARP_MISSING  # four tags of the outermost ring
WARP_FOCAL = 0.62  # the fisheye's focal length as a fraction of the rendered pinhole's: see warped_frame


@functools.lru_cache(maxsize=None)
def warped_frame():
    """board_pose_cases.warped_frame's rendered 6 x 6 frame seen through an equidistant lens of the pinhole's principal point and
    WARP_FOCAL of its focal length, with Kalibr-sized coefficients -> (luma, the equidistant camera, the zero-distortion radtan
    camera of the same fx, fy, cx, cy, the oracle's saddle list, the oracle's detect, (w, h, rows, cols))."""
    from oracle import oracle as O
    from tests import board_fit_cases as BC
    img, gt, tags, (w, h, rows, cols) = BC.frame(1)
    K = PC.camera_of(A.board_fit(BC.tag_rows(tags), cols, rows, (w, h))["H"], w, h)
    cam = A.Camera.equidistant(K[0] * WARP_FOCAL, K[1] * WARP_FOCAL, K[2], K[3], -0.013, 0.021, -0.013, 0.0026)
    luma = warp(img, K, cam)
    return luma, cam, A.Camera(*cam[:4]), O.refined_saddle_points(luma), O.detect(luma), (w, h, rows, cols)
