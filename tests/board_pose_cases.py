"""What tests/test_board_pose_cpu.py and tests/test_gpu_board_pose.py share: the cameras, boards and poses, a numpy
float64 statement of the pinhole + radial-tangential projection written independently of csrc/board_pose_math.h, the yardstick
(scipy.optimize.least_squares over a rotation vector and t, started from the ground truth), tables projected through the model
and rounded to binary32, splitmix64 noise, a batch of frames answered by agx_board_pose_tail into sentinel-filled arrays, the
batches the GPU suite launches, the zero-skew pinhole a rendered frame is a view through, and a rendered frame warped through the
barrel model with the recovery restated over the host forms."""
import ctypes as C
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests.board_fit_cases import FILL, TAG, untouched, swap_id, wrapped_ids  # noqa: F401  (one sentinel, one row type, one id wrap)

OK, LOOSE, FEW, SINGULAR, INPUT = _ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE, _ffi.AGX_FIT_FEW, _ffi.AGX_FIT_SINGULAR, _ffi.AGX_FIT_INPUT
INLIER, OUTLIER, OFF_BOARD = _ffi.AGX_FIT_ROW_INLIER, _ffi.AGX_FIT_ROW_OUTLIER, _ffi.AGX_FIT_ROW_OFF_BOARD
MISSING = _ffi.AGX_FIT_PREDICT_MISSING
SIZE = (800, 600)
# fx = fy = 400 on 800 x 600: a horizontal field of view of 90 degrees, the "wide lens" of the header.  At the image's corner
# r = 1.25, where k1 = -0.3, k2 = 0.1 pull a point in by 22 % of its radius.
CAMERAS = {
    "pinhole": A.Camera(400.0, 400.0, 400.0, 300.0),
    "mild": A.Camera(400.0, 410.0, 395.0, 305.0, -0.1, 0.01, 1e-3, -1e-3, 0.0),
    "barrel": A.Camera(400.0, 400.0, 400.0, 300.0, -0.3, 0.1, 0.0, 0.0, 0.0),
    # every term of the model live.  "k3": the radial map r rad(r) stays monotone out to the image's corner, where its slope
    # 1 + 3 k1 r^2 + 5 k2 r^4 + 7 k3 r^6 is 0.28 (a map that folds inside the image, k1 = k2 = 0, k3 = 0.05 for one, is not inverted
    # by the seed's 8 undistortion steps: a test under it measures the seed, not the model); without its k3 the "near" board's corners
    # move by hundreds of pixels, the frontal board's by 6.5 px.  "tangential": p1, p2 twenty times "mild"'s.  "full": anisotropic,
    # off-centre, no coefficient zero.
    "k3": A.Camera(400.0, 400.0, 400.0, 300.0, -0.3, 0.1, 0.0, 0.0, -0.02),
    "tangential": A.Camera(400.0, 400.0, 400.0, 300.0, 0.0, 0.0, 0.02, -0.015, 0.0),
    "full": A.Camera(380.0, 420.0, 410.0, 290.0, -0.25, 0.08, 0.01, -0.008, -0.015),
}
KEYS = ("pose", "err_sq", "row_status", "n_inliers", "rms", "best_iter", "pred", "n_pred", "status")


def board_points(cols, rows, s=0.3, tag_size=1.0):
    """[rows*cols, 4, 3] float64: Kalibr's layout in the plane Z = 0, centred on the board's centre, times tag_size."""
    t = np.arange(rows * cols)
    r, c = t // cols, t % cols
    bw, bh = cols * (1.0 + s) - s, rows * (1.0 + s) - s
    x = (c[:, None] * (1.0 + s) + np.array([0.0, 1.0, 1.0, 0.0]) - bw / 2) * tag_size
    y = (r[:, None] * (1.0 + s) + np.array([0.0, 0.0, 1.0, 1.0]) - bh / 2) * tag_size
    return np.stack([x, y, np.zeros_like(x)], axis=-1)


def project(cam, R, t, P):
    """The model in numpy float64: points P [..., 3] of the board -> pixels [..., 2]; NaN where Z is not > 0."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = [float(v) for v in cam]
    Q = P @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    z = np.where(Q[..., 2] > 0.0, Q[..., 2], np.nan)
    x, y = Q[..., 0] / z, Q[..., 1] / z
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=-1)


def rotation(rx, ry, rz):
    """R = Rz Ry Rx, angles in degrees."""
    a, b, c = np.radians([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


# name -> (rotation angles in degrees, t in units of the board's larger extent).  "near" fills the image to its corners.
POSES = {
    "frontal": ((0.0, 0.0, 3.0), (0.02, -0.01, 0.75)),
    "tilt40": ((40.0, 5.0, -4.0), (0.0, 0.03, 0.8)),
    "tilt60": ((8.0, 60.0, 10.0), (0.05, 0.0, 0.9)),
    "near": ((6.0, -7.0, 1.0), (0.0, 0.0, 0.5)),
    "far": ((-15.0, 12.0, 20.0), (0.6, -0.4, 2.5)),
}
LAYOUTS = ((6, 6), (4, 7))  # cols, rows
TAG_SIZE = 0.05


def extent(cols, rows, s=0.3, tag_size=TAG_SIZE):
    return max(cols * (1.0 + s) - s, rows * (1.0 + s) - s) * tag_size


def pose(name, cols, rows, tag_size=TAG_SIZE, s=0.3):
    ang, t = POSES[name]
    return rotation(*ang), np.asarray(t, np.float64) * extent(cols, rows, s, tag_size)


def layout_index(ids, first_id):
    """The layout's tag under each id: (id - first_id) mod 2^32 in int64 (what the header's wrapping subtraction gives)."""
    return (np.asarray(ids).astype(np.int64) - int(first_id)) & 0xFFFFFFFF


def splitmix64(n, seed):
    """n values in [-1, 1) from the splitmix64 sequence of `seed`."""
    out, x, mask = np.empty(n, np.float64), int(seed) & 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF
    for i in range(n):
        x = (x + 0x9E3779B97F4A7C15) & mask
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        out[i] = (z >> 11) / float(1 << 52) - 1.0
    return out


def exact_table(cols, rows, ids, cam, R, t, tag_size=TAG_SIZE, first_id=0, s=0.3, noise=0.0, seed=1):
    """TAG rows of the layout's tags `ids` (offsets from first_id) projected in float64 through the model, each coordinate moved
    by up to `noise` px (splitmix64), rounded to float32."""
    ids = np.asarray(ids, np.int64)
    uv = project(cam, R, t, board_points(cols, rows, s, tag_size)[ids])
    if noise:
        uv = uv + noise * splitmix64(uv.size, seed).reshape(uv.shape)
    out = np.zeros(len(ids), TAG)
    out["id"] = wrapped_ids(first_id, ids)
    out["xy"] = uv.reshape(len(ids), 8).astype(np.float32)
    return out


def yardstick(table, cols, rows, cam, R0, t0, tag_size=TAG_SIZE, first_id=0, s=0.3):
    """The least-squares pose of the table's rows by scipy, started from (R0, t0) -> (R, t, sum of |e|^2)."""
    from scipy.optimize import least_squares
    P = board_points(cols, rows, s, tag_size)[layout_index(table["id"], first_id)]
    obs = table["xy"].astype(np.float64).reshape(-1, 4, 2)

    def res(p):
        return (project(cam, rodrigues(p[:3]) @ R0, p[3:], P) - obs).ravel()

    sol = least_squares(res, np.concatenate([np.zeros(3), t0]), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return rodrigues(sol.x[:3]) @ R0, sol.x[3:], float(np.sum(res(sol.x) ** 2))


def camera_args(cam):
    return [float(v) for v in (cam if isinstance(cam, A.Camera) else A.Camera(*cam))]


class PoseBatch:
    """Frames that share one call's scalars; board_fit_cases.Batch for agx_board_pose_*."""

    def __init__(self, name, tables, cols, rows, cam, tag_size=TAG_SIZE, first_id=0, s=0.3, max_err_sq=4.0, max_drop=0, min_tags=1, iterations=10,
                 flags=0, counts=None, tag_status=None, tpf=None):
        self.name, self.tables, self.cols, self.rows, self.cam = name, [np.ascontiguousarray(t, TAG) for t in tables], cols, rows, cam
        self.tag_size, self.first_id, self.s, self.max_err_sq, self.max_drop = tag_size, first_id, s, max_err_sq, max_drop
        self.min_tags, self.iterations, self.flags = min_tags, iterations, flags
        self.counts = [len(t) for t in self.tables] if counts is None else list(counts)
        self.tag_status = tag_status
        self.tpf = max([len(t) for t in self.tables] + [1]) if tpf is None else tpf
        self.n = len(self.tables)

    def table(self):
        t = np.full((self.n, self.tpf), 0, TAG)
        t.view(np.uint8)[...] = FILL
        for f, rows in enumerate(self.tables):
            t[f, :len(rows)] = rows
        return t

    def empty_outputs(self):
        """Every output array, one frame of room more than the call is told about, every byte FILL."""
        n, nb = self.n + 1, self.cols * self.rows
        shapes = dict(pose=((n, 12), np.float64), err_sq=((n, self.tpf), np.float32), row_status=((n, self.tpf), np.uint32),
                      n_inliers=((n,), np.uint32), rms=((n,), np.float32), best_iter=((n,), np.uint32), pred=((n, nb), TAG),
                      n_pred=((n,), np.uint32), status=((n,), np.uint32))
        out = {}
        for k, (shape, dt) in shapes.items():
            a = np.zeros(shape, dt)
            a.view(np.uint8)[...] = FILL
            out[k] = a
        return out

    def host(self):
        """agx_board_pose_tail frame by frame into empty_outputs()."""
        out, table = self.empty_outputs(), self.table()
        u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        cam = (C.c_double * 9)(*camera_args(self.cam))
        for f in range(self.n):
            st = _ffi.AGX_TAGS_OK if self.tag_status is None else self.tag_status[f]
            rc = _ffi.lib().agx_board_pose_tail(
                table[f].ctypes.data, self.tpf, self.counts[f], st, self.cols, self.rows, self.first_id, float(self.s), float(self.tag_size), cam,
                float(self.max_err_sq), self.max_drop, self.min_tags, self.iterations, self.flags, out["pose"][f].ctypes.data,
                out["err_sq"][f].ctypes.data, out["row_status"][f].ctypes.data, C.cast(out["n_inliers"][f:].ctypes.data, u32),
                C.cast(out["rms"][f:].ctypes.data, f32), C.cast(out["best_iter"][f:].ctypes.data, u32), out["pred"][f].ctypes.data,
                C.cast(out["n_pred"][f:].ctypes.data, u32), C.cast(out["status"][f:].ctypes.data, u32))
            assert rc == _ffi.AGX_OK, (self.name, f, rc)
        return out


def flat_row(table):
    """One row whose four corners coincide: the seed's system is singular."""
    t = table[:1].copy()
    t["xy"][0] = np.tile(np.float32([100.0, 50.0]), 4)
    return t


def nan_row(table):
    t = table.copy()
    t["xy"][len(t) // 2, 5] = np.nan
    return t


# At iterations = 0 the answer is the seed, whose residuals are not at the noise level: a lone far tag's decomposed homography is
# 117 px off (frame 0 of the 64 x 64 launch), and the seed through 8 undistortion steps under the barrel leaves the 60 degree tilt
# above max_err_sq.  The statuses of those launches as the host form gives them, frame by frame:
SEED_ONLY_STATUS = {
    "64x64_mild_it0_drop0_all": [LOOSE] + [OK] * 8 + [LOOSE, FEW, SINGULAR, INPUT, INPUT, INPUT],
    "6x6_barrel_it0_drop2_missing": [OK, OK, LOOSE, OK, OK, LOOSE, FEW, SINGULAR, INPUT, LOOSE],
}
# The launches under the cameras with every term live and with a wrapping id window (first_id = 0xFFFFFFF0: the 36 ids run
# through 0xFFFFFFFF to 19): the statuses as the host form gives them, pinned.
WRAP_FIRST_ID = 0xFFFFFFF0
LIVE_STATUS = {
    "64x64_full_it10_drop2_missing": [OK] * 9 + [LOOSE, OK, FEW, SINGULAR, INPUT, INPUT, INPUT],
    "6x6_full_it10_drop2_missing": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT, OK],
    "6x6_k3_it10_drop0_all": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT],
    "6x6_full_s1_wrap": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT, OK],
    "6x6_full_s-0.5_wrap": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT, OK],
    "6x6_full_s0_wrap": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT, OK],
}


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """The launches of the GPU parity test: name -> (PoseBatch, the statuses its first frames must have).  The layout, the camera,
    iterations, max_drop, the flag, the spacing ratio and first_id are scalars of a call, so each combination is a launch of its
    own; every launch holds every frame status and tables whose row counts straddle the lane stride."""
    out = {}
    rng = np.random.RandomState(7)
    # 64 x 64, tag_size 0.01: the board spans 0.83; counts 1, 4, 36, 63, 64, 65, 129, 587 of a table of 600 rows
    R, t = pose("tilt40", 64, 64, 0.01)
    ids = rng.permutation(4096)[:587]
    for cam, it, drop, flags in (("barrel", 10, 2, MISSING), ("mild", 0, 0, 0), ("full", 10, 2, MISSING)):
        full = exact_table(64, 64, ids, CAMERAS[cam], R, t, 0.01, first_id=5, noise=0.05)
        off = full[:3].copy()
        off["id"] = [4, 5 + 4096, 0xFFFFFFFF]  # ids around the layout: never fitted
        tables = [full[:n] for n in (1, 4, 36, 63, 64, 65, 129, 587)]
        status = [OK] * 8
        tables.append(np.concatenate([off[:2], full[:40], off[2:]]))
        status.append(OK)
        n_wrong = drop + 1  # one more wrong id than the rounds may drop: AGX_FIT_LOOSE
        tables.append(_wrong(full[:36], n_wrong))
        status.append(LOOSE)
        if drop:
            tables.append(_wrong(full[:70], 1))  # a wrong id that one round drops
            status.append(OK)
        tables += [full[:0], flat_row(full), nan_row(full[:20])]
        status += [FEW, SINGULAR, INPUT]
        counts = [len(x) for x in tables] + [601, 10]
        tables += [full[:10], full[:10]]
        status += [INPUT, INPUT]  # a count above the rows per frame; a table whose status word is not AGX_TAGS_OK
        tag_status = [0] * (len(tables) - 1) + [_ffi.AGX_TAGS_CAPACITY]
        name = "64x64_%s_it%d_drop%d_%s" % (cam, it, drop, "missing" if flags else "all")
        status = LIVE_STATUS.get(name, SEED_ONLY_STATUS.get(name, status))
        out[name] = (PoseBatch(name, tables, 64, 64, CAMERAS[cam], 0.01, first_id=5, max_drop=drop, iterations=it, flags=flags, counts=counts,
                               tag_status=tag_status, tpf=600), status)
    # 6 x 6: the five poses under one camera a launch, a wrong id, and the refusals
    # (the launches after the first four draw from rng after them: the first four stay what they were)
    for cam, it, drop, flags, s, first_id in (("pinhole", 10, 0, MISSING, 0.3, 0), ("mild", 10, 2, 0, 0.3, 0), ("barrel", 0, 2, MISSING, 0.3, 0),
                                              ("barrel", 10, 0, 0, 0.3, 0), ("full", 10, 2, MISSING, 0.3, 0), ("k3", 10, 0, 0, 0.3, 0),
                                              ("full", 10, 1, MISSING, 1.0, WRAP_FIRST_ID), ("full", 10, 1, MISSING, -0.5, WRAP_FIRST_ID),
                                              ("full", 10, 1, MISSING, 0.0, WRAP_FIRST_ID)):
        tables, status = [], []
        for k, p in enumerate(sorted(POSES)):
            R, t = pose(p, 6, 6, s=s)
            full = exact_table(6, 6, range(36), CAMERAS[cam], R, t, first_id=first_id, s=s, noise=0.1, seed=k + 1)
            tables.append(full[rng.permutation(36)[:36 - 5 * k]])
            status.append(OK)
        base = tables[0]
        tables += [_wrong(base, drop + 1), base[:0], flat_row(base), nan_row(base)]
        status += [LOOSE, FEW, SINGULAR, INPUT]
        if drop:
            tables.append(_wrong(base, 1))
            status.append(OK)
        name = "6x6_%s_it%d_drop%d_%s" % (cam, it, drop, "missing" if flags else "all")
        if first_id:
            name = "6x6_%s_s%g_wrap" % (cam, s)
        status = LIVE_STATUS.get(name, SEED_ONLY_STATUS.get(name, status))
        out[name] = (PoseBatch(name, tables, 6, 6, CAMERAS[cam], first_id=first_id, s=s, max_drop=drop, iterations=it, flags=flags, tpf=40), status)
    R, t = pose("tilt40", 1, 1)
    one = exact_table(1, 1, [0], CAMERAS["mild"], R, t, first_id=7)
    out["1x1"] = (PoseBatch("1x1", [one, one[:0], flat_row(one)], 1, 1, CAMERAS["mild"], first_id=7, flags=MISSING, tpf=3), [OK, FEW, SINGULAR])
    return out


def _wrong(table, n):
    """The table with n rows under the ids of n other rows, which leave the table: tags decoded to wrong ids, every id still one
    of the layout's and none twice."""
    t, k = table.copy(), len(table)
    take = [k - 1 - 2 * i for i in range(n)]
    for i, b in enumerate(take):
        t["id"][2 + 2 * i] = table["id"][b]
    return np.delete(t, take)


# ---- the pinhole behind a rendered frame, and a frame seen through the barrel model ------------------------------------------------
def camera_of(H, w, h):
    """A real zero-skew pinhole (fx, fy, cx, cy) under which the homography H (board units -> pixels) is a rigid view of a plane.
    Zhang's two constraints h1' W h2 = 0, h1' W h1 = h2' W h2 on W = K^-T K^-1 are linear in (1/fx^2, 1/fy^2) once the principal
    point is fixed, and a zero-skew camera has four unknowns, so the principal point is free: it is scanned over a 41 x 41 grid
    from -0.5 to 1.5 image sizes and the camera with fx, fy > 0 nearest to square pixels is taken (then the nearest to the centre).
    Under it H is a rigid pose exactly, whatever the grid's step."""
    best = None
    for cy in np.linspace(-0.5 * h, 1.5 * h, 41):
        for cx in np.linspace(-0.5 * w, 1.5 * w, 41):
            Hc = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]]) @ H
            h1, h2 = Hc[:, 0], Hc[:, 1]
            M = np.array([[h1[0] * h2[0], h1[1] * h2[1]], [h1[0] ** 2 - h2[0] ** 2, h1[1] ** 2 - h2[1] ** 2]])
            if abs(np.linalg.det(M)) < 1e-300:
                continue
            a, b = np.linalg.solve(M, [-h1[2] * h2[2], -(h1[2] ** 2 - h2[2] ** 2)])
            if a > 0 and b > 0:
                key = (abs(np.log(a / b)), (cx - w / 2) ** 2 + (cy - h / 2) ** 2)
                if best is None or key < best[0]:
                    best = (key, (a ** -0.5, b ** -0.5, float(cx), float(cy)))
    return None if best is None else best[1]


def undistort_pixels(cam, u, v, steps=50):
    """Distorted pixels -> the pixels of the same rays through the camera without distortion (the fixed-point iteration, run long)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = [float(c) for c in cam]
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(steps):
        r2 = x * x + y * y
        rad = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3
        dx, dy = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) / rad, (y0 - dy) / rad
    return fx * x + cx, fy * y + cy


def warp(img, cam):
    """The frame as `cam` would have seen it: every output pixel samples the pinhole frame where its ray went, order 1."""
    from scipy.ndimage import map_coordinates
    v, u = np.mgrid[0:img.shape[0], 0:img.shape[1]].astype(np.float64)
    ui, vi = undistort_pixels(cam, u, v)
    return np.clip(np.rint(map_coordinates(img.astype(np.float64), [vi, ui], order=1, mode="nearest")), 0, 255).astype(np.uint8)


WARP_K1, WARP_K2 = -0.3, 0.1  # the strong barrel; at -0.1 / 0.01 and -0.2 / 0.05 the counts below are the same 34 against 36
WARP_MISSING = (0, 5, 30, 35)  # four tags of the outermost ring


@functools.lru_cache(maxsize=None)
def warped_frame():
    """The rendered 6 x 6 frame seen through its own pinhole (camera_of its fitted homography: fx 1099, fy 1098, principal point
    (920, -30)) with the strong barrel added -> (luma, camera, the oracle's saddle list, the oracle's detect {id: 4x2},
    (w, h, rows, cols)).  The oracle still detects all 36 tags on it."""
    from oracle import oracle as O
    from tests import board_fit_cases as BC
    img, gt, tags, (w, h, rows, cols) = BC.frame(1)
    K = camera_of(A.board_fit(BC.tag_rows(tags), cols, rows, (w, h))["H"], w, h)
    cam = A.Camera(*K, WARP_K1, WARP_K2)
    luma = warp(img, cam)
    return luma, cam, O.refined_saddle_points(luma), O.detect(luma), (w, h, rows, cols)


FRAME_FIRST_ID = 100


@functools.lru_cache(maxsize=None)
def frame_from_100():
    """The rendered 6 x 6 frame (seed 12, 800 x 600) of a board whose ids run from 100 to 135 -> (luma, the oracle's saddle list,
    the oracle's detect {id: 4x2}, the pinhole camera_of the homography fitted to it)."""
    from oracle import oracle as O
    from aprilgrid_rs_amd import synth
    img, _ = synth.render_frame(12, 800, 600, spec=synth.BoardSpec(rows=6, cols=6, first_id=FRAME_FIRST_ID))
    img = np.ascontiguousarray(img.numpy())
    tags = O.detect(img)
    from tests import board_fit_cases as BC
    K = camera_of(A.board_fit(BC.tag_rows(tags), 6, 6, (800, 600), first_id=FRAME_FIRST_ID)["H"], 800, 600)
    return img, O.refined_saddle_points(img), tags, A.Camera(*K)


def recovered_host(luma, saddles, tags, cols, rows, camera=None, first_id=0, max_dist=3.0, max_err=2.0, max_drop=4, min_tags=2, family="t36h11"):
    """recover_tags_enqueue restated over the host forms for one frame, with board_pose in board_fit's place when a camera is
    given (board_fit_cases.recovered_host is the same without one) -> ({id: 4x2 corners} in row order, the fit's dict)."""
    from tests import board_fit_cases as BC
    saddles = np.ascontiguousarray(saddles, A.SADDLE_DTYPE)
    h, w = luma.shape
    table = BC.tag_rows(tags)
    kw = dict(first_id=first_id, max_err_sq=max_err * max_err, max_drop=max_drop, min_tags=min_tags, predict_missing=True)
    fit = A.board_fit(table, cols, rows, (w, h), **kw) if camera is None else A.board_pose(table, cols, rows, camera, **kw)
    if fit["status"] not in (OK, LOOSE) or not len(fit["pred"]) or not len(saddles):
        return dict(tags), fit
    _slots, _dist, quads, index, sst = A.snap_points(saddles, fit["pred"], max_dist * max_dist, reverse=True)
    if sst != _ffi.AGX_SNAP_OK or not len(quads):
        return dict(tags), fit
    pts = np.stack([saddles["x"][quads], saddles["y"][quads]], axis=-1)
    qtags, qstatus = A.decode_quads_tail(family, luma, pts)
    want = fit["pred"]["id"][index]
    qstatus = np.where((qstatus == _ffi.AGX_QUAD_DECODED) & (qtags["id"] == want), qstatus, _ffi.AGX_QUAD_NO_MATCH).astype(np.uint32)
    room = np.zeros(587, TAG)
    room[:len(table)] = table
    out, n, status, _ = A.collect_tags(family, quads, _ffi.AGX_BOARD_FOUND, qtags, qstatus, len(saddles), None, room, len(table), _ffi.AGX_TAGS_OK, 587)
    assert status == _ffi.AGX_TAGS_OK
    return {int(t["id"]): np.array(t["xy"], np.float32).reshape(4, 2) for t in out[:n]}, fit
