"""What tests/test_calibrate_cpu.py and tests/test_gpu_calibrate.py share: the three cameras, batches of tables projected by the
library's own agx_debug_pose_project from known poses (board_pose_looking_at with distinct tilts), the pose call's answers for
them (agx_board_pose_tail_m per frame), scipy's joint least-squares optimum over the same 9 + 6 n unknowns, and the batches of
the GPU suite."""
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import board_pose_cases as PC
from tests.board_pose_equi_cases import library_project

TAG = A.TagDetector.TAG_DTYPE
OK, FEW, SINGULAR = _ffi.AGX_CALIB_OK, _ffi.AGX_CALIB_FEW, _ffi.AGX_CALIB_SINGULAR
SIZE = (800, 600)
TAG_SIZE = 0.05
COLS = ROWS = 6
S = float(np.float32(0.3))  # the spacing ratio as the library reads it (a binary32)
# the strong-barrel camera of the README's pose row on a 90 degree lens; Kalibr-sized equidistant coefficients; a double sphere of
# the size Usenko et al. report for a 190 degree lens, scaled to the 800 x 600 frame
CAMERAS = {
    "radtan": A.Camera(400.0, 400.0, 400.0, 300.0, -0.3, 0.1, 0.0, 0.0, 0.0),
    "equidistant": A.Camera.equidistant(400.0, 410.0, 395.0, 305.0, -0.013, 0.021, -0.013, 0.0026),
    "double_sphere": A.Camera.double_sphere(250.0, 250.0, 400.0, 300.0, -0.2, 0.55),
}
# the doubles the tests leave free per model (radial-tangential: k3 held -- eight views of a 6 x 6 board do not pin a sixth-order term)
FIXED = {"radtan": 0x100, "equidistant": 0, "double_sphere": 0}
# 8 poses with distinct tilts (degrees), distances in metres (the board is 0.385 m wide) and offsets
POSES = [(0.45, 25.0, 0.0, 0.0, (0.0, 0.0)), (0.5, -20.0, 15.0, 10.0, (0.05, 0.0)), (0.55, 0.0, 30.0, -5.0, (-0.08, 0.03)),
         (0.4, 10.0, -28.0, 20.0, (0.06, -0.05)), (0.6, -32.0, -10.0, 90.0, (0.0, 0.06)), (0.5, 18.0, 22.0, 45.0, (-0.1, -0.04)),
         (0.65, -15.0, -25.0, -30.0, (0.12, 0.05)), (0.42, 35.0, 5.0, 3.0, (-0.03, -0.02))]


def poses(n=8):
    """[n, 12] float64: R row major, then t, of board_pose_looking_at at POSES (cycled, each cycle a little further away)"""
    out = []
    for k in range(n):
        d, tx, ty, rz, off = POSES[k % len(POSES)]
        R, t = A.board_pose_looking_at(d * (1.0 + 0.07 * (k // len(POSES))), tx, ty, rz, off)
        out.append(np.concatenate([R.reshape(9), t]))
    return np.array(out)


def table(cam, pose, ids=None, noise=0.0, seed=1, cols=COLS, rows=ROWS, tag_size=TAG_SIZE):
    """rows of TAG_DTYPE: the layout's tags `ids` projected by agx_debug_pose_project, plus uniform noise of +-`noise` px"""
    ids = np.arange(cols * rows) if ids is None else np.asarray(ids, np.int64)
    P = PC.board_points(cols, rows, S, tag_size)[ids]
    Q = P.reshape(-1, 3) @ pose[:9].reshape(3, 3).T + pose[9:]
    uv = library_project(cam, Q).reshape(len(ids), 8)
    if noise:
        uv = uv + noise * PC.splitmix64(uv.size, seed).reshape(uv.shape)
    out = np.zeros(len(ids), TAG)
    out["id"] = ids
    out["xy"] = uv.astype(np.float32)
    return out


class Batch:
    """Tables of n frames in one array [n, tpf] with their counts, and the pose call's answers under `seed`."""

    def __init__(self, tables, seed, tpf=None, cols=COLS, rows=ROWS, tag_size=TAG_SIZE, pose_iterations=10, max_err_sq=1e12):
        self.n, self.cols, self.rows, self.tag_size, self.seed = len(tables), cols, rows, tag_size, seed
        self.tpf = max([len(t) for t in tables] + [1]) + 3 if tpf is None else tpf  # (tags_per_frame larger than any count)
        self.tags = np.zeros((self.n, self.tpf), TAG)
        self.tags["id"] = 0xFFFFFFFF
        self.counts = np.array([len(t) for t in tables], np.uint32)
        self.pose = np.zeros((self.n, 12), np.float64)
        self.row_status = np.full((self.n, self.tpf), _ffi.AGX_FIT_ROW_OFF_BOARD, np.uint32)
        self.fit_status = np.full(self.n, _ffi.AGX_FIT_FEW, np.uint32)
        for f, t in enumerate(tables):
            self.tags[f, :len(t)] = t
            r = A.board_pose(t, cols, rows, seed, tag_size=tag_size, max_err_sq=max_err_sq, iterations=pose_iterations)
            self.fit_status[f] = r["status"]
            if r["status"] in (_ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE):
                self.pose[f] = r["pose"]
                self.row_status[f, :len(t)] = r["row_status"]

    def subset(self, keep):
        """the batch of the frames `keep`, in that order"""
        b = object.__new__(Batch)
        b.__dict__.update(self.__dict__)
        keep = np.asarray(keep, np.int64)
        b.n = len(keep)
        for k in ("tags", "counts", "pose", "row_status", "fit_status"):
            setattr(b, k, np.ascontiguousarray(getattr(self, k)[keep]))
        return b

    def host(self, camera=None, **kw):
        """agx_calibrate_tail on the batch -> calibrate's dict with the raw output arrays"""
        return A.calibrate(self.tags, self.counts, self.cols, self.rows, self.seed if camera is None else camera, self.pose, self.row_status,
                           self.fit_status, tag_size=self.tag_size, raw=True, **kw)

    def residuals(self, cam, pose):
        """the pixel residuals of the inlier rows of the usable frames under (cam, pose [n, 12]), by agx_debug_pose_project"""
        out = []
        for f in range(self.n):
            if self.fit_status[f] != _ffi.AGX_FIT_OK:
                continue
            t = self.tags[f, :self.counts[f]][self.row_status[f, :self.counts[f]] == _ffi.AGX_FIT_ROW_INLIER]
            P = PC.board_points(self.cols, self.rows, S, self.tag_size)[t["id"].astype(np.int64)]
            Q = P.reshape(-1, 3) @ pose[f, :9].reshape(3, 3).T + pose[f, 9:]
            out.append((library_project(cam, Q) - t["xy"].astype(np.float64).reshape(-1, 2)).ravel())
        return np.concatenate(out)


def make_camera(like, nine):
    return type(like)(*[float(v) for v in nine])


def off_seed(cam):
    """the exact-data tests' seed: focal lengths 5 % off, the principal point 10 px off, the distortion at zero (a double sphere
    keeps a xi and an alpha inside the domain: xi = 0, alpha = 0.5)"""
    nine = [cam[0] * 1.05, cam[1] * 0.95, cam[2] + 10.0, cam[3] - 10.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    if cam.model == _ffi.AGX_LENS_DOUBLE_SPHERE:
        nine[4], nine[5] = 0.0, 0.5
    return make_camera(cam, nine)


def scipy_joint(batch, cam0, pose0, fixed_mask):
    """scipy's least-squares optimum over the free camera doubles and the 6 unknowns of every usable frame, from (cam0, pose0):
    -> (camera nine, pose [n, 12], sum of |e|^2).  The model is the library's projection (agx_debug_pose_project)."""
    from scipy.optimize import least_squares
    free = [i for i in range(9) if not (fixed_mask >> i) & 1]
    use = [f for f in range(batch.n) if batch.fit_status[f] == _ffi.AGX_FIT_OK]
    c0 = np.array([float(v) for v in cam0])

    def unpack(p):
        c = c0.copy()
        c[free] = p[:len(free)]
        pose = pose0.copy()
        for k, f in enumerate(use):
            q = p[len(free) + 6 * k:len(free) + 6 * k + 6]
            pose[f, :9] = (pose0[f, :9].reshape(3, 3) @ PC.rodrigues(q[:3])).reshape(9)
            pose[f, 9:] = pose0[f, 9:] + q[3:]
        return c, pose

    def res(p):
        c, pose = unpack(p)
        try:
            return batch.residuals(make_camera(cam0, c), pose)
        except AssertionError:  # the camera left the model's domain
            return np.full(n_res, 1e6)

    p0 = np.concatenate([c0[free], np.zeros(6 * len(use))])
    n_res = len(batch.residuals(cam0, pose0))
    sol = least_squares(res, p0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000, x_scale="jac")
    c, pose = unpack(sol.x)
    return c, pose, float(np.sum(res(sol.x) ** 2))


@functools.lru_cache(maxsize=None)
def exact_batch(lens, noise=0.0, n=8):
    """8 full 6 x 6 tables from CAMERAS[lens] at POSES, posed under off_seed"""
    cam = CAMERAS[lens]
    return Batch([table(cam, p, noise=noise, seed=k + 1) for k, p in enumerate(poses(n))], off_seed(cam))


# ---- the numerical cases (found on the CPU): seeds under which the steps leave the model's domain or the cost rises ----------------
# the first step from here takes alpha above 1: iterate 1's cost is +inf, the answer is iterate 0
DS_ALPHA_LEAVES = A.Camera.double_sphere(325.0, 325.0, 410.0, 290.0, 0.3, 0.97)
# undamped steps from here raise the cost three times and then leave the domain
DS_DIVERGES = A.Camera.double_sphere(262.5, 262.5, 410.0, 290.0, -0.1, 0.5)
# a poor radial-tangential seed: the cost rises at iterates 1, 2 and 5 and then falls to the noise floor
RT_RISES = A.Camera(200.0, 700.0, 400.0, 300.0, 0.8, 0.8, 0.0, 0.0, 0.0)


def fronto_batch(n=4):
    """n frames fronto-parallel at one distance (distinct rolls and offsets): fx and fy against the distance are not determined"""
    cam = A.Camera(400.0, 400.0, 400.0, 300.0)  # (a pinhole: under distortion the distance shows in the radial term)
    ps = []
    for k in range(n):
        R, t = A.board_pose_looking_at(0.5, 0.0, 0.0, 17.0 * k, (0.03 * k, -0.02 * k))
        ps.append(np.concatenate([R.reshape(9), t]))
    return Batch([table(cam, p) for p in ps], cam)


def few_batch():
    """3 frames of one tag each: 12 corners, fewer than the 8 free doubles and 18 pose unknowns"""
    cam = CAMERAS["radtan"]
    return Batch([table(cam, p, ids=[14 + k]) for k, p in enumerate(poses(3))], cam)


def host_rounds(tables, cols, rows, size, tag_size=TAG_SIZE, fixed=0, rounds=3, iterations=10, lens="radtan", cap=None, tag_status=None, damping=None):
    """TagDetector.calibrate_batch's stages by the host forms on host tables (a list of rows of TAG_DTYPE) -> (Camera, pose, report)"""
    n, cap = len(tables), cols * rows if cap is None else cap
    tst = [0] * n if tag_status is None else tag_status
    fits = [A.board_fit(t, cols, rows, size, tag_status=int(tst[f]), tags_per_frame=cap) for f, t in enumerate(tables)]
    hs = np.array([r["H"].reshape(9) if "H" in r else np.zeros(9) for r in fits])
    seed = A.calibrate_seed(hs, [r["status"] for r in fits], size)
    assert seed["status"] == OK, seed
    from aprilgrid_rs_amd.detector import _lens_seed, _seed_damping
    camera = _lens_seed(lens, seed["camera"])
    damping = _seed_damping(camera, damping)
    tags = np.zeros((n, cap), TAG)
    for f, t in enumerate(tables):
        tags[f, :len(t)] = t
    pose, rep, first = np.zeros((n, 12)), None, None
    rst, fst = np.zeros((n, cap), np.uint32), np.zeros(n, np.uint32)
    for _ in range(rounds):
        for f, t in enumerate(tables):
            r = A.board_pose(t, cols, rows, camera, tag_size=tag_size, tag_status=int(tst[f]), tags_per_frame=cap)
            fst[f] = r["status"]
            if "pose" in r:
                pose[f] = r["pose"]
                rst[f, :len(t)] = r["row_status"]
        rep = A.calibrate(tags, [len(t) for t in tables], cols, rows, camera, pose, rst, fst, tag_size=tag_size, fixed=fixed, iterations=iterations,
                          damping=damping, accept_loose=True, tag_status=tst)
        first = float(np.sqrt(rep["cost"][0] / max(rep["n_corners"], 1))) if first is None else first
        rep["first_rms"] = first  # the RMS under the seed camera's poses, before any calibration step
        if rep["status"] != OK:
            break
        camera, pose = rep["camera"], rep["pose"].copy()
    return camera, pose, rep


def host_calibrate_batch(det, frames, cols, rows, size, **kw):
    """calibrate_batch's answer by the host forms on the tables the device detected (fetched here, for the comparison only)"""
    import torch
    n, cap = int(frames.shape[0]), cols * rows
    tags, counts, status = (torch.zeros((n, cap, 9), dtype=torch.int32, device=frames.device), torch.zeros(n, dtype=torch.int32, device=frames.device),
                            torch.zeros(n, dtype=torch.int32, device=frames.device))
    det.detect_batch_enqueue(frames, cap, out=(tags, counts, status))
    det.detect_batch_fetch(raise_on_overflow=False)
    t, c = tags.cpu().numpy().view(TAG).reshape(n, cap), counts.cpu().numpy()
    return host_rounds([t[f, :c[f]] for f in range(n)], cols, rows, size, cap=cap, tag_status=status.cpu().numpy().astype(np.uint32), **kw)


# |fx - the rendering camera's| of test_gpu_calibrate's rendered case.  Measured on the CPU with the host forms alone -- render_boards
# (the host form of the same renderer), the oracle's detect on those frames, host_rounds: fx = 299.7816 against 300, 0.2184 off (on
# the exact tables of the case, render_case_exact_error(), 2.4e-6: the rest is the detector's corner error).  3 x the measurement:
FX_MARGIN = 0.66


def render_case():
    cam = A.Camera(300.0, 300.0, 159.5, 119.5, -0.2, 0.05, 0.0, 0.0, 0.0)
    ps = poses(6)
    ps[:, 9:11] *= 0.3
    ps[:, 11] *= 0.45
    return cam, ps


def render_case_exact_error():
    cam, ps = render_case()
    got, _, rep = host_rounds([table(cam, p, cols=4, rows=4) for p in ps], 4, 4, (320, 240), fixed=0x1c0)
    return abs(got.fx - cam.fx), rep
