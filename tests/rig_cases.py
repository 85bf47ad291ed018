"""What tests/test_rig_cpu.py, tests/test_rig_py_cpu.py and tests/test_gpu_rig.py share: rigs of the three cameras of
tests/calibrate_cases.py looking at one board at synchronised instants (tables by CC.table from E_c o T_s, the pose call's
answers per frame), a numpy restatement of the model (its own projection of the three lens models, the Cayley update) and scipy's
joint least-squares optimum over every E_c, c >= 1, and every T_s."""
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import calibrate_cases as CC

TAG = CC.TAG
OK, FEW, SINGULAR = _ffi.AGX_RIG_OK, _ffi.AGX_RIG_FEW, _ffi.AGX_RIG_SINGULAR
LENSES = ("radtan", "equidistant", "double_sphere")
IDENT = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])


def rot(axis, deg):
    a = np.zeros(3)
    a[axis] = np.radians(deg)
    from tests.board_pose_cases import rodrigues
    return rodrigues(a)


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)])


def compose(a, b):
    """a o b of two poses as 12 numbers: first b, then a"""
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    return pose12(Ra @ Rb, Ra @ b[9:] + a[9:])


def inverse(a):
    R = a[:9].reshape(3, 3)
    return pose12(R.T, -R.T @ a[9:])


def cayley(w):
    a = np.asarray(w, np.float64) / 2.0
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.linalg.solve(np.eye(3) - K, np.eye(3) + K)


def update(p, d):
    """the library's update of a pose by six unknowns: R <- R C(w), t <- t + dt"""
    return pose12(p[:9].reshape(3, 3) @ cayley(d[:3]), p[9:] + d[3:])


def project(cam, Q):
    """numpy's own projection of camera-frame points Q [n, 3] under a Camera of any of the three models -> [n, 2]"""
    c = [float(v) for v in cam]
    fx, fy, cx, cy = c[:4]
    X, Y, Z = Q[:, 0], Q[:, 1], Q[:, 2]
    if cam.model == _ffi.AGX_LENS_DOUBLE_SPHERE:
        xi, al = c[4], c[5]
        d1 = np.sqrt(X * X + Y * Y + Z * Z)
        k = xi * d1 + Z
        d2 = np.sqrt(X * X + Y * Y + k * k)
        den = al * d2 + (1.0 - al) * k
        return np.column_stack([fx * X / den + cx, fy * Y / den + cy])
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    if cam.model == _ffi.AGX_LENS_EQUIDISTANT:
        r = np.sqrt(r2)
        th = np.arctan(r)
        s = np.where(r > 1e-9, th / np.where(r > 1e-9, r, 1.0), 1.0) * (1.0 + c[4] * th ** 2 + c[5] * th ** 4 + c[6] * th ** 6 + c[7] * th ** 8)
        return np.column_stack([fx * s * x + cx, fy * s * y + cy])
    k1, k2, p1, p2, k3 = c[4:9]
    rad = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.column_stack([fx * xd + cx, fy * yd + cy])


def project_board(cam, E, T, XY):
    """board points XY [n, 2] (Z = 0) through T (rig from board), E (camera from rig) and the camera"""
    P = compose(E, T)
    Q = np.column_stack([XY, np.zeros(len(XY))]) @ P[:9].reshape(3, 3).T + P[9:]
    return project(cam, Q)


# the rigs' true extrinsics: camera 1 a 0.1-unit baseline to the right and 5 degrees of toe-in, camera 2 up and rolled, ...
def true_extrinsics(n_cams):
    out = [IDENT.copy()]
    for c in range(1, n_cams):
        R = rot(1, 5.0 * (1 if c % 2 else -1)) @ rot(0, -3.0 * (c // 2)) @ rot(2, 2.0 * c)
        out.append(pose12(R, [-0.1 * c if c % 2 else 0.05 * c, 0.02 * (c // 2), 0.01 * c]))
    return np.array(out)


def off_extrinsics(E, deg=2.0, frac=0.05):
    """the exact-data tests' seed: every E_c, c >= 1, turned by `deg` degrees and moved by `frac` of its baseline"""
    out = E.copy()
    for c in range(1, len(E)):
        R = E[c, :9].reshape(3, 3) @ rot(c % 3, deg)
        b = np.linalg.norm(E[c, 9:])
        out[c] = pose12(R, E[c, 9:] + frac * b * np.array([0.6, -0.64, 0.48]))
    return out


class Rig:
    """Tables of C cameras x S instants [C, S, tpf] with their counts and the pose call's answers under `cams`."""

    def __init__(self, cams, E, T, noise=0.0, ids=None, tpf=None, cols=CC.COLS, rows=CC.ROWS, tag_size=CC.TAG_SIZE, missing=()):
        self.cams, self.E, self.T = list(cams), np.asarray(E, np.float64), np.asarray(T, np.float64)
        self.nc, self.ns, self.cols, self.rows, self.tag_size = len(cams), len(T), cols, rows, tag_size
        n_ids = cols * rows if ids is None else max(len(i) for i in ids) if isinstance(ids, dict) else len(ids)
        self.tpf = n_ids + 3 if tpf is None else tpf
        self.tags = np.zeros((self.nc, self.ns, self.tpf), TAG)
        self.tags["id"] = 0xFFFFFFFF
        self.counts = np.zeros((self.nc, self.ns), np.uint32)
        self.pose = np.zeros((self.nc, self.ns, 12))
        self.row_status = np.full((self.nc, self.ns, self.tpf), _ffi.AGX_FIT_ROW_OFF_BOARD, np.uint32)
        self.fit_status = np.full((self.nc, self.ns), _ffi.AGX_FIT_FEW, np.uint32)
        for c in range(self.nc):
            for s in range(self.ns):
                if (c, s) in missing:
                    continue
                use = ids.get((c, s), ids.get(None)) if isinstance(ids, dict) else ids
                t = CC.table(self.cams[c], compose(self.E[c], self.T[s]), ids=use, noise=noise, seed=1 + c * self.ns + s, cols=cols, rows=rows,
                             tag_size=tag_size)
                self.tags[c, s, :len(t)] = t
                self.counts[c, s] = len(t)
                r = A.board_pose(t, cols, rows, self.cams[c], tag_size=tag_size, max_err_sq=1e12, iterations=10)
                self.fit_status[c, s] = r["status"]
                if r["status"] in (_ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE):
                    self.pose[c, s] = r["pose"]
                    self.row_status[c, s, :len(t)] = r["row_status"]

    def subset(self, cams=None, instants=None):
        b = object.__new__(Rig)
        b.__dict__.update(self.__dict__)
        cs = np.arange(self.nc) if cams is None else np.asarray(cams, np.int64)
        ss = np.arange(self.ns) if instants is None else np.asarray(instants, np.int64)
        b.nc, b.ns = len(cs), len(ss)
        b.cams, b.E, b.T = [self.cams[c] for c in cs], self.E[cs], self.T[ss]
        for k in ("tags", "counts", "pose", "row_status", "fit_status"):
            setattr(b, k, np.ascontiguousarray(getattr(self, k)[cs][:, ss]))
        return b

    def host(self, seed, **kw):
        """agx_rig_calibrate_tail on the rig -> rig_calibrate's dict with the raw output arrays"""
        return A.rig_calibrate(self.tags, self.counts, self.cols, self.rows, self.cams, self.pose, self.row_status, self.fit_status, seed,
                               tag_size=self.tag_size, raw=True, **kw)

    def frames(self, min_cams=2):
        """the counted frames (c, s) under the defaults: AGX_FIT_OK frames of instants with min_cams of them"""
        ok = self.fit_status == _ffi.AGX_FIT_OK
        inst = ok.sum(axis=0) >= min_cams
        return [(c, s) for c in range(self.nc) for s in range(self.ns) if ok[c, s] and inst[s]]

    def residuals(self, E, T, min_cams=2):
        """the pixel residuals of the inlier rows of the counted frames under (E [C, 12], T [S, 12]) by numpy's own projection"""
        from tests.board_pose_cases import board_points
        B = board_points(self.cols, self.rows, CC.S, self.tag_size)
        out = []
        for c, s in self.frames(min_cams):
            n = self.counts[c, s]
            t = self.tags[c, s, :n][self.row_status[c, s, :n] == _ffi.AGX_FIT_ROW_INLIER]
            XY = B[t["id"].astype(np.int64)].reshape(-1, 3)[:, :2]
            out.append((project_board(self.cams[c], E[c], T[s], XY) - t["xy"].astype(np.float64).reshape(-1, 2)).ravel())
        return np.concatenate(out)

    def seed_poses(self, seed, min_cams=2):
        """T_s's seed as the library makes it: E_c^-1 o pose[c, s] of the lowest usable camera (NaN rows: an unusable instant)"""
        T = np.full((self.ns, 12), np.nan)
        ok = self.fit_status == _ffi.AGX_FIT_OK
        for s in range(self.ns):
            if ok[:, s].sum() >= min_cams:
                c = int(np.argmax(ok[:, s]))
                T[s] = self.pose[c, s] if c == 0 else compose(inverse(seed[c]), self.pose[c, s])
        return T


def scipy_joint(rig, E0, T0, min_cams=2):
    """scipy's optimum over all E_c (c >= 1, the counted cameras) and T_s from (E0, T0) -> (E, T, sum of |e|^2)"""
    from scipy.optimize import least_squares
    fr = rig.frames(min_cams)
    cams = sorted({c for c, _ in fr if c >= 1})
    inst = sorted({s for _, s in fr})

    def unpack(p):
        E, T = E0.copy(), T0.copy()
        for k, c in enumerate(cams):
            E[c] = update(E0[c], p[6 * k:6 * k + 6])
        for k, s in enumerate(inst):
            T[s] = update(T0[s], p[6 * (len(cams) + k):6 * (len(cams) + k) + 6])
        return E, T

    res = lambda p: rig.residuals(*unpack(p), min_cams=min_cams)
    sol = least_squares(res, np.zeros(6 * (len(cams) + len(inst))), method="lm", xtol=1e-12, ftol=1e-12, gtol=1e-12, max_nfev=20000)
    E, T = unpack(sol.x)
    return E, T, float(np.sum(res(sol.x) ** 2))


def ext_distance(a, b):
    """the distance of two extrinsics: the rotation between them (radians) plus the distance of their translations"""
    R = a[:9].reshape(3, 3).T @ b[:9].reshape(3, 3)
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)) + np.linalg.norm(a[9:] - b[9:]))


def three_cameras():
    return [CC.CAMERAS[k] for k in LENSES]


@functools.lru_cache(maxsize=None)
def three_rig(noise=0.0, n=8):
    """3 cameras (radtan, equidistant, double sphere) x n instants of full 6 x 6 tables"""
    return Rig(three_cameras(), true_extrinsics(3), CC.poses(n), noise=noise)


@functools.lru_cache(maxsize=None)
def stereo_rig(noise=0.0, n=8, lens="radtan", tpf=None, ids=None):
    return Rig([CC.CAMERAS[lens]] * 2, true_extrinsics(2), CC.poses(n), noise=noise, tpf=tpf, ids=ids)


# the numerical cases (found on the CPU) on stereo_rig(noise=0.1): from a seed 60 degrees and 5 baselines off the undamped steps lower
# the cost once and then put a corner behind the camera (+inf: the answer is iterate 1 of 2); at damping 1e-3 every later iterate's
# cost is finite and far above iterate 0's (the answer is the inputs after 12 iterates)
RISES_SEED = dict(deg=60.0, frac=5.0)
RISES_THEN_LEAVES = dict(damping=0.0)
RISES_FINITE = dict(damping=1e-3)


# |baseline - 0.03| of test_gpu_rig's rendered case.  Measured on the CPU with the host forms alone -- render_boards (the host form
# of the same renderer) of render_case(), the oracle's detect on those frames (4, 6, 8, 0, 2, 5, 6 and 3 tags of the 16: the tags
# are small at 320 x 240), host_rig_rounds: a baseline of 0.0299363 against 0.03, 6.4e-5 off, 3 instants used, RMS 0.053 px.
# Twice the measurement:
BASELINE_MARGIN = 1.3e-4


def render_case():
    """2 cameras x 4 instants of a 4 x 4 board at 320 x 240: the camera, E [2, 12], T [4, 12]"""
    cam = A.Camera(300.0, 300.0, 159.5, 119.5, -0.2, 0.05, 0.0, 0.0, 0.0)
    T = CC.poses(4)
    T[:, 9:11] *= 0.25
    T[:, 11] *= 0.45
    E = np.array([IDENT, pose12(rot(1, 3.0), [-0.03, 0.0, 0.0])])
    return cam, E, T


def host_rig_rounds(tables, n_cams, n_instants, cols, rows, cameras, tag_size=CC.TAG_SIZE, rounds=2, iterations=10, cap=None, tag_status=None):
    """TagDetector.rig_calibrate_batch's stages by the host forms on host tables (a list of C * S row arrays, frame f = c S + s)
    -> (extrinsics, rig_pose, report)"""
    n, cap = n_cams * n_instants, cols * rows if cap is None else cap
    tst = np.zeros(n, np.uint32) if tag_status is None else np.asarray(tag_status, np.uint32)
    tags = np.zeros((n, cap), TAG)
    pose, rst, fst, n_inl = np.zeros((n, 12)), np.zeros((n, cap), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for f, t in enumerate(tables):
        tags[f, :len(t)] = t
        r = A.board_pose(t, cols, rows, cameras[f // n_instants], tag_size=tag_size, tag_status=int(tst[f]), tags_per_frame=cap)
        fst[f] = r["status"]
        if "pose" in r:
            pose[f], n_inl[f] = r["pose"], r["n_inliers"]
            rst[f, :len(t)] = r["row_status"]
    shape = (n_cams, n_instants)
    ext = A.rig_seed(pose.reshape(shape + (12,)), fst.reshape(shape), n_inl.reshape(shape))["extrinsics"]
    rep = None
    for _ in range(rounds):
        rep = A.rig_calibrate(tags.reshape(shape + (cap,)), np.array([len(t) for t in tables]).reshape(shape), cols, rows, cameras, pose, rst, fst, ext,
                              tag_size=tag_size, iterations=iterations, accept_loose=True, tag_status=tst)
        if rep["status"] != OK:
            break
        ext = rep["extrinsics"]
    return ext, rep.get("rig_pose"), rep


def host_rig_batch(det, frames, cols, rows, cameras, **kw):
    """rig_calibrate_batch's answer by the host forms on the tables the device detected (fetched here, for the comparison only)"""
    import torch
    nc, ns, cap = int(frames.shape[0]), int(frames.shape[1]), cols * rows
    n = nc * ns
    tags, counts, status = (torch.zeros((n, cap, 9), dtype=torch.int32, device=frames.device), torch.zeros(n, dtype=torch.int32, device=frames.device),
                            torch.zeros(n, dtype=torch.int32, device=frames.device))
    det.detect_batch_enqueue(frames.reshape(n, int(frames.shape[2]), int(frames.shape[3])), cap, out=(tags, counts, status))
    det.detect_batch_fetch(raise_on_overflow=False)
    t, c = tags.cpu().numpy().view(TAG).reshape(n, cap), counts.cpu().numpy()
    return host_rig_rounds([t[f, :c[f]] for f in range(n)], nc, ns, cols, rows, cameras, cap=cap, tag_status=status.cpu().numpy().astype(np.uint32), **kw)
