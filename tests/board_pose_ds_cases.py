"""What the double-sphere tests share (tests/test_board_pose_ds_cpu.py, tests/test_gpu_board_pose_ds.py, tests/test_rectify_ds_cpu.py,
tests/test_gpu_rectify_ds.py): the four (xi, alpha) cameras, a numpy float64 restatement of the double-sphere projection, its valid
cone and its unprojection (Usenko, Demmel, Cremers 2018) written independently of csrc/board_pose_math.h, tables and the scipy
yardstick through it, the launches of the GPU suite (board_pose_cases's construction under the four cameras) and the launch whose
tables hold the corners only this model has: on the principal point, behind the image plane, clamped by the seed, outside the
unprojection's domain."""
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import board_pose_cases as PC
from tests import board_pose_equi_cases as EC
from tests.board_pose_cases import FEW, INPUT, LOOSE, MISSING, OK, SINGULAR, TAG, TAG_SIZE

DS = 2  # AGX_LENS_DOUBLE_SPHERE, as the issue fixes it
THETA_MAX = 1.5
# 800 x 600 as board_pose_cases; fx is 400 (1 + xi), so that the image near the axis is the 400 px pinhole's under every camera.
# "pinhole": (xi, alpha) = (0, 0), the model's pinhole limit.  "neg": a negative xi with alpha > 0.5.  "mid": Kalibr-sized numbers
# of a 190 degree lens.  "high": alpha = 0.8, the unprojection is defined for r2 <= 1 / (2 alpha - 1) = 1.67 only.
XI_ALPHA = {"pinhole": (0.0, 0.0), "neg": (-0.2, 0.59), "mid": (0.6, 0.45), "high": (0.1, 0.8)}


def camera(xi, alpha, fx=None, fy=None, cx=400.0, cy=300.0):
    fx = 400.0 * (1.0 + xi) if fx is None else fx
    return A.Camera.double_sphere(fx, fx if fy is None else fy, cx, cy, xi, alpha)


CAMERAS = {
    "pinhole": camera(0.0, 0.0),
    "neg": camera(-0.2, 0.59, 320.0, 328.0, 395.0, 305.0),
    "mid": camera(0.6, 0.45, 640.0, 650.0, 410.0, 290.0),
    "high": camera(0.1, 0.8, 440.0, 430.0, 402.0, 297.0),
}
WIDE = camera(-0.2, 0.59, 240.0, 240.0)  # fx = 0.3 of the width


def cone(cam):
    """w2 of the validity rule Z > -w2 d1."""
    xi, al = float(cam[4]), float(cam[5])
    w1 = al / (1.0 - al) if al <= 0.5 else (1.0 - al) / al
    return (w1 + xi) / np.sqrt(2.0 * w1 * xi + xi * xi + 1.0)


def cone_angle(cam):
    """The half angle of the valid cone, radians off the optical axis."""
    return float(np.arccos(-cone(cam)))


def valid(cam, Q):
    Q = np.asarray(Q, np.float64)
    d1 = np.sqrt((Q ** 2).sum(axis=-1))
    return (d1 > 0.0) & (Q[..., 2] > -cone(cam) * d1)


def project_rays(cam, Q):
    """Camera-frame points Q [..., 3] -> pixels under the double-sphere model; NaN outside the valid cone and at the origin."""
    fx, fy, cx, cy, xi, al = [float(v) for v in cam[:6]]
    Q = np.asarray(Q, np.float64)
    X, Y, Z = Q[..., 0], Q[..., 1], Q[..., 2]
    d1 = np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    k = xi * d1 + Z
    d2 = np.sqrt(X ** 2 + Y ** 2 + k ** 2)
    den = al * d2 + (1.0 - al) * k
    with np.errstate(invalid="ignore", divide="ignore"):
        uv = np.stack([fx * X / den + cx, fy * Y / den + cy], axis=-1)
    return np.where(valid(cam, Q)[..., None], uv, np.nan)


def project(cam, R, t, P):
    """Points P [..., 3] of the board -> pixels under cam.model (any of the three)."""
    if getattr(cam, "model", EC.RADTAN) != DS:
        return EC.project(cam, R, t, P)
    return project_rays(cam, P @ np.asarray(R, np.float64).T + np.asarray(t, np.float64))


def in_domain(cam, u, v):
    """Is the pixel inside the unprojection's domain: alpha <= 0.5, or r2 <= 1 / (2 alpha - 1)."""
    fx, fy, cx, cy, xi, al = [float(c) for c in cam[:6]]
    r2 = ((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2
    return (r2 <= 1.0 / (2.0 * al - 1.0)) if al > 0.5 else np.ones_like(r2, bool)


def unproject(cam, u, v):
    """Pixels -> rays [..., 3] (not normalised to a pinhole), NaN outside the domain."""
    fx, fy, cx, cy, xi, al = [float(c) for c in cam[:6]]
    mx, my = (u - cx) / fx, (v - cy) / fy
    r2 = mx ** 2 + my ** 2
    with np.errstate(invalid="ignore"):
        mz = (1.0 - al ** 2 * r2) / (al * np.sqrt(1.0 - (2.0 * al - 1.0) * r2) + 1.0 - al)
        s = (mz * xi + np.sqrt(mz ** 2 + (1.0 - xi ** 2) * r2)) / (mz ** 2 + r2)
    return np.stack([s * mx, s * my, s * mz - xi], axis=-1)


def exact_table(cols, rows, ids, cam, R, t, tag_size=TAG_SIZE, first_id=0, s=0.3, noise=0.0, seed=1):
    """board_pose_cases.exact_table through `project`."""
    ids = np.asarray(ids, np.int64)
    uv = project(cam, R, t, PC.board_points(cols, rows, s, tag_size)[ids])
    assert np.isfinite(uv).all()
    if noise:
        uv = uv + noise * PC.splitmix64(uv.size, seed).reshape(uv.shape)
    out = np.zeros(len(ids), TAG)
    out["id"] = PC.wrapped_ids(first_id, ids)
    out["xy"] = uv.reshape(len(ids), 8).astype(np.float32)
    return out


def yardstick(table, cols, rows, cam, R0, t0, tag_size=TAG_SIZE, first_id=0, s=0.3):
    """scipy's least-squares pose through `project`, started from (R0, t0) -> (R, t, sum of |e|^2)."""
    from scipy.optimize import least_squares
    P = PC.board_points(cols, rows, s, tag_size)[PC.layout_index(table["id"], first_id)]
    obs = table["xy"].astype(np.float64).reshape(-1, 4, 2)

    def res(p):
        return (project(cam, PC.rodrigues(p[:3]) @ R0, p[3:], P) - obs).ravel()

    sol = least_squares(res, np.concatenate([np.zeros(3), t0]), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return PC.rodrigues(sol.x[:3]) @ R0, sol.x[3:], float(np.sum(res(sol.x) ** 2))


Batch = EC.EquiBatch  # answered by agx_board_pose_tail_m under the camera's model

# ---- a board that reaches behind the image plane ---------------------------------------------------------------------------------
# A 6 x 6 board 0.2 of its extent ahead of the lens, turned by 35 degrees about Y: the columns on its far side have Zc < 0.
BEHIND = ((3.0, 35.0, 2.0), (0.05, 0.0, 0.2))
BEHIND_MISSING = (5, 23, 35)  # tags of the far column, their corners at Zc < 0: taken out of the GPU launch's table and predicted


def behind_pose():
    return EC.pose_of(BEHIND, 6, 6)


def camera_points(R, t, cols=6, rows=6, tag_size=TAG_SIZE):
    return PC.board_points(cols, rows, tag_size=tag_size) @ np.asarray(R).T + np.asarray(t)


# ---- the GPU suite's launches -----------------------------------------------------------------------------------------------------
# the statuses that are not the construction's nominal ones, as the host form gives them, pinned (at iterations = 0 the answer is the seed)
PINNED_STATUS = {
    "6x6_pinhole_it0_drop2_missing": [OK] * 5 + [LOOSE, FEW, SINGULAR, INPUT, LOOSE],
}


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """board_pose_cases.gpu_batches' construction under the four double-sphere cameras: name -> (Batch, the statuses of its frames)."""
    out = {}
    rng = np.random.RandomState(7)
    R, t = PC.pose("tilt40", 64, 64, 0.01)
    ids = rng.permutation(4096)[:587]
    cam, it, drop, flags = "mid", 10, 2, MISSING  # 64 x 64 once
    full = exact_table(64, 64, ids, CAMERAS[cam], R, t, 0.01, first_id=5, noise=0.05)
    off = full[:3].copy()
    off["id"] = [4, 5 + 4096, 0xFFFFFFFF]
    tables = [full[:n] for n in (1, 4, 36, 63, 64, 65, 129, 587)]
    status = [OK] * 8
    tables.append(np.concatenate([off[:2], full[:40], off[2:]]))
    status.append(OK)
    tables.append(PC._wrong(full[:36], drop + 1))
    status.append(LOOSE)
    tables.append(PC._wrong(full[:70], 1))
    status.append(OK)
    tables += [full[:0], PC.flat_row(full), PC.nan_row(full[:20])]
    status += [FEW, SINGULAR, INPUT]
    counts = [len(x) for x in tables] + [601, 10]
    tables += [full[:10], full[:10]]
    status += [INPUT, INPUT]
    tag_status = [0] * (len(tables) - 1) + [_ffi.AGX_TAGS_CAPACITY]
    name = "64x64_%s_it%d_drop%d_missing" % (cam, it, drop)
    out[name] = (Batch(name, tables, 64, 64, CAMERAS[cam], 0.01, first_id=5, max_drop=drop, iterations=it, flags=flags, counts=counts,
                       tag_status=tag_status, tpf=600), PINNED_STATUS.get(name, status))
    for cam, it, drop, flags in (("pinhole", 10, 0, MISSING), ("pinhole", 0, 2, MISSING), ("neg", 10, 2, 0), ("neg", 5, 0, MISSING),
                                 ("mid", 10, 2, MISSING), ("mid", 0, 0, 0), ("high", 10, 0, 0), ("high", 5, 2, MISSING)):
        tables, status = [], []
        poses = [PC.POSES[p] for p in sorted(PC.POSES)] + ([EC.VNEAR] if cam in ("neg", "mid") else [])
        for k, spec in enumerate(poses):
            R, t = EC.pose_of(spec, 6, 6)
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
        out[name] = (Batch(name, tables, 6, 6, CAMERAS[cam], max_drop=drop, iterations=it, flags=flags, tpf=40), PINNED_STATUS.get(name, status))
    R, t = PC.pose("tilt40", 1, 1)
    one = exact_table(1, 1, [0], CAMERAS["neg"], R, t, first_id=7)
    out["1x1"] = (Batch("1x1", [one, one[:0], PC.flat_row(one)], 1, 1, CAMERAS["neg"], first_id=7, flags=MISSING, tpf=3), [OK, FEW, SINGULAR])
    return out


def special_tables(cam):
    """Three exact 6 x 6 tables under `cam` (the alpha = 0.8 camera in the GPU launch):
    0: a corner observed exactly on the principal point;
    1: the board of BEHIND -- corners with Zc < 0 inside the cone, which the seed clamps (ray_z <= 0 or 1.5 rad and more off axis);
    2: the frontal board with one corner pushed out along its direction beyond the unprojection's domain (alpha > 0.5 only) and
       one to 1.52 rad off the axis in front of the image plane (the seed's clamp by angle)."""
    fx, fy, cx, cy, xi, al = [float(v) for v in cam[:6]]
    R, t = EC.axis_pose(0.0)
    on_axis = exact_table(6, 6, range(36), cam, R, t)
    on_axis["xy"][14, 4:6] = [cx, cy]
    R, t = behind_pose()
    behind = exact_table(6, 6, [i for i in range(36) if i not in BEHIND_MISSING], cam, R, t)
    R, t = EC.pose_of(PC.POSES["near"], 6, 6)
    pushed = exact_table(6, 6, range(36), cam, R, t)
    xy = pushed["xy"].reshape(36, 4, 2)
    if al > 0.5:
        r_out = 1.05 * np.sqrt(1.0 / (2.0 * al - 1.0))
        d = (xy[35, 2] - [cx, cy]) / [fx, fy]
        xy[35, 2] = np.array([cx, cy]) + d / np.linalg.norm(d) * r_out * np.array([fx, fy])
    a = 1.52
    xy[0, 0] = project_rays(cam, np.array([-np.sin(a) * np.sqrt(0.5), -np.sin(a) * np.sqrt(0.5), np.cos(a)]))
    return [on_axis, behind, pushed]
