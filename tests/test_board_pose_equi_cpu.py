"""agx_board_pose_tail_m at AGX_LENS_EQUIDISTANT, the host form of k_board_pose<AGX_LENS_EQUIDISTANT>
(tests/test_gpu_board_pose_equi.py holds the kernel to its bytes), against numpy and scipy statements of the pinhole-equidistant
model written independently of csrc/board_pose_math.h (tests/board_pose_equi_cases.py).

Measured on the host form (x86-64, the library's own build flags), each bound 10 x its measurement unless the issue fixes it:
  pose_atan     2.3e-16 absolute at worst against numpy.arctan over the grid (bound 1e-14, fixed); monotone over the sorted grid;
  projection    3.5e-13 px at worst against the numpy model over rays up to 85 degrees, four cameras (bound 1e-9 px, fixed);
  seed          iterations = 0 on exact data of a fronto-parallel board: the seed reprojects within 8.9e-6 px;
  step          iterate 1 against the finite-difference step: 1.8e-12 px at worst over eight cases; the bound is 10 x the
                finite-difference reference's own error as tests/test_board_pose_cpu.py records it (5.6e-8 px);
  exact data    3.5e-6 px at worst from the scipy yardstick's reprojection over 40 cases;
  noisy data    the sum of |e|^2 within 4.1e-10 relative of the yardstick's minimum at +-0.1 px of noise;
  the model     a board whose corners lie 77 degrees off the axis, +-0.1 px of noise: equidistant rms 0.078 px and predictions
                0.024 px off; radial-tangential with zero distortion 35.4 px and 127 px; board_fit 35.5 px and 137 px."""
import ctypes as C
import functools

import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi
from tests import board_pose_cases as PC
from tests import board_pose_equi_cases as EC
from tests.board_pose_cases import FEW, INPUT, LAYOUTS, LOOSE, OK, POSES, SINGULAR, TAG_SIZE
from tests.board_pose_equi_cases import CAMERAS

ATAN_BOUND = 1e-14
SEED_MEASURED = 8.9e-6   # px
EXACT_MEASURED = 3.5e-6  # px
NOISY_MEASURED = 4.1e-10  # relative
STEP_MEASURED = 5.6e-8   # px: the finite-difference reference's own error (tests/test_board_pose_cpu.py: STEP_SELF_MEASURED)
STEP_H, STEP_S = 1e-5, float(np.float32(0.3))
CASES = [(c, r, p, k) for c, r in LAYOUTS for p in sorted(POSES) for k in sorted(CAMERAS)]


# ---- pose_atan --------------------------------------------------------------------------------------------------------------------
def atan_breaks():
    """The points where pose_atan changes its path: (2 k + 1) / 16 (the table index steps), their reciprocals, and 1."""
    b = [(2 * k + 1) / 16.0 for k in range(8)]
    return b + [1.0 / v for v in b] + [1.0]


def library_atan(r):
    r = np.ascontiguousarray(r, np.float64)
    out = np.zeros_like(r)
    assert _ffi.lib().agx_debug_pose_atan(r.ctypes.data, len(r), out.ctypes.data) == _ffi.AGX_OK
    return out


def test_pose_atan_against_numpy_and_monotone():
    near = [f(v) for v in atan_breaks() for f in (lambda v: np.nextafter(v, 0.0), lambda v: v, lambda v: np.nextafter(v, np.inf))]
    r = np.sort(np.concatenate([[0.0], np.logspace(-300, 300, 200000), near]))
    got = library_atan(r)
    err = np.abs(got - np.arctan(r)).max()
    print("pose_atan: %.3g absolute at worst over %d values (bound %g)" % (err, len(r), ATAN_BOUND))
    assert err <= ATAN_BOUND and got[0] == 0.0
    assert np.all(np.diff(got) >= 0.0)
    bad = np.array([-1.0])
    assert _ffi.lib().agx_debug_pose_atan(bad.ctypes.data, 1, bad.ctypes.data) == _ffi.AGX_ERR_ARG
    bad = np.array([np.nan])
    assert _ffi.lib().agx_debug_pose_atan(bad.ctypes.data, 1, bad.ctypes.data) == _ffi.AGX_ERR_ARG


# ---- the projection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_projection_against_the_numpy_model(cam):
    ang, az = np.radians(np.linspace(0.0, 85.0, 341)), np.linspace(0.0, 2.0 * np.pi, 37)
    Q = np.array([[np.tan(a) * np.cos(z) * 0.7, np.tan(a) * np.sin(z) * 0.7, 0.7] for a in ang for z in az])
    d = np.abs(EC.library_project(CAMERAS[cam], Q) - EC.project_rays(CAMERAS[cam], Q)).max()
    print("projection under %s: %.3g px at worst over %d rays up to 85 degrees (bound 1e-9)" % (cam, d, len(Q)))
    assert d <= 1e-9
    behind = EC.library_project(CAMERAS[cam], [[0.1, 0.1, 0.0], [0.1, 0.1, -1.0]])
    assert np.isnan(behind).all()


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_projection_is_continuous_across_the_small_r_threshold_and_exact_on_the_axis(cam):
    c = CAMERAS[cam]
    assert EC.library_project(c, [[0.0, 0.0, 1.0], [0.0, 0.0, 3.5]]).tolist() == [[c.cx, c.cy]] * 2
    # x = r exactly (Z = 1, Y = 0): r2 = x x straddles 2^-13 at the two neighbours of 2^-6.5 in binary64
    x = np.sqrt(EC.SMALL_R2)
    lo, hi = (x, np.nextafter(x, 1.0)) if x * x < EC.SMALL_R2 else (np.nextafter(x, 0.0), x)
    assert lo * lo < EC.SMALL_R2 <= hi * hi
    u = EC.library_project(c, [[lo, 0.0, 1.0], [hi, 0.0, 1.0]])[:, 0] - c.cx
    # the two branches at neighbouring arguments: u / (fx x) = s is the same function of r to 1e-15 relative
    s_lo, s_hi = u[0] / (c.fx * lo), u[1] / (c.fx * hi)
    want = EC.project_rays(c, np.array([[lo, 0.0, 1.0], [hi, 0.0, 1.0]]))[:, 0] - c.cx
    print("threshold under %s: s below %.17g, above %.17g (relative difference %.3g); numpy %.3g relative" %
          (cam, s_lo, s_hi, abs(s_lo - s_hi) / s_hi, np.abs(u / want - 1.0).max()))
    assert abs(s_lo - s_hi) <= 1e-15 * s_hi
    assert np.abs(u / want - 1.0).max() <= 1e-15


# ---- the seed -----------------------------------------------------------------------------------------------------------------------
def frontal_table(cam, z):
    R, t = PC.rotation(0.0, 0.0, 3.0), np.array([0.002, -0.001, z])
    return EC.exact_table(6, 6, range(36), cam, R, t), R, t


def test_the_seed_round_trip_on_a_fronto_parallel_board():
    """iterations = 0 on exact data: the homography through the undistorted corners is the pose's own, so the seed reprojects at
    the level of the binary32 observations (measured 8.9e-6 px at worst over the four cameras; bound 10 x)."""
    worst = 0.0
    P = PC.board_points(6, 6, tag_size=TAG_SIZE)
    for cam in sorted(CAMERAS):
        table, R, t = frontal_table(CAMERAS[cam], 0.28)
        got = A.board_pose(table, 6, 6, CAMERAS[cam], tag_size=TAG_SIZE, iterations=0)
        assert got["status"] == OK and got["best_iter"] == 0
        worst = max(worst, np.linalg.norm(EC.project(CAMERAS[cam], got["R"], got["t"], P) - EC.project(CAMERAS[cam], R, t, P), axis=-1).max())
    print("seed: %.3g px at worst from the true reprojection (recorded %.3g, bound 10 x)" % (worst, SEED_MEASURED))
    assert worst <= 10.0 * SEED_MEASURED


def test_corners_beyond_the_seeds_clamp_give_a_finite_seed():
    """Observed corners at theta_d = 1.6 rad, beyond POSE_EQUI_THETA_MAX = 1.5 rad: the outermost corners of a board 2 cm from
    the lens pushed outwards along their rays' directions in the image.  The seed clamps them and stays finite."""
    cam = CAMERAS["zero"]
    table, R, t = frontal_table(cam, 0.02)
    far = table.copy()
    xy = far["xy"].reshape(-1, 4, 2)
    c = np.array([cam.cx, cam.cy], np.float32)
    radius = np.linalg.norm(xy - c, axis=-1)
    outer = radius > 0.95 * radius.max()
    xy[outer] = c + (xy[outer] - c) / radius[outer][:, None] * np.float32(1.6 * cam.fx)  # theta_d = 1.6 rad
    assert (np.linalg.norm(xy - c, axis=-1) / cam.fx).max() > EC.THETA_MAX
    got = A.board_pose(far, 6, 6, cam, tag_size=TAG_SIZE, iterations=0, max_err_sq=1e30)
    assert got["status"] in (OK, LOOSE) and np.isfinite(got["pose"]).all() and np.isfinite(got["rms"])


# ---- one Gauss-Newton step against a step from a finite-difference Jacobian ---------------------------------------------------------
def cayley(w):
    a = np.asarray(w, np.float64) / 2.0
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.linalg.solve(np.eye(3) - K, np.eye(3) + K)


def reference_step(cam, R0, t0, P, obs, h):
    def f(d):
        return EC.project(cam, R0 @ cayley(d[:3]), t0 + d[3:], P).ravel()

    J = np.empty((obs.size, 6))
    for i in range(6):
        d = np.zeros(6)
        d[i] = h if i < 3 else h * TAG_SIZE
        J[:, i] = (f(d) - f(-d)) / (2.0 * d[i])
    step = np.linalg.lstsq(J, obs.ravel() - f(np.zeros(6)), rcond=None)[0]
    U, _, Vt = np.linalg.svd(R0 @ cayley(step[:3]))
    return U @ Vt, t0 + step[3:]


STEP_POSES = {"tilt40": PC.POSES["tilt40"], "near": PC.POSES["near"], "vnear": EC.VNEAR}
STEP_CASES = [(cam, p) for cam in ("kalibr", "four", "wide") for p in ("tilt40", "near")] + [("wide", "vnear"), ("four", "axis")]


@pytest.mark.parametrize("cam,p", STEP_CASES)
def test_one_gauss_newton_step_is_the_finite_difference_step(cam, p):
    """tests/test_board_pose_cpu.py's method over the equidistant cameras: iterate 1 from the seed against the step of a Jacobian
    taken by central differences of the numpy projection.  "axis": a board whose centre corner lies on the optical axis (the
    Jacobian's small-r branch).  Measured: 1.8e-12 px at worst; bound 10 x the finite-difference reference's own
    error as recorded there (5.6e-8 px)."""
    c = CAMERAS[cam]
    R, t = EC.axis_pose(0.0) if p == "axis" else EC.pose_of(STEP_POSES[p], 6, 6)
    table = EC.exact_table(6, 6, range(36), c, R, t, s=STEP_S, noise=0.1, seed=11)
    seed = A.board_pose(table, 6, 6, c, tag_size=TAG_SIZE, spacing_ratio=STEP_S, iterations=0, max_err_sq=1e30)
    got = A.board_pose(table, 6, 6, c, tag_size=TAG_SIZE, spacing_ratio=STEP_S, iterations=1, max_err_sq=1e30)
    assert seed["status"] == OK and seed["best_iter"] == 0 and got["status"] == OK and got["best_iter"] == 1, (cam, p)
    P = PC.board_points(6, 6, STEP_S, TAG_SIZE)
    obs = table["xy"].astype(np.float64).reshape(36, 4, 2)
    ref = EC.project(c, *reference_step(c, seed["R"], seed["t"], P, obs, STEP_H), P)
    mine = EC.project(c, got["R"], got["t"], P)
    moved = np.linalg.norm(mine - EC.project(c, seed["R"], seed["t"], P), axis=-1).max()
    d = np.linalg.norm(mine - ref, axis=-1).max()
    print("step %s / %s: iterate 1 is %.3g px from the reference's (the step moved the corners %.3g px; bound %.3g px)" % (cam, p, d, moved, 10 * STEP_MEASURED))
    assert moved > 0.01 and d <= 10.0 * STEP_MEASURED


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved(cols, rows, p, cam, noise):
    R, t = PC.pose(p, cols, rows)
    table = EC.exact_table(cols, rows, range(cols * rows), CAMERAS[cam], R, t, noise=noise, seed=11)
    got = A.board_pose(table, cols, rows, CAMERAS[cam], tag_size=TAG_SIZE)
    return table, got, EC.yardstick(table, cols, rows, CAMERAS[cam], R, t), (R, t)


def test_exact_data_reprojects_like_the_yardstick():
    """Measured: 3.5e-6 px at worst over the 40 cases (the binary32 observations' level); bound 10 x."""
    worst = 0.0
    for cols, rows, p, cam in CASES:
        table, got, (Ry, ty, _), (R, t) = solved(cols, rows, p, cam, 0.0)
        assert got["status"] == OK, (cols, rows, p, cam)
        P = PC.board_points(cols, rows, tag_size=TAG_SIZE)
        worst = max(worst, np.linalg.norm(EC.project(CAMERAS[cam], got["R"], got["t"], P) - EC.project(CAMERAS[cam], Ry, ty, P), axis=-1).max())
        assert np.abs(got["R"].T @ got["R"] - np.eye(3)).max() < 1e-14
        assert np.abs(got["R"] - R).max() < 1e-4 and np.abs(got["t"] - t).max() < 1e-4 * PC.extent(cols, rows), (p, cam)
        assert np.abs(got["pred"]["xy"].reshape(-1, 4, 2) - EC.project(CAMERAS[cam], got["R"], got["t"], P)).max() < 1e-4
    print("exact data: %.3g px at worst from the yardstick over %d cases (recorded %.3g, bound 10 x)" % (worst, len(CASES), EXACT_MEASURED))
    assert worst <= 10.0 * EXACT_MEASURED


def test_noisy_data_reaches_the_yardsticks_minimum():
    """Measured: the sum of |e|^2 at most 4.1e-10 relative above the yardstick's minimum at +-0.1 px of noise; bound 10 x."""
    worst = -1.0
    for cols, rows, p, cam in CASES:
        table, got, (_, _, ssq), _ = solved(cols, rows, p, cam, 0.1)
        assert got["status"] == OK
        mine = float(np.sum((EC.project(CAMERAS[cam], got["R"], got["t"], PC.board_points(cols, rows, tag_size=TAG_SIZE)) -
                             table["xy"].astype(np.float64).reshape(-1, 4, 2)) ** 2))
        worst = max(worst, (mine - ssq) / ssq)
        assert abs(mine / (4 * len(table)) - float(got["rms"]) ** 2) < 1e-6
    print("noisy data: relative gap to the yardstick's minimum %.3g at worst (recorded %.3g, bound 10 x)" % (worst, NOISY_MEASURED))
    assert worst <= 10.0 * NOISY_MEASURED


# ---- what the model is for ----------------------------------------------------------------------------------------------------------
def test_what_the_model_is_for():
    """A 6 x 6 board filling the wide lens (fx = 0.3 of the width), its outer corners 77 degrees off the axis (>= 60 asked), +-0.1
    px of noise, the four corner tags taken out and predicted.  Recorded: equidistant pose rms 0.0785 px, predictions of the missing
    outer-ring tags 0.024 px off at worst; the radial-tangential pose with zero distortion 35.4 px and 127 px; board_fit 35.5 px and 137 px.
    Asserted: the equidistant rms is at noise level, the others are worse by at least the factor 10 in rms and prediction."""
    cam = CAMERAS["wide"]
    R, t = EC.pose_of(EC.VNEAR, 6, 6)
    P = PC.board_points(6, 6, tag_size=TAG_SIZE)
    assert EC.field_angle(R, t, P) >= 60.0
    full = EC.exact_table(6, 6, range(36), cam, R, t, noise=0.1, seed=3)
    miss = [0, 5, 30, 35]
    keep = np.array([i for i in range(36) if i not in miss])
    truth = EC.project(cam, R, t, P)[miss]
    kw = dict(max_err_sq=1e30, predict_missing=True)
    equi = A.board_pose(full[keep], 6, 6, cam, tag_size=TAG_SIZE, **kw)
    radtan = A.board_pose(full[keep], 6, 6, A.Camera(*cam[:4]), tag_size=TAG_SIZE, **kw)
    fit = A.board_fit(full[keep], 6, 6, PC.SIZE, **kw)
    out = {}
    for name, r in (("equidistant", equi), ("radtan", radtan), ("board_fit", fit)):
        assert r["status"] in (OK, LOOSE) and r["pred"]["id"].tolist() == miss, name
        out[name] = (float(r["rms"]), float(np.linalg.norm(r["pred"]["xy"].reshape(4, 4, 2) - truth, axis=-1).max()))
        print("%s: rms %.4g px, worst outer-ring prediction %.4g px off" % ((name,) + out[name]))
    assert out["equidistant"][0] < 0.2
    for name in ("radtan", "board_fit"):
        assert out[name][0] >= 10.0 * out["equidistant"][0] and out[name][1] >= 10.0 * out["equidistant"][1], name


# ---- arguments and the contract -----------------------------------------------------------------------------------------------------
def tail_m(table, cols, rows, model, cam9, iterations=10, tag_size=TAG_SIZE, max_drop=0, first_id=0):
    """agx_board_pose_tail_m into sentinel-filled arrays -> (rc, EquiBatch outputs)."""
    b = EC.EquiBatch("args", [table], cols, rows, CAMERAS["kalibr"], tag_size=tag_size, first_id=first_id, max_drop=max_drop, iterations=iterations)
    out, t = b.empty_outputs(), b.table()
    u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    rc = _ffi.lib().agx_board_pose_tail_m(
        t[0].ctypes.data, b.tpf, b.counts[0], 0, cols, rows, first_id, 0.3, float(tag_size), model, (C.c_double * 9)(*cam9), 4.0, max_drop, 1, iterations, 0,
        out["pose"][0].ctypes.data, out["err_sq"][0].ctypes.data, out["row_status"][0].ctypes.data, C.cast(out["n_inliers"].ctypes.data, u32),
        C.cast(out["rms"].ctypes.data, f32), C.cast(out["best_iter"].ctypes.data, u32), out["pred"][0].ctypes.data, C.cast(out["n_pred"].ctypes.data, u32),
        C.cast(out["status"].ctypes.data, u32))
    return rc, out


def test_unknown_models_and_a_non_zero_ninth_double_are_refused():
    cam = CAMERAS["kalibr"]
    R, t = PC.pose("tilt40", 6, 6)
    table = EC.exact_table(6, 6, range(36), cam, R, t)
    good = PC.camera_args(cam)
    assert tail_m(table, 6, 6, EC.EQUI, good)[0] == _ffi.AGX_OK
    for model, c9 in ((2, good), (-1, good), (EC.EQUI, good[:8] + [-0.02]), (EC.EQUI, good[:8] + [5e-324]), (EC.EQUI, good[:4] + [np.nan] + good[5:]),
                      (EC.EQUI, [0.0] + good[1:])):
        rc, out = tail_m(table, 6, 6, model, c9)
        assert rc == _ffi.AGX_ERR_ARG and all(PC.untouched(out[k]) for k in PC.KEYS), (model, c9)
    sums = np.zeros(11)
    st = C.c_uint32(0)
    head = (table.ctypes.data, 36, 36, 0, 6, 6, 0, 0.3, TAG_SIZE)
    assert _ffi.lib().agx_debug_board_pose_sums_m(*head, 2, (C.c_double * 9)(*good), 4.0, 0, 1, 10, 0, C.byref(st), sums.ctypes.data) == _ffi.AGX_ERR_ARG
    assert _ffi.lib().agx_debug_board_pose_sums_m(*head, EC.EQUI, (C.c_double * 9)(*good), 4.0, 0, 1, 10, 0, C.byref(st), sums.ctypes.data) == _ffi.AGX_OK
    assert st.value == OK and np.isfinite(sums[0]) and np.nanmin(sums) <= sums[0]
    with pytest.raises(A.AgxError):
        A.board_pose(table, 6, 6, cam._replace(k3=0.1))  # (the ninth field by position: _replace names the tuple's fields)
    assert A.Camera(1.0, 1.0, 0.0, 0.0).model == EC.RADTAN and cam.model == EC.EQUI and cam.k3 == -0.013 and cam.k4 == 0.0026
    assert isinstance(cam, A.Camera) and len(cam) == 9 and cam[8] == 0.0


def test_refused_frames_write_their_status_and_two_zero_counts_only():
    cam = CAMERAS["four"]
    R, t = PC.pose("tilt40", 6, 6)
    table = EC.exact_table(6, 6, range(36), cam, R, t)
    b = EC.EquiBatch("refused", [table[:0], PC.flat_row(table), PC.nan_row(table), table], 6, 6, cam)
    out = b.host()
    assert out["status"][:4].tolist() == [FEW, SINGULAR, INPUT, OK]
    for f in range(3):
        assert out["n_inliers"][f] == 0 and out["n_pred"][f] == 0
        assert all(PC.untouched(out[k][f]) for k in ("pose", "err_sq", "row_status", "rms", "best_iter", "pred"))
    assert all(PC.untouched(out[k][4:]) for k in PC.KEYS)


def test_a_wrong_id_is_dropped_in_one_round_and_a_tie_goes_to_the_lower_row():
    cam = CAMERAS["kalibr"]
    R, t = PC.pose("tilt40", 6, 6)
    t36 = EC.exact_table(6, 6, range(36), cam, R, t, noise=0.1)
    wrong = PC._wrong(t36, 1)
    got = A.board_pose(wrong, 6, 6, cam, tag_size=TAG_SIZE, max_drop=1)
    assert got["status"] == OK and got["n_inliers"] == len(wrong) - 1 and got["row_status"].tolist().count(PC.OUTLIER) == 1
    assert got["row_status"][2] == PC.OUTLIER and got["rms"] < 0.2
    assert A.board_pose(wrong, 6, 6, cam, tag_size=TAG_SIZE, max_drop=0)["status"] == LOOSE
    tie = np.concatenate([wrong[:3], wrong[2:]])  # the wrong row twice: equal residual bits, the lower row goes first
    got = A.board_pose(tie, 6, 6, cam, tag_size=TAG_SIZE, max_drop=1)
    assert got["status"] == LOOSE and got["row_status"][2] == PC.OUTLIER and got["row_status"][3] == PC.INLIER
    got = A.board_pose(tie, 6, 6, cam, tag_size=TAG_SIZE, max_drop=2)
    assert got["status"] == OK and got["row_status"][2] == got["row_status"][3] == PC.OUTLIER


def test_layouts_1_by_1_and_64_by_64_and_a_prediction_behind_the_camera():
    cam = CAMERAS["kalibr"]
    R, t = PC.pose("tilt40", 1, 1)
    one = EC.exact_table(1, 1, [0], cam, R, t, first_id=7)
    got = A.board_pose(one, 1, 1, cam, tag_size=TAG_SIZE, first_id=7)
    assert got["status"] == OK and got["n_inliers"] == 1 and len(got["pred"]) == 1
    R, t = PC.pose("tilt40", 64, 64, 0.01)
    ids = np.random.RandomState(3).permutation(4096)[:200]
    table = EC.exact_table(64, 64, ids, cam, R, t, 0.01, first_id=5, noise=0.05)
    got = A.board_pose(table, 64, 64, cam, tag_size=0.01, first_id=5)
    assert got["status"] == OK and got["rms"] < 0.1 and len(got["pred"]) == 4096
    want = EC.project(cam, got["R"], got["t"], PC.board_points(64, 64, tag_size=0.01))
    assert np.nanmax(np.abs(got["pred"]["xy"].reshape(4096, 4, 2) - want)) < 1e-3
    # a board through the camera's plane: a 64 x 64 board 5 mm ahead, tilted by 60 degrees -- its far half lies behind
    R, t = PC.rotation(8.0, 60.0, 10.0), np.array([0.0, 0.0, 0.1])
    near = np.arange(4096)[(PC.board_points(64, 64, tag_size=0.01) @ R.T + t)[:, :, 2].min(axis=1) > 0.05][:300]
    table = EC.exact_table(64, 64, near, cam, R, t, 0.01)
    got = A.board_pose(table, 64, 64, cam, tag_size=0.01, max_err_sq=1e30)
    assert got["status"] in (OK, LOOSE)
    Z = (PC.board_points(64, 64, tag_size=0.01) @ got["R"].T + got["t"])[:, :, 2]
    pred = got["pred"]["xy"].reshape(4096, 4, 2)
    assert (Z <= 0.0).any() and np.isnan(pred[Z <= 0.0]).all() and np.isfinite(pred[Z > 1e-6]).all()


@pytest.mark.parametrize("name", ("6x6_mild_it10_drop2_all", "6x6_full_it10_drop2_missing", "6x6_barrel_it0_drop2_missing", "1x1", "64x64_full_it10_drop2_missing"))
def test_the_m_forms_at_radtan_give_the_existing_forms_bytes(name):
    b, _ = PC.gpu_batches()[name]
    want = b.host()
    m = EC.EquiBatch(name, b.tables, b.cols, b.rows, b.cam, b.tag_size, b.first_id, b.s, b.max_err_sq, b.max_drop, b.min_tags, b.iterations, b.flags,
                     b.counts, b.tag_status, b.tpf)
    got = m.host(model=EC.RADTAN)
    for k in PC.KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (name, k)


def test_the_abi_declares_the_lens_models():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "aprilgrid_amd.h")).read()
    rust = open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(root, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"enum \{ AGX_LENS_RADTAN = 0, AGX_LENS_EQUIDISTANT = 1 \};", hdr)
    assert (_ffi.AGX_LENS_RADTAN, _ffi.AGX_LENS_EQUIDISTANT) == (0, 1) and _ffi.lib().agx_abi_version() == 1
    for fn, n in (("agx_board_pose_enqueue_m", 27), ("agx_board_pose_tail_m", 25), ("agx_debug_board_pose_sums_m", 18), ("agx_debug_pose_atan", 3)):
        assert re.search(r"\bint %s\(" % fn, hdr) and ("pub fn %s(" % fn) in rust and len(_ffi.SYMBOLS[fn][1]) == n, fn
        assert getattr(_ffi.lib(), fn).argtypes == _ffi.SYMBOLS[fn][1]
    for text in ("pub enum LensModel", "pub fn equidistant(", "pub fn board_pose_tail_m("):
        assert text in lib_rs, text


# ---- recovery on a rendered frame seen through a fisheye ----------------------------------------------------------------------------
WARP_COUNTS = {"equidistant": 36, "none": 34, "radtan": 33}  # tags after the recovery of the four that were taken out, as measured


def test_on_a_frame_seen_through_a_fisheye_the_equidistant_camera_recovers_strictly_more_tags():
    """The rendered 6 x 6 frame warped through an equidistant lens of 0.62 of the pinhole's focal length (board_pose_equi_cases.
    warped_frame; at 0.5 the oracle's detect loses four tags, at 0.62 and 0.75 it keeps all 36), four outer-ring tags taken out of the
    table: recovered_host brings back 4 of 4 with the equidistant camera (pose rms 0.030 px), 2 of 4 without a camera (board_fit rms
    0.875 px) and 1 of 4 with the zero-distortion radial-tangential camera (rms 1.349 px)."""
    luma, cam, radtan, saddles, tags, (w, h, rows, cols) = EC.warped_frame()
    assert len(tags) >= 34
    less = {t: xy for t, xy in tags.items() if t not in EC.WARP_MISSING}
    assert len(less) == len(tags) - 4
    got = {}
    for name, c in (("equidistant", cam), ("none", None), ("radtan", radtan)):
        out, fit = PC.recovered_host(luma, saddles, less, cols, rows, camera=c)
        got[name] = len(out)
        print("fisheye frame, %s: %d tags, fit status %d, rms %.3f px" % (name, len(out), fit["status"], fit["rms"]))
    assert got["equidistant"] > got["none"] and got["equidistant"] > got["radtan"]
    assert got == WARP_COUNTS
