"""agx_board_pose_tail_m at AGX_LENS_DOUBLE_SPHERE, the host form of k_board_pose<AGX_LENS_DOUBLE_SPHERE>
(tests/test_gpu_board_pose_ds.py holds the kernel to its bytes), against numpy and scipy statements of the double-sphere model
written independently of csrc/board_pose_math.h (tests/board_pose_ds_cases.py).

Measured on the host form (x86-64, the library's own build flags), each bound 10 x its measurement:
  projection    2.9e-11 px at worst against the numpy restatement over rays from the axis to 0.999 of each camera's valid cone,
                rays with Z < 0 included, four cameras (the worst lies at the cone's edge, where the denominator is small;
                9.1e-13 px under the other three cameras);
  pinhole limit 1.3e-12 px between the poses through model 2 at (xi, alpha) = (0, 0) and through AGX_LENS_RADTAN;
  seed          iterations = 0 on exact data of a fronto-parallel board: 9.8e-6 px from the truth;
  step          iterate 1 against the finite-difference step of the restatement: 8.6e-10 px at worst (the board behind the
                image plane, whose step moves the corners 90 px; 2e-12 px in the other cases);
  exact data    9.0e-6 px at worst from the scipy yardstick's reprojection over 40 cases;
  noisy data    the sum of |e|^2 within 1.7e-9 relative of the yardstick's minimum at +-0.1 px of noise;
  the model     a board reaching behind the image plane: pose rms 0.079 px at +-0.1 px of noise, the predicted rows of the Zc < 0
                tags 0.020 px from the truth at worst; the equidistant zero-coefficient pose of the same table is AGX_FIT_LOOSE
                with an infinite rms and predicts 25 of those 28 corners as NaN, the other three 78 px off."""
import ctypes as C
import functools

import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi
from tests import board_pose_cases as PC
from tests import board_pose_equi_cases as EC
from tests import board_pose_ds_cases as DC
from tests.board_pose_cases import LAYOUTS, LOOSE, OK, POSES, TAG_SIZE
from tests.board_pose_ds_cases import CAMERAS, DS

PROJ_MEASURED = 2.9e-11   # px
PINHOLE_MEASURED = 1.3e-12  # px
SEED_MEASURED = 9.8e-6   # px
STEP_MEASURED = 8.6e-10  # px
EXACT_MEASURED = 9.0e-6   # px
NOISY_MEASURED = 1.7e-9   # relative
BEHIND_MEASURED = 0.020    # px
STEP_H, STEP_S = 1e-5, float(np.float32(0.3))
CASES = [(c, r, p, k) for c, r in LAYOUTS for p in sorted(POSES) for k in sorted(CAMERAS)]


def test_the_constant_and_the_camera():
    assert getattr(_ffi, "AGX_LENS_DOUBLE_SPHERE", None) == DS
    cam = CAMERAS["neg"]
    assert isinstance(cam, A.Camera) and cam.model == DS and cam.xi == -0.2 and cam.alpha == 0.59 and len(cam) == 9 and tuple(cam[6:]) == (0.0, 0.0, 0.0)
    assert "double_sphere" in repr(cam)


# ---- the projection -----------------------------------------------------------------------------------------------------------------
def cone_rays(cam, n_ang=400, frac=0.999):
    lim = DC.cone_angle(cam) * frac
    ang, az = np.linspace(0.0, lim, n_ang), np.linspace(0.0, 2.0 * np.pi, 37)
    return np.array([[np.sin(a) * np.cos(z) * 0.7, np.sin(a) * np.sin(z) * 0.7, np.cos(a) * 0.7] for a in ang for z in az])


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_projection_against_the_numpy_restatement(cam):
    c = CAMERAS[cam]
    Q = cone_rays(c)
    assert DC.valid(c, Q).all() and ((Q[:, 2] < 0.0).any() or cam == "pinhole")
    got, want = EC.library_project(c, Q), DC.project_rays(c, Q)
    assert np.isfinite(want).all()
    d = np.abs(got - want).max()
    print("projection under %s: %.3g px at worst over %d rays out to %.1f degrees (recorded %.3g, bound 10 x)" %
          (cam, d, len(Q), np.degrees(DC.cone_angle(c) * 0.999), PROJ_MEASURED))
    assert d <= 10.0 * PROJ_MEASURED
    lim = DC.cone_angle(c)
    outside = [[np.sin(a), 0.0, np.cos(a)] for a in (lim * 1.001, min(lim * 1.2, np.pi), np.pi) if a <= np.pi] + [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0]]
    assert not DC.valid(c, np.array(outside)).any()
    assert np.isnan(EC.library_project(c, outside)).all()
    assert EC.library_project(c, [[0.0, 0.0, 2.0]]).tolist() == [[c.cx, c.cy]]


# ---- the pinhole limit ----------------------------------------------------------------------------------------------------------------
def test_the_pinhole_limit_is_the_radial_tangential_pose():
    cam, pin = CAMERAS["pinhole"], A.Camera(*CAMERAS["pinhole"][:4])
    worst = 0.0
    for cols, rows in LAYOUTS:
        for p in sorted(POSES):
            R, t = PC.pose(p, cols, rows)
            table = PC.exact_table(cols, rows, range(cols * rows), pin, R, t)
            a = A.board_pose(table, cols, rows, cam, tag_size=TAG_SIZE)
            b = A.board_pose(table, cols, rows, pin, tag_size=TAG_SIZE)
            assert a["status"] == OK and b["status"] == OK
            P = PC.board_points(cols, rows, tag_size=TAG_SIZE)
            worst = max(worst, np.linalg.norm(PC.project(pin, a["R"], a["t"], P) - PC.project(pin, b["R"], b["t"], P), axis=-1).max())
            worst = max(worst, np.abs(a["pred"]["xy"] - b["pred"]["xy"]).max())
    print("pinhole limit: %.3g px at worst between the two models' poses (recorded %.3g, bound 10 x)" % (worst, PINHOLE_MEASURED))
    assert worst <= 10.0 * PINHOLE_MEASURED


# ---- the seed -----------------------------------------------------------------------------------------------------------------------
def frontal_table(cam, z):
    R, t = PC.rotation(0.0, 0.0, 3.0), np.array([0.002, -0.001, z])
    return DC.exact_table(6, 6, range(36), cam, R, t), R, t


def test_the_seed_round_trip_on_a_fronto_parallel_board():
    worst = 0.0
    P = PC.board_points(6, 6, tag_size=TAG_SIZE)
    for cam in sorted(CAMERAS):
        table, R, t = frontal_table(CAMERAS[cam], 0.28)
        got = A.board_pose(table, 6, 6, CAMERAS[cam], tag_size=TAG_SIZE, iterations=0)
        assert got["status"] == OK and got["best_iter"] == 0
        worst = max(worst, np.linalg.norm(DC.project(CAMERAS[cam], got["R"], got["t"], P) - DC.project(CAMERAS[cam], R, t, P), axis=-1).max())
    print("seed: %.3g px at worst from the true reprojection (recorded %.3g, bound 10 x)" % (worst, SEED_MEASURED))
    assert worst <= 10.0 * SEED_MEASURED


def test_the_unprojection_restated_inverts_the_projection():
    """(of the yardstick itself: the seed's domain and clamp cases below are chosen with it)"""
    for cam in sorted(CAMERAS):
        c = CAMERAS[cam]
        Q = cone_rays(c, 60, 0.98)
        uv = DC.project_rays(c, Q)
        assert DC.in_domain(c, uv[:, 0], uv[:, 1]).all()
        ray = DC.unproject(c, uv[:, 0], uv[:, 1])
        ray = ray / np.linalg.norm(ray, axis=-1, keepdims=True)
        assert np.abs(ray - Q / 0.7).max() < 1e-9, cam


@pytest.mark.parametrize("what", ("beyond_1.5_rad", "ray_z_not_positive", "outside_the_domain", "principal_point"))
def test_the_seed_stays_finite_where_it_clamps(what):
    cam = CAMERAS["high"]
    fx, fy, cx, cy = cam[:4]
    table, R, t = frontal_table(cam, 0.1)
    xy = table["xy"].reshape(36, 4, 2)
    if what == "beyond_1.5_rad":
        px = DC.project_rays(cam, np.array([np.sin(1.52), 0.0, np.cos(1.52)]))
        ray = DC.unproject(cam, px[0], px[1])
        assert ray[2] > 0.0 and np.arctan2(np.hypot(ray[0], ray[1]), ray[2]) > DC.THETA_MAX
    elif what == "ray_z_not_positive":
        px = DC.project_rays(cam, np.array([np.sin(1.7), 0.0, np.cos(1.7)]))
        assert DC.in_domain(cam, px[0], px[1]) and DC.unproject(cam, px[0], px[1])[2] < 0.0
    elif what == "outside_the_domain":
        px = np.array([cx + 1.4 * fx, cy])
        assert not DC.in_domain(cam, px[0], px[1])
    else:
        px = np.array([cx, cy])
    xy[17, 1] = px
    assert np.array_equal(xy[17, 1], np.float32(px)) or what != "principal_point"
    got = A.board_pose(table, 6, 6, cam, tag_size=TAG_SIZE, iterations=0, max_err_sq=1e30)
    assert got["status"] in (OK, LOOSE) and np.isfinite(got["pose"]).all() and np.isfinite(got["rms"]), what
    got = A.board_pose(table, 6, 6, cam, tag_size=TAG_SIZE, iterations=10, max_err_sq=1e30)
    assert got["status"] in (OK, LOOSE) and np.isfinite(got["pose"]).all() and np.isfinite(got["rms"]), what


# ---- one Gauss-Newton step against a step from a finite-difference Jacobian ---------------------------------------------------------
def cayley(w):
    a = np.asarray(w, np.float64) / 2.0
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.linalg.solve(np.eye(3) - K, np.eye(3) + K)


def reference_step(cam, R0, t0, P, obs, h):
    def f(d):
        return DC.project(cam, R0 @ cayley(d[:3]), t0 + d[3:], P).ravel()

    J = np.empty((obs.size, 6))
    for i in range(6):
        d = np.zeros(6)
        d[i] = h if i < 3 else h * TAG_SIZE
        J[:, i] = (f(d) - f(-d)) / (2.0 * d[i])
    step = np.linalg.lstsq(J, obs.ravel() - f(np.zeros(6)), rcond=None)[0]
    U, _, Vt = np.linalg.svd(R0 @ cayley(step[:3]))
    return U @ Vt, t0 + step[3:]


STEP_POSES = {"tilt40": PC.POSES["tilt40"], "near": PC.POSES["near"], "vnear": EC.VNEAR, "behind": DC.BEHIND}
STEP_CASES = [(cam, p) for cam in ("neg", "mid", "high") for p in ("tilt40", "near")] + [("mid", "vnear"), ("neg", "behind"), ("pinhole", "axis")]


@pytest.mark.parametrize("cam,p", STEP_CASES)
def test_one_gauss_newton_step_is_the_finite_difference_step(cam, p):
    """tests/test_board_pose_equi_cpu.py's construction: iterate 1 from the seed against the step of a Jacobian taken by central
    differences of the numpy restatement.  "behind": corners with Zc < 0, where no x = X / Z exists."""
    c = CAMERAS[cam]
    R, t = EC.axis_pose(0.0) if p == "axis" else EC.pose_of(STEP_POSES[p], 6, 6)
    table = DC.exact_table(6, 6, range(36), c, R, t, s=STEP_S, noise=0.1, seed=11)
    seed = A.board_pose(table, 6, 6, c, tag_size=TAG_SIZE, spacing_ratio=STEP_S, iterations=0, max_err_sq=1e30)
    got = A.board_pose(table, 6, 6, c, tag_size=TAG_SIZE, spacing_ratio=STEP_S, iterations=1, max_err_sq=1e30)
    assert seed["status"] == OK and seed["best_iter"] == 0 and got["status"] == OK and got["best_iter"] == 1, (cam, p)
    P = PC.board_points(6, 6, STEP_S, TAG_SIZE)
    obs = table["xy"].astype(np.float64).reshape(36, 4, 2)
    ref = DC.project(c, *reference_step(c, seed["R"], seed["t"], P, obs, STEP_H), P)
    mine = DC.project(c, got["R"], got["t"], P)
    moved = np.linalg.norm(mine - DC.project(c, seed["R"], seed["t"], P), axis=-1).max()
    d = np.linalg.norm(mine - ref, axis=-1).max()
    print("step %s / %s: iterate 1 is %.3g px from the reference's (the step moved the corners %.3g px; recorded %.3g, bound 10 x)" % (cam, p, d, moved, STEP_MEASURED))
    assert moved > 0.01 and d <= 10.0 * STEP_MEASURED


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved(cols, rows, p, cam, noise):
    R, t = PC.pose(p, cols, rows)
    table = DC.exact_table(cols, rows, range(cols * rows), CAMERAS[cam], R, t, noise=noise, seed=11)
    got = A.board_pose(table, cols, rows, CAMERAS[cam], tag_size=TAG_SIZE)
    return table, got, DC.yardstick(table, cols, rows, CAMERAS[cam], R, t), (R, t)


def test_exact_data_reprojects_like_the_yardstick():
    worst = 0.0
    for cols, rows, p, cam in CASES:
        table, got, (Ry, ty, _), (R, t) = solved(cols, rows, p, cam, 0.0)
        assert got["status"] == OK, (cols, rows, p, cam)
        P = PC.board_points(cols, rows, tag_size=TAG_SIZE)
        worst = max(worst, np.linalg.norm(DC.project(CAMERAS[cam], got["R"], got["t"], P) - DC.project(CAMERAS[cam], Ry, ty, P), axis=-1).max())
        assert np.abs(got["R"].T @ got["R"] - np.eye(3)).max() < 1e-14
        assert np.abs(got["R"] - R).max() < 1e-4 and np.abs(got["t"] - t).max() < 1e-4 * PC.extent(cols, rows), (p, cam)
        assert np.abs(got["pred"]["xy"].reshape(-1, 4, 2) - DC.project(CAMERAS[cam], got["R"], got["t"], P)).max() < 1e-4
    print("exact data: %.3g px at worst from the yardstick over %d cases (recorded %.3g, bound 10 x)" % (worst, len(CASES), EXACT_MEASURED))
    assert worst <= 10.0 * EXACT_MEASURED


def test_noisy_data_reaches_the_yardsticks_minimum():
    worst = -1.0
    for cols, rows, p, cam in CASES:
        table, got, (_, _, ssq), _ = solved(cols, rows, p, cam, 0.1)
        assert got["status"] == OK
        mine = float(np.sum((DC.project(CAMERAS[cam], got["R"], got["t"], PC.board_points(cols, rows, tag_size=TAG_SIZE)) -
                             table["xy"].astype(np.float64).reshape(-1, 4, 2)) ** 2))
        worst = max(worst, (mine - ssq) / ssq)
        assert abs(mine / (4 * len(table)) - float(got["rms"]) ** 2) < 1e-6
    print("noisy data: relative gap to the yardstick's minimum %.3g at worst (recorded %.3g, bound 10 x)" % (worst, NOISY_MEASURED))
    assert worst <= 10.0 * NOISY_MEASURED


# ---- what the model is for ----------------------------------------------------------------------------------------------------------
def test_what_the_model_is_for():
    """A 6 x 6 board 0.2 of its extent ahead of the (-0.2, 0.59) lens with fx = 0.3 of the width, turned by 35 degrees about Y
    (board_pose_ds_cases.BEHIND): its far columns lie behind the image plane, every corner inside the valid cone by the restatement
    alone.  +-0.1 px of noise, the outer-ring tags with a corner at Zc < 0 taken out and predicted."""
    cam = DC.WIDE
    R, t = DC.behind_pose()
    Q = DC.camera_points(R, t)
    assert DC.valid(cam, Q).all()
    ring = [i for i in range(36) if i // 6 in (0, 5) or i % 6 in (0, 5)]
    miss = [i for i in ring if (Q[i, :, 2] < 0.0).any()]
    assert len(miss) >= 3 and (Q[miss][:, :, 2] < 0.0).any()
    print("behind: outer-ring tags %s have corners with Zc < 0; the farthest corner is %.1f degrees off the axis (cone %.1f)" %
          (miss, np.degrees(np.arctan2(np.hypot(Q[..., 0], Q[..., 1]), Q[..., 2])).max(), np.degrees(DC.cone_angle(cam))))
    full = DC.exact_table(6, 6, range(36), cam, R, t, noise=0.1, seed=3)
    keep = np.array([i for i in range(36) if i not in miss])
    assert (Q[keep][:, :, 2] < 0.0).any()  # and corners behind the image plane stay in the fit
    truth = DC.project(cam, R, t, PC.board_points(6, 6, tag_size=TAG_SIZE))[miss]
    kw = dict(max_err_sq=1e30, predict_missing=True)
    ds = A.board_pose(full[keep], 6, 6, cam, tag_size=TAG_SIZE, **kw)
    assert ds["status"] == OK and ds["pred"]["id"].tolist() == miss
    d = float(np.linalg.norm(ds["pred"]["xy"].reshape(-1, 4, 2) - truth, axis=-1).max())
    print("double sphere: rms %.4g px, predictions of the Zc < 0 tags %.4g px off at worst (recorded %.3g, bound 10 x)" % (ds["rms"], d, BEHIND_MEASURED))
    assert ds["rms"] < 0.2 and np.isfinite(ds["pred"]["xy"]).all() and d <= 10.0 * BEHIND_MEASURED
    Zs = (PC.board_points(6, 6, tag_size=TAG_SIZE) @ ds["R"].T + ds["t"])[miss][:, :, 2]
    assert (Zs < 0.0).any()
    equi = A.board_pose(full[keep], 6, 6, A.Camera.equidistant(*cam[:4]), tag_size=TAG_SIZE, **kw)
    if equi["status"] in (OK, LOOSE):
        got = equi["pred"]["xy"].reshape(-1, 4, 2)
        off = np.linalg.norm(got - truth, axis=-1)
        print("equidistant, zero coefficients: status %d, rms %.4g px, %d of %d predicted corners NaN, the others %.4g px off at best" %
              (equi["status"], equi["rms"], int(np.isnan(off).sum()), off.size, np.nanmin(off) if np.isfinite(off).any() else np.nan))
        assert not (np.nan_to_num(off, nan=np.inf) <= 10.0 * max(d, 0.1)).all()
    else:
        print("equidistant, zero coefficients: status %d" % equi["status"])


# ---- arguments and the contract -----------------------------------------------------------------------------------------------------
def tail_m(table, model, cam9):
    b = DC.Batch("args", [table], 6, 6, CAMERAS["neg"])
    out, t = b.empty_outputs(), b.table()
    u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    rc = _ffi.lib().agx_board_pose_tail_m(
        t[0].ctypes.data, b.tpf, b.counts[0], 0, 6, 6, 0, 0.3, TAG_SIZE, model, (C.c_double * 9)(*cam9), 4.0, 0, 1, 10, 0,
        out["pose"][0].ctypes.data, out["err_sq"][0].ctypes.data, out["row_status"][0].ctypes.data, C.cast(out["n_inliers"].ctypes.data, u32),
        C.cast(out["rms"].ctypes.data, f32), C.cast(out["best_iter"].ctypes.data, u32), out["pred"][0].ctypes.data, C.cast(out["n_pred"].ctypes.data, u32),
        C.cast(out["status"].ctypes.data, u32))
    return rc, out


def refusals(good):
    """(model, nine doubles) that every camera-taking call refuses, from a camera it takes."""
    def put(i, v):
        return good[:i] + [v] + good[i + 1:]
    out = [(DS, put(5, v)) for v in (-1e-9, 1.0 + 1e-9, np.nan)] + [(DS, put(4, v)) for v in (-1.0, 1.0 + 1e-9, np.inf)]
    out += [(DS, put(i, 5e-324)) for i in (6, 7, 8)]
    return out + [(3, good), (-1, good)]


def test_refusals():
    cam = CAMERAS["neg"]
    R, t = PC.pose("tilt40", 6, 6)
    table = DC.exact_table(6, 6, range(36), cam, R, t)
    good = PC.camera_args(cam)
    rc, out = tail_m(table, DS, good)
    assert rc == _ffi.AGX_OK and out["status"][0] == OK
    for xi, al in ((1.0, 0.0), (1.0, 1.0), (-1.0 + 1e-9, 0.5), (0.0, 1.0)):  # the closed ends of the ranges pass
        assert tail_m(table, DS, good[:4] + [xi, al, 0.0, 0.0, 0.0])[0] == _ffi.AGX_OK, (xi, al)
    sums, st = np.zeros(11), C.c_uint32(0)
    head = (table.ctypes.data, 36, 36, 0, 6, 6, 0, 0.3, TAG_SIZE)
    uv, q = np.zeros(2), np.array([0.1, 0.1, 1.0])
    for model, c9 in refusals(good):
        rc, out = tail_m(table, model, c9)
        assert rc == _ffi.AGX_ERR_ARG and all(PC.untouched(out[k]) for k in PC.KEYS), (model, c9)
        c = (C.c_double * 9)(*c9)
        assert _ffi.lib().agx_debug_board_pose_sums_m(*head, model, c, 4.0, 0, 1, 10, 0, C.byref(st), sums.ctypes.data) == _ffi.AGX_ERR_ARG
        assert _ffi.lib().agx_debug_pose_project(model, c, q.ctypes.data, 1, uv.ctypes.data) == _ffi.AGX_ERR_ARG
    assert _ffi.lib().agx_debug_board_pose_sums_m(*head, DS, (C.c_double * 9)(*good), 4.0, 0, 1, 10, 0, C.byref(st), sums.ctypes.data) == _ffi.AGX_OK
    assert st.value == OK and np.isfinite(sums[0]) and np.nanmin(sums) <= sums[0]
    with pytest.raises(A.AgxError):
        A.board_pose(table, 6, 6, A.Camera.double_sphere(320.0, 320.0, 400.0, 300.0, -0.2, 1.5))


@pytest.mark.parametrize("name", ("6x6_mild_it10_drop2_all", "6x6_full_it10_drop2_missing", "1x1"))
def test_the_m_forms_at_radtan_still_give_the_existing_forms_bytes(name):
    b, _ = PC.gpu_batches()[name]
    want = b.host()
    m = DC.Batch(name, b.tables, b.cols, b.rows, b.cam, b.tag_size, b.first_id, b.s, b.max_err_sq, b.max_drop, b.min_tags, b.iterations, b.flags,
                 b.counts, b.tag_status, b.tpf)
    got = m.host(model=EC.RADTAN)
    for k in PC.KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (name, k)


def test_the_equidistant_m_forms_answer_as_before_beside_the_new_model():
    """The equidistant batches run through the _m form with the model given and with the model taken from the camera: one answer
    (tests/test_board_pose_equi_cpu.py pins that answer's numbers)."""
    for name in ("6x6_kalibr_it10_drop2_all", "6x6_wide_it5_drop2_missing", "1x1"):
        b, status = EC.gpu_batches()[name]
        a, c = b.host(), b.host(model=EC.EQUI)
        assert a["status"][:b.n].tolist() == status
        for k in PC.KEYS:
            assert a[k].tobytes() == c[k].tobytes(), (name, k)


def test_the_abi_declares_the_third_model():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "aprilgrid_amd.h")).read()
    rust = open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(root, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"\bAGX_LENS_DOUBLE_SPHERE = 2\b", hdr) and "pub const AGX_LENS_DOUBLE_SPHERE: c_int = 2;" in rust
    for text in ("DoubleSphere = 2", "pub fn double_sphere("):
        assert text in lib_rs, text
