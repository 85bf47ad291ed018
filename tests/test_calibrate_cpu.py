"""agx_calibrate_tail, agx_calibrate_seed_tail and agx_debug_calib_param_jacobian (csrc/calib_math.h, the host form) against
numpy / scipy restatements written here and in tests/calibrate_cases.py.  Every bound is 10 x a figure measured on this code and
written beside it (the project's standing rule: tests/test_board_pose_equi_cpu.py's step test is the model)."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import board_pose_cases as PC
from tests import calibrate_cases as CC
from tests.board_pose_equi_cases import library_project

LENSES = ("radtan", "equidistant", "double_sphere")


def jacobian_points(lens):
    rng = np.random.RandomState(11)
    Q = np.column_stack([rng.uniform(-0.6, 0.6, 40), rng.uniform(-0.5, 0.5, 40), rng.uniform(0.4, 1.2, 40)])
    if lens == "equidistant":  # both sides of POSE_EQUI_SMALL_R2 = 2^-13 (r = 0.011), and the axis
        r = np.sqrt(2.0 ** -13)
        Q = np.vstack([Q, [[0.0, 0.0, 1.0], [r * 0.999, 0.0, 1.0], [r * 1.001, 0.0, 1.0], [0.003, -0.004, 1.0], [0.02, 0.01, 1.0]]])
    if lens == "double_sphere":  # Zc < 0 inside the cone (w2 = 0.79 for xi = -0.2, alpha = 0.55)
        Q = np.vstack([Q, [[1.0, 0.2, -0.05], [-0.8, 0.9, -0.3], [0.5, -1.0, -0.5], [1.0, 1.0, 0.0]]])
    return Q


# the largest |analytic - central difference| relative to the column's largest entry, measured: radtan 5.7e-9, equidistant
# 2.5e-7 (k4 = 0.0026: its step of 2.6e-9 leaves the difference quotient few digits), double sphere 1.1e-9 (steps of 1e-6
# relative, 1e-6 absolute for a zero entry)
JACOBIAN_BOUND = {"radtan": 5.7e-8, "equidistant": 2.5e-6, "double_sphere": 1.1e-8}


@pytest.mark.parametrize("lens", LENSES)
def test_parameter_jacobian_against_central_differences(lens):
    cam, Q = CC.CAMERAS[lens], jacobian_points(lens)
    if lens == "radtan":
        cam = A.Camera(380.0, 420.0, 410.0, 290.0, -0.25, 0.08, 0.01, -0.008, -0.015)
    J = A.calib_param_jacobian(cam, Q)
    assert np.isfinite(J).all()
    held = {"radtan": [], "equidistant": [8], "double_sphere": [6, 7, 8]}[lens]
    worst = 0.0
    for i in range(9):
        if i in held:
            assert (J[:, :, i] == 0.0).all()
            continue
        h = abs(cam[i]) * 1e-6 if cam[i] != 0.0 else 1e-6
        lo, hi = list(cam), list(cam)
        lo[i] -= h
        hi[i] += h
        fd = (library_project(CC.make_camera(cam, hi), Q) - library_project(CC.make_camera(cam, lo), Q)) / (2.0 * h)
        worst = max(worst, float(np.max(np.abs(fd - J[:, :, i])) / max(np.max(np.abs(J[:, :, i])), 1.0)))
    print(lens, "jacobian: largest relative difference", worst)
    assert worst <= JACOBIAN_BOUND[lens]
    assert np.isnan(A.calib_param_jacobian(cam, [[0.0, 0.0, -1.0]])).all()  # no projection


# exact tables of 8 poses; seeds: focal lengths 5 % off, principal point 10 px off, zero distortion (CC.off_seed), per lens.  The
# double sphere's zero distortion is xi = 0 (alpha = 0.5), where the undamped system of iterate 0 is AGX_CALIB_SINGULAR
# (test_statuses) and from where undamped steps would diverge (CC.DS_DIVERGES): that case runs at damping 1e-6, the driver's default
# under this lens, and 64 iterations (the damped steps close in on the flat fx / xi / alpha valley slowly).  "double_sphere_far" is
# an additional case: undamped from xi = -0.5, alpha = 0.9, focal lengths 30 % off.
# Measured: the largest |camera - truth| relative to max(|truth|, 1): radtan 5.1e-8, equidistant 5.5e-6, double sphere 4.3e-8,
# double_sphere_far 4.3e-8 (the corners are binary32: the RMS at the answer is 1.3e-5 px); the final cost over scipy's from the
# answer: ratio - 1 = -1.2e-10, 2.8e-11, -2.6e-12, 3.9e-11.
CASES = {"radtan": ("radtan", 0.0, 20), "equidistant": ("equidistant", 0.0, 20), "double_sphere": ("double_sphere", 1e-6, 64),
         "double_sphere_far": ("double_sphere", 0.0, 20)}
EXACT_CAMERA_BOUND = {"radtan": 5.1e-7, "equidistant": 5.5e-5, "double_sphere": 4.3e-7, "double_sphere_far": 4.3e-7}
EXACT_COST_MARGIN = 3.9e-10
LENS_HELD = {"radtan": 0, "equidistant": 0x100, "double_sphere": 0x1c0}


def exact_seed(case):
    cam = CC.CAMERAS[CASES[case][0]]
    if case == "double_sphere_far":
        return A.Camera.double_sphere(cam[0] * 0.7, cam[1] * 0.7, 410.0, 290.0, -0.5, 0.9)
    return CC.off_seed(cam)


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_data_recovers_the_camera_and_scipys_optimum(case):
    lens, damping, iterations = CASES[case]
    cam = CC.CAMERAS[lens]
    b = CC.Batch([CC.table(cam, p) for p in CC.poses(8)], exact_seed(case))
    r = b.host(fixed=CC.FIXED[lens], iterations=iterations, damping=damping)
    assert r["status"] == CC.OK and r["n_frames_used"] == 8 and r["n_corners"] == 8 * 144
    err = float(np.max(np.abs(np.array(r["camera"]) - np.array(cam)) / np.maximum(np.abs(np.array(cam)), 1.0)))
    _, _, best = CC.scipy_joint(b, r["camera"], r["pose"], CC.FIXED[lens] | LENS_HELD[lens])
    cost = r["cost"][r["best_iter"]]
    print(case, "exact: camera error", err, "cost", cost, "scipy", best, "ratio - 1", cost / best - 1.0, "rms", r["rms"])
    assert err <= EXACT_CAMERA_BOUND[case]
    assert cost <= best * (1.0 + EXACT_COST_MARGIN)
    assert np.isclose(np.sum(b.residuals(r["camera"], r["pose"]) ** 2), cost, rtol=1e-9)


# +-0.1 px of uniform noise, fixed seed, the same seeds and damping: the cost over scipy's minimum from the
# answer, measured ratio - 1: radtan 6.9e-15, equidistant -1.1e-16, double sphere -3.1e-15, double_sphere_far 2.2e-14 (the
# rounding of a sum of 2304 squares); 10 x the largest, for all
NOISY_MARGIN = 2.2e-13


@pytest.mark.parametrize("case", sorted(CASES))
def test_noisy_data_reaches_scipys_minimum(case):
    lens, damping, iterations = CASES[case]
    cam = CC.CAMERAS[lens]
    b = CC.Batch([CC.table(cam, p, noise=0.1, seed=k + 1) for k, p in enumerate(CC.poses(8))], exact_seed(case))
    r = b.host(fixed=CC.FIXED[lens], iterations=max(iterations, 25), damping=damping)
    assert r["status"] == CC.OK
    _, _, best = CC.scipy_joint(b, r["camera"], r["pose"], CC.FIXED[lens] | LENS_HELD[lens])
    cost = r["cost"][r["best_iter"]]
    print(case, "noisy: cost", cost, "scipy", best, "ratio - 1", cost / best - 1.0, "rms", r["rms"])
    assert cost <= best * (1.0 + NOISY_MARGIN)


# seed + 3 rounds by the host forms (TagDetector.calibrate_batch's stages and defaults) on +-0.1 px tables, per lens: the RMS from
# the seed camera's poses down to the floor.  Measured: radtan 3.04 -> 0.0802 px (0.0804 at the true camera), equidistant 1.33 ->
# 0.0802 (0.0804), double sphere 0.918 -> 0.0807 (0.0804: three rounds of damped steps are still on their way down the valley).
# The assertion is test_what_it_is_for's: below twice the RMS at the true camera.
@pytest.mark.parametrize("lens", LENSES)
def test_host_composition_for_every_lens(lens):
    cam = CC.CAMERAS[lens]
    tabs = [CC.table(cam, p, noise=0.1, seed=k + 1) for k, p in enumerate(CC.poses(8))]
    got, pose, rep = CC.host_rounds(tabs, 6, 6, CC.SIZE, fixed=CC.FIXED[lens], lens=lens, cap=36)
    truth = CC.Batch(tabs, cam).host(fixed=0x1ff, iterations=5)
    print(lens, "seed + 3 rounds: rms", rep["rms"], "from", rep["first_rms"], "at the true camera", truth["rms"])
    assert rep["status"] == CC.OK and got.model == cam.model and rep["n_frames_used"] == 8
    assert rep["rms"] < 2.0 * truth["rms"] < rep["first_rms"]


def test_masks_and_zero_iterations():
    b = CC.exact_batch("radtan", noise=0.1)
    seed = b.seed
    r = b.host(fixed=0x10c, iterations=8)  # cx, cy, k3 held
    out = np.array(r["camera"])
    assert r["status"] == CC.OK and r["best_iter"] > 0
    for i in (2, 3, 8):
        assert out[i].tobytes() == np.float64(seed[i]).tobytes()
    assert out[0] != seed[0] and out[4] != 0.0
    held = A.calibrate(b.tags, b.counts, 6, 6, A.Camera(*[-0.0 if v == 0.0 else v for v in seed]), b.pose, b.row_status, b.fit_status,
                       tag_size=CC.TAG_SIZE, fixed=["k1", "k2", "p1", "p2", "k3"], iterations=3)
    assert np.signbit(np.array(held["camera"])[4:]).all()  # a held -0.0 keeps its bits
    every = b.host(fixed=0x1ff, iterations=6)  # poses only
    c = every["cost"][:every["iterations_run"] + 1]
    assert every["status"] == CC.OK and np.array(every["camera"]).tobytes() == np.array(seed, np.float64).tobytes()
    assert every["cost"][every["best_iter"]] <= c[0] and every["best_iter"] == int(np.argmin(c))
    zero = b.host(iterations=0)
    assert zero["status"] == CC.OK and zero["best_iter"] == 0 and zero["iterations_run"] == 0
    assert np.array(zero["camera"]).tobytes() == np.array(seed, np.float64).tobytes() and zero["pose"].tobytes() == b.pose.tobytes()
    assert np.isnan(zero["cost"][1:]).all()
    # cost[0] is the sum of pose_row_residual's sums: the frames' rms of the pose call, squared, times their corners
    assert np.isclose(zero["cost"][0], np.sum(b.residuals(seed, b.pose) ** 2), rtol=1e-12)
    assert np.allclose(zero["frame_cost"].sum(), zero["cost"][0], rtol=1e-6) and (zero["frame_n"] == 144).all()


def test_best_iterate():
    cam = CC.CAMERAS["radtan"]
    b = CC.Batch([CC.table(cam, p) for p in CC.poses(8)], CC.RT_RISES)
    r = b.host(iterations=12, fixed=0x100)
    c = r["cost"][:13]
    assert r["status"] == CC.OK and np.any(np.diff(c) > 0) and r["best_iter"] == int(np.argmin(c)) and r["iterations_run"] == 12
    short = b.host(iterations=2, fixed=0x100)  # both steps raise the cost: the answer is the inputs
    assert short["best_iter"] == 0 and np.array(short["camera"]).tobytes() == np.array(CC.RT_RISES, np.float64).tobytes()
    assert short["pose"].tobytes() == b.pose.tobytes()
    cam = CC.CAMERAS["double_sphere"]
    tabs = [CC.table(cam, p) for p in CC.poses(8)]
    r = CC.Batch(tabs, CC.DS_ALPHA_LEAVES).host(iterations=12)
    assert r["status"] == CC.OK and r["best_iter"] == 0 and r["iterations_run"] == 1 and np.isposinf(r["cost"][1]) and np.isnan(r["cost"][2:]).all()
    assert np.array(r["camera"]).tobytes() == np.array(CC.DS_ALPHA_LEAVES, np.float64).tobytes()
    r = CC.Batch(tabs, CC.DS_DIVERGES).host(iterations=12)
    assert r["status"] == CC.OK and r["best_iter"] == 0 and np.isposinf(r["cost"][r["iterations_run"]])


def test_statuses():
    b = CC.exact_batch("radtan", noise=0.1)
    one = b.subset([0])
    assert one.host(min_frames=3, fixed=0x1f0)["status"] == CC.FEW
    few = CC.few_batch().host(fixed=0x100)
    assert few["status"] == CC.FEW and few["n_corners"] == 12 and few["n_frames_used"] == 3 and np.isnan(few["rms"])
    assert np.isnan(few["camera_raw"]).all() and (few["frame_n_raw"] == 0xFFFFFFFF).all()
    sing = CC.fronto_batch().host(fixed=0x1fc, iterations=5)  # fx, fy and the poses free
    assert sing["status"] == CC.SINGULAR and sing["best_iter"] == 0 and np.isnan(sing["camera_raw"]).all() and np.isfinite(sing["cost"][0])
    assert CC.fronto_batch().host(fixed=0x1ff, iterations=5)["status"] == CC.OK  # (the poses alone are determined)
    # frames with a refused pose or too few inliers contribute nothing: without them the same bytes
    mixed = b.subset([0, 1, 2, 3, 4, 5])
    mixed.fit_status[1] = _ffi.AGX_FIT_SINGULAR
    mixed.fit_status[4] = _ffi.AGX_FIT_LOOSE
    mixed.row_status[5, 3:] = _ffi.AGX_FIT_ROW_OUTLIER
    r = mixed.host(fixed=0x100, iterations=6, min_tags=4)
    keep = [0, 2, 3]
    s = mixed.subset(keep).host(fixed=0x100, iterations=6, min_tags=4)
    assert list(r["frame_n"]) == [144, 0, 144, 144, 0, 0] and r["n_frames_used"] == 3
    assert np.array(r["camera"]).tobytes() == np.array(s["camera"]).tobytes() and r["pose"][keep].tobytes() == s["pose"].tobytes()
    assert r["report_raw"].tobytes() == s["report_raw"].tobytes() and r["pose"][[1, 4, 5]].tobytes() == mixed.pose[[1, 4, 5]].tobytes()
    assert mixed.host(fixed=0x100, iterations=1, min_tags=4, accept_loose=True)["n_frames_used"] == 4


# exact pinhole tables: |fx - 400| and |fy - 400| of the seed, measured 3.5e-6 (the binary32 corners)
SEED_BOUND = 3.5e-5


def test_seed():
    cam = A.Camera(400.0, 400.0, 399.5, 299.5)
    fits = [A.board_fit(CC.table(cam, p), 6, 6, CC.SIZE) for p in CC.poses(8)]
    s = A.calibrate_seed([f["H"] for f in fits], [f["status"] for f in fits], CC.SIZE)
    err = max(abs(s["camera"].fx - 400.0), abs(s["camera"].fy - 400.0))
    print("seed: error", err, s["camera"])
    assert s["status"] == CC.OK and err <= SEED_BOUND and tuple(s["camera"])[2:] == (399.5, 299.5, 0.0, 0.0, 0.0, 0.0, 0.0)
    fb = CC.fronto_batch()
    fits = [A.board_fit(fb.tags[f, :36], 6, 6, CC.SIZE) for f in range(fb.n)]
    assert A.calibrate_seed([f["H"] for f in fits], [f["status"] for f in fits], CC.SIZE)["status"] == CC.SINGULAR
    assert A.calibrate_seed(np.zeros((2, 9)), [_ffi.AGX_FIT_FEW, _ffi.AGX_FIT_SINGULAR], CC.SIZE)["status"] == CC.FEW


def test_what_it_is_for():
    """The strong-barrel camera (k1 = -0.3, k2 = 0.1 on a 90 degree lens), +-0.1 px of noise: calibrate_seed and 3 rounds bring the
    RMS from the zero-distortion pose's 3.04 px (rep["first_rms"]) down to 0.0802 px; at the true camera the same tables
    give 0.0804 px (the 8 + 48 fitted unknowns take their share of the noise)."""
    cam = CC.CAMERAS["radtan"]
    tabs = [CC.table(cam, p, noise=0.1, seed=k + 1) for k, p in enumerate(CC.poses(8))]
    got, pose, rep = CC.host_rounds(tabs, 6, 6, CC.SIZE, fixed=0x100, cap=36)
    truth = CC.Batch(tabs, cam).host(fixed=0x1ff, iterations=5)
    print("seed + 3 rounds: rms", rep["rms"], "from", rep["first_rms"], "at the true camera", truth["rms"], np.array(got))
    assert rep["status"] == CC.OK and rep["rms"] < 2.0 * truth["rms"] < rep["first_rms"]
