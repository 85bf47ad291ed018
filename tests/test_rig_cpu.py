"""agx_rig_calibrate_tail, agx_rig_seed_tail and agx_debug_rig_jacobian (csrc/rig_math.h, the host form) against the numpy / scipy
restatement of tests/rig_cases.py: its own projection of the three lens models, the Cayley update, and
scipy.optimize.least_squares over every E_c and T_s at ftol = xtol = gtol = 1e-12."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import calibrate_cases as CC
from tests import rig_cases as RC
from tests.test_calibrate_cpu import JACOBIAN_BOUND

# 10 x the largest difference tests/test_calibrate_cpu.py accepts for agx_debug_calib_param_jacobian (its equidistant bound)
RIG_JACOBIAN_BOUND = 10.0 * max(JACOBIAN_BOUND.values())
# the half field the points are placed in, degrees: the 800 x 600 frame's half width under each camera of CC.CAMERAS
FIELD = {"radtan": 45.0, "equidistant": 57.0, "double_sphere": 90.0}


@pytest.mark.parametrize("lens", RC.LENSES)
@pytest.mark.parametrize("which", ("camera0", "camera1"))
def test_jacobian_against_central_differences_of_the_numpy_model(lens, which):
    """The largest |analytic - central difference| relative to the column's largest entry (at least 1), steps of 1e-6.
    Measured: radtan 1.7e-10 / 2.9e-10 (camera 0 / camera 1), equidistant 2.2e-10 / 1.5e-10, double sphere 1.6e-10 / 4.2e-10; the
    bound is 2.5e-5."""
    cam = CC.CAMERAS[lens]
    T = RC.pose12(RC.rot(0, 12.0) @ RC.rot(1, -9.0), [0.01, -0.02, 0.5])
    E = None if which == "camera0" else RC.true_extrinsics(2)[1]
    Ev = RC.IDENT if E is None else E
    far = 0.5 * np.tan(np.radians(0.9 * FIELD[lens]))  # a board point 0.9 of the field off the axis, and one near the axis
    XY = np.array([[0.001, -0.002], [far, 0.0], [0.0, -far * 0.7], [0.03, 0.04]])
    J = A.rig_jacobian(cam, E, T, XY)
    assert np.isfinite(J).all()
    if E is None:
        assert (J[:, :, :6] == 0.0).all()
    worst, h = 0.0, 1e-6
    for k in range(12 if E is not None else 6):
        col = k if E is not None else 6 + k
        d = np.zeros(6)
        d[col % 6] = h
        if col < 6:
            hi, lo = RC.project_board(cam, RC.update(Ev, d), T, XY), RC.project_board(cam, RC.update(Ev, -d), T, XY)
        else:
            hi, lo = RC.project_board(cam, Ev, RC.update(T, d), XY), RC.project_board(cam, Ev, RC.update(T, -d), XY)
        fd = (hi - lo) / (2.0 * h)
        worst = max(worst, float(np.max(np.abs(fd - J[:, :, col])) / max(np.max(np.abs(J[:, :, col])), 1.0)))
    print(lens, which, "rig jacobian: largest relative difference", worst)
    assert worst <= RIG_JACOBIAN_BOUND
    assert np.isnan(A.rig_jacobian(cam, E, RC.pose12(np.eye(3), [0, 0, -1.0]), [[0.0, 0.0]])).all()  # no projection


def test_exact_data_recovers_the_extrinsics():
    """3 cameras (radtan, equidistant, double sphere), 8 instants, the seed 2 degrees and 5 % of the baseline off.  Measured: the
    largest reprojection error under the answer 3.2e-5 px (the corners are binary32); each E_c's distance from the truth 2.7e-9 and
    2.4e-9, against 4.1e-9 and 3.0e-8 for scipy's answer from the same seed."""
    rig = RC.three_rig()
    seed = RC.off_extrinsics(rig.E)
    r = rig.host(seed, iterations=15)
    assert r["status"] == RC.OK and r["n_instants_used"] == 8 and r["n_frames_used"] == 24 and r["n_cams_free"] == 2 and r["n_corners"] == 24 * 144
    res = rig.residuals(r["extrinsics"], r["rig_pose"])
    print("exact: largest reprojection error", np.abs(res).max(), "rms", r["rms"], "best", r["best_iter"])
    assert np.abs(res).max() <= 1e-3
    assert r["extrinsics"][0].tobytes() == RC.IDENT.tobytes()
    Es, Ts, best = RC.scipy_joint(rig, seed, rig.seed_poses(seed))  # scipy from the seed: it knows nothing of the answer
    for c in (1, 2):
        mine, theirs = RC.ext_distance(r["extrinsics"][c], rig.E[c]), RC.ext_distance(Es[c], rig.E[c])
        print("exact: camera", c, "distance from the truth", mine, "scipy's", theirs)
        assert mine <= 10.0 * theirs
    assert np.isclose(np.sum(res ** 2), r["cost"][r["best_iter"]], rtol=1e-6)


def test_noisy_data_reaches_scipys_minimum():
    """+-0.1 px: the total cost over scipy's minimum from the answer.  scipy starts from the same seed.  Measured ratio - 1: -2.5e-7 (scipy's
    own stopping rules leave it that far above); the cap is 1e-6."""
    rig = RC.three_rig(noise=0.1)
    seed = RC.off_extrinsics(rig.E)
    r = rig.host(seed, iterations=25)
    assert r["status"] == RC.OK
    _, _, best = RC.scipy_joint(rig, seed, rig.seed_poses(seed))  # scipy from the seed: it knows nothing of the answer
    cost = r["cost"][r["best_iter"]]
    print("noisy: cost", cost, "scipy", best, "ratio - 1", cost / best - 1.0, "rms", r["rms"])
    assert cost <= best * (1.0 + 1e-6)


def test_unusable_frames_and_instants_contribute_nothing():
    rig = RC.three_rig(noise=0.1).subset(instants=range(6))
    seed = RC.off_extrinsics(rig.E)
    rig.fit_status = rig.fit_status.copy()
    rig.fit_status[1, 2] = _ffi.AGX_FIT_SINGULAR      # one frame: the instant stays (2 cameras left)
    rig.fit_status[:, 4] = _ffi.AGX_FIT_FEW           # a whole instant
    rig.fit_status[0, 0] = rig.fit_status[2, 0] = _ffi.AGX_FIT_SINGULAR  # an instant with one camera left: unusable at min_cams 2
    r = rig.host(seed, iterations=6)
    assert r["status"] == RC.OK and r["n_instants_used"] == 4 and list(r["cam_n"]) == [4, 3, 4]
    assert (r["frame_n"] > 0).sum() == 11 and r["frame_n"][1, 0] == 0 and np.isnan(r["rig_pose"][[0, 4]]).all()
    keep = [1, 2, 3, 5]
    s = rig.subset(instants=keep).host(seed, iterations=6)
    assert s["extrinsics"].tobytes() == r["extrinsics"].tobytes() and s["rig_pose"].tobytes() == r["rig_pose"][keep].tobytes()
    assert s["report_raw"].tobytes() == r["report_raw"].tobytes() and s["frame_cost"].tobytes() == r["frame_cost"][:, keep].tobytes()


def test_a_camera_without_a_counted_frame_keeps_its_seed():
    rig = RC.three_rig(noise=0.1).subset(instants=range(5))
    seed = RC.off_extrinsics(rig.E)
    rig.fit_status = rig.fit_status.copy()
    rig.fit_status[2, :] = _ffi.AGX_FIT_FEW
    r = rig.host(seed, iterations=5)
    assert r["status"] == RC.OK and r["n_cams_free"] == 1 and list(r["cam_n"]) == [5, 5, 0]
    assert r["extrinsics"][2].tobytes() == seed[2].tobytes() and r["extrinsics"][1].tobytes() != seed[1].tobytes()
    two = rig.subset(cams=[0, 1]).host(seed[:2], iterations=5)  # the held camera's block is the identity: the pair alone is the same
    assert two["extrinsics"][1].tobytes() == r["extrinsics"][1].tobytes() and two["rig_pose"].tobytes() == r["rig_pose"].tobytes()


def test_min_cams_one_adds_the_single_view_instants_only():
    rig = RC.stereo_rig(noise=0.1).subset(instants=range(6))
    seed = RC.off_extrinsics(rig.E)
    rig.fit_status = rig.fit_status.copy()
    rig.fit_status[0, 3] = _ffi.AGX_FIT_SINGULAR  # instant 3 is seen by camera 1 only
    two, one = rig.host(seed, iterations=12, min_cams=2), rig.host(seed, iterations=12, min_cams=1)
    assert two["status"] == one["status"] == RC.OK and two["n_instants_used"] == 5 and one["n_instants_used"] == 6
    assert np.isnan(two["rig_pose"][3]).all() and np.isfinite(one["rig_pose"][3]).all()
    # a single-view instant is fitted by its own T_s whatever E_1 is: it adds its own cost and moves E_1 by no more than a step
    extra = float(one["frame_cost"][1, 3])
    c2, c1 = two["cost"][two["best_iter"]], one["cost"][one["best_iter"]]
    print("min_cams: cost", c2, "+", extra, "against", c1, "E_1 apart", RC.ext_distance(one["extrinsics"][1], two["extrinsics"][1]))
    assert np.isclose(c2 + extra, c1, rtol=1e-6)
    assert RC.ext_distance(one["extrinsics"][1], two["extrinsics"][1]) <= 1e-6


def test_two_groups_that_never_share_an_instant_are_singular():
    cams = [CC.CAMERAS["radtan"]] * 4
    rig = RC.Rig(cams, RC.true_extrinsics(4), CC.poses(6), missing={(c, s) for c in range(4) for s in range(6) if (c < 2) != (s < 3)})
    r = rig.host(RC.off_extrinsics(rig.E), iterations=5)
    assert r["status"] == RC.SINGULAR and r["best_iter"] == 0 and np.isfinite(r["cost"][0]) and np.isnan(r["extrinsics_raw"]).all()
    assert np.isnan(r["rig_pose_raw"]).all() and (r["frame_n_raw"] == 0xFFFFFFFF).all() and (r["cam_n_raw"] == 0xFFFFFFFF).all()


def test_few_by_each_rule():
    rig = RC.stereo_rig(noise=0.1).subset(instants=range(3))
    seed = RC.off_extrinsics(rig.E)
    r = rig.host(seed, min_instants=4)
    assert r["status"] == RC.FEW and r["n_instants_used"] == 3 and np.isnan(r["rms"]) and np.isnan(r["extrinsics_raw"]).all()
    solo = rig.subset()
    solo.fit_status = solo.fit_status.copy()
    solo.fit_status[1, :] = _ffi.AGX_FIT_FEW
    r = solo.host(seed, min_cams=1)  # camera 1 has no counted frame: no free camera
    assert r["status"] == RC.FEW and r["n_cams_free"] == 0 and r["n_instants_used"] == 3
    tiny = RC.Rig([CC.CAMERAS["radtan"]] * 2, RC.true_extrinsics(2), CC.poses(3), ids=[14])  # 6 frames of one tag: 24 corners
    r = tiny.host(seed)
    assert r["status"] != RC.FEW and r["n_corners"] == 24 and r["n_cams_free"] == 1 and r["n_instants_used"] == 3  # 24 >= 6 + 18
    r = tiny.subset(instants=[0, 1]).host(seed)
    assert r["n_corners"] == 16 and r["status"] == RC.FEW  # 16 < 6 + 12


def test_a_cost_that_rises_keeps_the_best_iterate():
    """RC.RISES_THEN_LEAVES (a seed 60 degrees and 5 baselines off, undamped): cost 4.9e10, 2.7e8, then a corner without a
    projection (+inf): the answer is iterate 1 of the 2 that ran.  RC.RISES_FINITE (the same seed at damping 1e-3): cost 4.9e10,
    6.9e28, then falling to 6.4e19 at iterate 12, never below iterate 0: the answer is the inputs."""
    rig = RC.stereo_rig(noise=0.1)
    seed = RC.off_extrinsics(rig.E, **RC.RISES_SEED)
    r = rig.host(seed, iterations=12, **RC.RISES_THEN_LEAVES)
    c = r["cost"][:r["iterations_run"] + 1]
    print("rises then leaves: cost", c)
    assert r["status"] == RC.OK and r["iterations_run"] == 2 and r["best_iter"] == 1 and np.isposinf(c[2]) and c[1] < c[0] and np.isnan(r["cost"][3:]).all()
    at = rig.host(seed, iterations=1, **RC.RISES_THEN_LEAVES)  # the answer is iterate 1's bytes, not the last iterate's
    assert at["best_iter"] == 1
    for k in ("extrinsics", "rig_pose", "frame_cost", "frame_n"):
        assert r[k].tobytes() == at[k].tobytes(), k
    assert r["extrinsics"][1].tobytes() != seed[1].tobytes()
    r = rig.host(seed, iterations=12, **RC.RISES_FINITE)
    c = r["cost"][:13]
    print("rises, finite: cost", c)
    assert r["status"] == RC.OK and r["iterations_run"] == 12 and np.isfinite(c).all() and c[1] > 1e6 * c[0] and (c[1:] > 1e6 * c[0]).all()
    assert r["best_iter"] == 0 == int(np.argmin(c))
    at = rig.host(seed, iterations=0, **RC.RISES_FINITE)
    for k in ("extrinsics", "rig_pose", "frame_cost", "frame_n"):
        assert r[k].tobytes() == at[k].tobytes(), k
    assert r["extrinsics"][1].tobytes() == seed[1].tobytes() and r["rig_pose"].tobytes() == rig.seed_poses(seed).tobytes()


def test_zero_iterations_and_aliasing():
    rig = RC.stereo_rig(noise=0.1)
    seed = RC.off_extrinsics(rig.E, deg=25.0, frac=2.0)
    zero = rig.host(seed, iterations=0)
    assert zero["status"] == RC.OK and zero["best_iter"] == 0 and np.isnan(zero["cost"][1:]).all()
    assert zero["extrinsics"][1].tobytes() == seed[1].tobytes() and zero["rig_pose"].tobytes() == rig.seed_poses(seed).tobytes()
    good = RC.off_extrinsics(rig.E)
    a = rig.host(good, iterations=7)
    b = rig.host(good.copy(), iterations=7, in_place=True)
    assert a["extrinsics"].tobytes() == b["extrinsics"].tobytes() and a["report_raw"].tobytes() == b["report_raw"].tobytes()
    with pytest.raises(A.AgxError):
        bad = good.copy()
        bad[1, 3] = np.inf
        rig.host(bad)


def chain_poses():
    """3 cameras, 4 instants: cameras 0 and 1 share instants 0 and 1, cameras 1 and 2 share instants 2 and 3; 2 never sees 0's"""
    E, T = RC.true_extrinsics(3), CC.poses(4)
    pose = np.array([[RC.compose(E[c], T[s]) for s in range(4)] for c in range(3)])
    fst = np.full((3, 4), _ffi.AGX_FIT_FEW, np.uint32)
    fst[0, :2] = fst[1, :] = fst[2, 2:] = _ffi.AGX_FIT_OK
    return E, pose, fst


def test_seed_chain_ties_and_a_detached_camera():
    E, pose, fst = chain_poses()
    s = A.rig_seed(pose, fst)
    assert list(s["cam_status"]) == [0, 0, 0] and s["extrinsics"][0].tobytes() == RC.IDENT.tobytes()
    for c in (1, 2):
        assert RC.ext_distance(s["extrinsics"][c], E[c]) < 1e-12
    # ties: the lowest shared instant without counts, the one with the most correspondences with them
    moved = pose.copy()
    moved[1, 1] = RC.compose(RC.pose12(RC.rot(0, 1.0), [0.01, 0, 0]), pose[1, 1])  # instant 1 disagrees with instant 0 about E_1
    first = A.rig_seed(moved, fst)["extrinsics"][1]
    assert RC.ext_distance(first, E[1]) < 1e-12
    n = np.full((3, 4), 10, np.uint32)
    n[1, 1] = 30
    second = A.rig_seed(moved, fst, n)["extrinsics"][1]
    assert RC.ext_distance(second, RC.compose(moved[1, 1], RC.inverse(moved[0, 1]))) < 1e-12 and RC.ext_distance(second, E[1]) > 1e-3
    n[1, 0] = 30  # equal again: the lowest instant
    assert A.rig_seed(moved, fst, n)["extrinsics"][1].tobytes() == first.tobytes()
    fst[2, :] = _ffi.AGX_FIT_FEW
    d = A.rig_seed(pose, fst)
    assert list(d["cam_status"]) == [0, 0, _ffi.AGX_RIG_CAM_DETACHED] and d["extrinsics"][2].tobytes() == RC.IDENT.tobytes()


def test_what_it_is_for():
    """A stereo pair with a 0.1-unit baseline, 12 instants, +-0.1 px: the baseline's error of the joint estimate against the
    seed's single-instant composition and the mean of the per-instant compositions.  Printed, not gated; measured: joint 6.4e-6,
    the seed's instant 8.4e-5, the mean of 12 compositions 2.4e-8 (on this draw the mean lands closer)."""
    rig = RC.stereo_rig(noise=0.1, n=12)
    seed = A.rig_seed(rig.pose, rig.fit_status, rig.counts)["extrinsics"]
    r = rig.host(seed, iterations=10)
    per = np.array([RC.compose(rig.pose[1, s], RC.inverse(rig.pose[0, s]))[9:] for s in range(12)])
    base = np.linalg.norm(rig.E[1, 9:])
    err = lambda t: abs(np.linalg.norm(t) - base)
    print("baseline error: joint", err(r["extrinsics"][1, 9:]), "seed (one instant)", err(seed[1, 9:]), "mean of per-instant", err(per.mean(axis=0)))
    assert r["status"] == RC.OK and r["cost"][r["best_iter"]] <= r["cost"][0]
