"""agx_board_pose_tail, the host form of k_board_pose (tests/test_gpu_board_pose.py holds the kernel to its bytes), against a
yardstick written independently of csrc/board_pose_math.h: numpy float64 projection and scipy.optimize.least_squares over a
rotation vector and t, started from the ground truth (tests/board_pose_cases.py).

Measured on the cases below (printed by the tests before they assert):
  exact data   the largest corner distance between the host form's reprojection and the yardstick's: 2.55e-5 px over 60 cases
               (2 layouts x 5 poses x 6 cameras, three of them with k3, strong tangential terms and all nine numbers live; the
               corners are rounded to binary32, 3e-5 px at 800 px, and the minimum is flat at that level), so the bound is 10 x
               that, 2.55e-4 px (the ceiling is 1e-3 px); the worst of the three live cameras alone is 1.11e-5 px;
  noisy data   +-0.1 px: the host form's sum of |e|^2 exceeds the yardstick's minimum by at most 1.75e-9 relative (bound 1e-6);
  step         one Gauss-Newton step from the seed against the step of a central-difference Jacobian (cameras full, k3, barrel x
               poses tilt40, near): the reference at h = 1e-5 against itself at h / 2 differs by 5.6e-8 px at worst, so the bound
               is 10 x that, 5.6e-7 px (the ceiling is 1e-3 px); the library's iterate 1 lies 1.4e-12 .. 7.4e-8 px from the
               reference's, after steps that move the corners 0.016 .. 87 px;
  scale        tag_size 1e-3 and 1e3 against 0.05 on the same pixels: R differs by 1.7e-15 at most, t / tag_size by 2.0e-11
               relative, rms and all 288 predicted values by 0 ulp; the pose's doubles are not bit-equal;
  barrel       board_fit's rms over the whole board 21.3 px, its predictions of the 20 tags of the outermost ring (taken out
               four at a time) 10.7 .. 199.7 px off; board_pose's rms 0.077 .. 0.079 px, its predictions 0.127 px off at most;
  rendered     board_fit / board_pose rms on the three rendered frames: 0.0294 / 0.0294, 0.0368 / 0.0368, 0.0445 / 0.0445 px;
  warped frame recovery of four outer-ring tags on the barrel-warped 6 x 6 frame: 2 of 4 through board_fit, 4 of 4 through board_pose.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from tests import board_fit_cases as BC
from tests import board_pose_cases as PC
from tests.board_pose_cases import CAMERAS, FEW, INPUT, LAYOUTS, LOOSE, OK, POSES, SINGULAR, TAG_SIZE

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

EXACT_MEASURED = 2.55e-5  # px: see the module's docstring
EXACT_BOUND = min(10.0 * EXACT_MEASURED, 1e-3)
CASES = [(c, r, p, k) for c, r in LAYOUTS for p in sorted(POSES) for k in sorted(CAMERAS)]
LIVE = ("full", "k3", "tangential")  # the cameras whose k3 and tangential products are not products with 0 or 1e-3


@functools.lru_cache(maxsize=None)
def solved(cols, rows, p, cam, noise):
    """One case -> (table, the host form's answer, the yardstick's (R, t, sum), ground truth (R, t))."""
    R, t = PC.pose(p, cols, rows)
    table = PC.exact_table(cols, rows, range(cols * rows), CAMERAS[cam], R, t, noise=noise, seed=11)
    got = A.board_pose(table, cols, rows, CAMERAS[cam], tag_size=TAG_SIZE)
    return table, got, PC.yardstick(table, cols, rows, CAMERAS[cam], R, t), (R, t)


def is_rotation(R):
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14


def test_exact_data_reprojects_like_the_yardstick():
    worst = worst_live = 0.0
    for cols, rows, p, cam in CASES:
        table, got, (Ry, ty, _), (R, t) = solved(cols, rows, p, cam, 0.0)
        assert got["status"] == OK, (cols, rows, p, cam)
        P = PC.board_points(cols, rows, tag_size=TAG_SIZE)
        d = np.linalg.norm(PC.project(CAMERAS[cam], got["R"], got["t"], P) - PC.project(CAMERAS[cam], Ry, ty, P), axis=-1).max()
        worst = max(worst, d)
        if cam in LIVE:
            worst_live = max(worst_live, d)
        is_rotation(got["R"])
        assert np.abs(got["R"] - R).max() < 1e-4 and np.abs(got["t"] - t).max() < 1e-4 * PC.extent(cols, rows), (p, cam)
        # the predicted rows are the pose's reprojection rounded to binary32
        assert np.abs(got["pred"]["xy"].reshape(-1, 4, 2) - PC.project(CAMERAS[cam], got["R"], got["t"], P)).max() < 1e-4
    print("exact data: largest corner distance to the yardstick %.3g px over %d cases (bound %.3g); under %s alone %.3g px"
          % (worst, len(CASES), EXACT_BOUND, ", ".join(LIVE), worst_live))
    assert worst <= EXACT_BOUND


def test_noisy_data_reaches_the_yardsticks_minimum():
    worst = -1.0
    for cols, rows, p, cam in CASES:
        table, got, (_, _, ssq), _ = solved(cols, rows, p, cam, 0.1)
        assert got["status"] == OK
        mine = float(np.sum((PC.project(CAMERAS[cam], got["R"], got["t"], PC.board_points(cols, rows, tag_size=TAG_SIZE)) -
                             table["xy"].astype(np.float64).reshape(-1, 4, 2)) ** 2))
        worst = max(worst, (mine - ssq) / ssq)
        assert abs(mine / (4 * len(table)) - float(got["rms"]) ** 2) < 1e-6  # rms is the root mean square of the same residuals
        is_rotation(got["R"])
    print("noisy data: largest relative gap of the sum of |e|^2 to the yardstick's minimum %.3g (bound 1e-6)" % worst)
    assert worst <= 1e-6


def test_the_ninth_double_of_the_camera_is_read():
    """k3 on the whole way Python -> C ABI -> the host form: the predicted rows under camera "k3" are the numpy projection with
    k3, and far from the projection without it."""
    cam = CAMERAS["k3"]
    table, got, _, _ = solved(6, 6, "tilt40", "k3", 0.0)
    assert got["status"] == OK and cam.k3 == -0.02 and len(got["pred"]) == 36
    P = PC.board_points(6, 6, tag_size=TAG_SIZE)
    pred = got["pred"]["xy"].reshape(36, 4, 2).astype(np.float64)
    with_k3 = np.linalg.norm(pred - PC.project(cam, got["R"], got["t"], P), axis=-1).max()
    without = np.linalg.norm(pred - PC.project(cam._replace(k3=0.0), got["R"], got["t"], P), axis=-1).max()
    print("k3: pred against the projection with k3 %.3g px, with k3 = 0 %.3g px" % (with_k3, without))
    assert with_k3 < 1e-4 and without > 10.0


# ---- one Gauss-Newton step against a step from a finite-difference Jacobian ---------------------------------------------------------
STEP_H = 1e-5  # the difference step: radians for w, tag sides for dt
# The ABI carries spacing_ratio as binary32: at 0.3 the library's board is the one of 0.300000012, whose corners lie up to 2e-5 px
# from the board of the binary64 0.3 -- two hundred times the reference's own error, so the reference takes the ratio the library gets.
STEP_S = float(np.float32(0.3))
STEP_SELF_MEASURED = 5.6e-8  # px: see the module's docstring
STEP_BOUND = min(10.0 * STEP_SELF_MEASURED, 1e-3)
STEP_CASES = [(cam, p) for cam in ("full", "k3", "barrel") for p in ("tilt40", "near")]
STEP_NOISE_SEED = 11


def cayley(w):
    """C(w) = (I - [w/2]x)^-1 (I + [w/2]x)."""
    a = np.asarray(w, np.float64) / 2.0
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.linalg.solve(np.eye(3) - K, np.eye(3) + K)


def reference_step(cam, R0, t0, P, obs, h):
    """Iterate 1 of Gauss-Newton from (R0, t0) in numpy float64: the Jacobian of the projection by (w, dt) from central
    differences of step h (h * TAG_SIZE for dt), the step from lstsq, R orthonormalised (its nearest rotation, by SVD)."""
    def f(d):
        return PC.project(cam, R0 @ cayley(d[:3]), t0 + d[3:], P).ravel()

    J = np.empty((obs.size, 6))
    for i in range(6):
        d = np.zeros(6)
        d[i] = h if i < 3 else h * TAG_SIZE
        J[:, i] = (f(d) - f(-d)) / (2.0 * d[i])
    step = np.linalg.lstsq(J, obs.ravel() - f(np.zeros(6)), rcond=None)[0]
    U, _, Vt = np.linalg.svd(R0 @ cayley(step[:3]))
    return U @ Vt, t0 + step[3:]


@functools.lru_cache(maxsize=None)
def stepped(cam, p):
    """-> (distance of the library's iterate 1 to the reference's, distance of the reference at STEP_H to itself at STEP_H / 2),
    both the largest distance in px between the two poses' projections of the board's 144 corners."""
    c = CAMERAS[cam]
    R, t = PC.pose(p, 6, 6)
    table = PC.exact_table(6, 6, range(36), c, R, t, s=STEP_S, noise=0.1, seed=STEP_NOISE_SEED)
    seed = A.board_pose(table, 6, 6, c, tag_size=TAG_SIZE, spacing_ratio=STEP_S, iterations=0, max_err_sq=1e30)
    got = A.board_pose(table, 6, 6, c, tag_size=TAG_SIZE, spacing_ratio=STEP_S, iterations=1, max_err_sq=1e30)
    assert seed["status"] == OK and seed["best_iter"] == 0 and got["status"] == OK
    assert got["best_iter"] == 1, (cam, p)  # (holds for all six cases at noise seed STEP_NOISE_SEED)
    P = PC.board_points(6, 6, STEP_S, TAG_SIZE)
    obs = table["xy"].astype(np.float64).reshape(36, 4, 2)
    uv = [PC.project(c, Rr, tr, P) for Rr, tr in (reference_step(c, seed["R"], seed["t"], P, obs, STEP_H),
                                                  reference_step(c, seed["R"], seed["t"], P, obs, STEP_H / 2.0))]
    mine = PC.project(c, got["R"], got["t"], P)
    moved = np.linalg.norm(mine - PC.project(c, seed["R"], seed["t"], P), axis=-1).max()
    assert moved > 0.01, (cam, p, moved)  # the step is there to be compared: the seed is not the minimum
    return np.linalg.norm(mine - uv[0], axis=-1).max(), np.linalg.norm(uv[0] - uv[1], axis=-1).max(), moved


def test_the_finite_difference_reference_agrees_with_itself_as_measured():
    worst = max(stepped(cam, p)[1] for cam, p in STEP_CASES)
    print("step: the finite-difference reference at h = %g against h / 2: %.3g px at worst (recorded %.3g, bound 10 x = %.3g px)"
          % (STEP_H, worst, STEP_SELF_MEASURED, STEP_BOUND))
    assert worst <= STEP_SELF_MEASURED


@pytest.mark.parametrize("cam,p", STEP_CASES)
def test_one_gauss_newton_step_is_the_finite_difference_step(cam, p):
    """The analytic Jacobian of pose_accumulate, compared step for step and not through convergence: iterate 1 from the seed
    (iterations = 0 returns it) against the step of a Jacobian taken by central differences of the numpy projection."""
    d, self_d, moved = stepped(cam, p)
    print("step %s / %s: the library's iterate 1 is %.3g px from the reference's (the step moved the corners %.3g px; bound %.3g px)"
          % (cam, p, d, moved, STEP_BOUND))
    assert d <= STEP_BOUND


@pytest.mark.parametrize("s", (0.0, -0.5, 1.0))
def test_spacing_ratios_with_an_id_window_that_passes_2_to_the_32(s):
    """Camera "full", the 40 degree tilt, the 6 x 6 layout from 0xFFFFFFF0 (its ids run through 0xFFFFFFFF to 19) at the spacing
    ratios 0, -0.5 and 1, t scaled with the board's extent at that ratio: pitch, bx, by, sb, the seed's q and the wrapping id
    arithmetic, against the yardstick on exact data under the exact-data bound."""
    cam, first = CAMERAS["full"], PC.WRAP_FIRST_ID
    R, t = PC.pose("tilt40", 6, 6, s=s)
    assert np.allclose(t, np.array(POSES["tilt40"][1]) * PC.extent(6, 6, s))
    table = PC.exact_table(6, 6, range(36), cam, R, t, first_id=first, s=s)
    layout = [(first + k) % (1 << 32) for k in range(36)]
    assert table["id"].tolist() == layout and layout[15:17] == [0xFFFFFFFF, 0]
    got = A.board_pose(table, 6, 6, cam, tag_size=TAG_SIZE, first_id=first, spacing_ratio=s)
    Ry, ty, _ = PC.yardstick(table, 6, 6, cam, R, t, first_id=first, s=s)
    P = PC.board_points(6, 6, s, TAG_SIZE)
    d = np.linalg.norm(PC.project(cam, got["R"], got["t"], P) - PC.project(cam, Ry, ty, P), axis=-1).max()
    print("spacing %g, first_id 0x%X: largest corner distance to the yardstick %.3g px (bound %.3g)" % (s, first, d, EXACT_BOUND))
    assert got["status"] == OK and got["n_inliers"] == 36 and d <= EXACT_BOUND
    is_rotation(got["R"])
    assert np.abs(got["R"] - R).max() < 1e-4 and np.abs(got["t"] - t).max() < 1e-4 * PC.extent(6, 6, s)
    # the ids survive the Python wrapper as unsigned values, in layout order; the rows are the pose's reprojection
    assert got["pred"]["id"].dtype == np.uint32 and got["pred"]["id"].tolist() == layout
    assert np.abs(got["pred"]["xy"].reshape(-1, 4, 2) - PC.project(cam, got["R"], got["t"], P)).max() < 1e-4
    gone = [3, 15, 16, 30]  # on either side of the wrap
    less = A.board_pose(np.delete(table, gone), 6, 6, cam, tag_size=TAG_SIZE, first_id=first, spacing_ratio=s, predict_missing=True)
    assert less["status"] == OK and less["pred"]["id"].tolist() == [layout[k] for k in gone]
    assert np.abs(less["pred"]["xy"].reshape(-1, 4, 2) - PC.project(cam, R, t, P[gone])).max() < 1e-3
    off = table[:2].copy()
    off["id"] = [first - 1, (first + 36) % (1 << 32)]  # next to the window on either side
    mixed = A.board_pose(np.concatenate([off[:1], table, off[1:]]), 6, 6, cam, tag_size=TAG_SIZE, first_id=first, spacing_ratio=s)
    assert mixed["row_status"].tolist() == [PC.OFF_BOARD] + [PC.INLIER] * 36 + [PC.OFF_BOARD] and mixed["n_inliers"] == 36


def test_the_unit_of_tag_size_only_scales_t():
    """The same pixels at tag_size 1e-3, 0.05 and 1e3: R and t / tag_size agree to 1e-9, rms and the predicted rows to one
    binary32 ulp.  Observed: not bit-equal -- q = sb / tag_size and X = (...) tag_size round differently at each tag_size (0.05 and
    1e-3 are no powers of two), so the doubles differ in their last bits; the binary32 results are the same bits at all but
    the few values where that falls on a rounding boundary (printed)."""
    cam = CAMERAS["full"]
    R, t = PC.pose("tilt40", 6, 6)
    table = PC.exact_table(6, 6, range(36), cam, R, t, noise=0.1, seed=11)
    got = {ts: A.board_pose(table, 6, 6, cam, tag_size=ts) for ts in (1e-3, TAG_SIZE, 1e3)}
    ref = got[TAG_SIZE]
    assert ref["status"] == OK and np.abs(ref["t"] - t).max() < 1e-2 * PC.extent(6, 6)
    for ts, g in got.items():
        assert g["status"] == OK
        dR = np.abs(g["R"] - ref["R"]).max()
        dt = (np.abs(g["t"] / ts - ref["t"] / TAG_SIZE) / np.abs(ref["t"] / TAG_SIZE)).max()
        a, b = g["pred"]["xy"].view(np.int32).astype(np.int64), ref["pred"]["xy"].view(np.int32).astype(np.int64)
        ulp_pred = int(np.abs(a - b).max())
        ulp_rms = abs(int(np.float32(g["rms"]).view(np.int32)) - int(np.float32(ref["rms"]).view(np.int32)))
        print("tag_size %g against %g: R differs by %.3g, t / tag_size by %.3g relative, pred by %d ulp (%d of %d values), rms by %d ulp, pose bytes %s"
              % (ts, TAG_SIZE, dR, dt, ulp_pred, int((a != b).sum()), a.size, ulp_rms, "equal" if g["pose"][:9].tobytes() == ref["pose"][:9].tobytes() else "differ"))
        assert dR <= 1e-9 and dt <= 1e-9 and ulp_pred <= 1 and ulp_rms <= 1
        assert g["pred"]["id"].tolist() == ref["pred"]["id"].tolist() and g["row_status"].tolist() == ref["row_status"].tolist()


def outer_ring(cols, rows):
    return [r * cols + c for r in range(rows) for c in range(cols) if r in (0, rows - 1) or c in (0, cols - 1)]


def test_the_homography_fails_under_a_strong_barrel_where_the_pose_does_not():
    """Why the feature exists: the 6 x 6 board that fills the wide camera's image ("near"), +-0.1 px of noise.  Every tag of the
    outermost ring is predicted from a table that lacks it: the ring's 20 tags leave the table four at a time (what a board search
    loses at the border of a frame; with all 20 gone at once the remaining 4 x 4 tags extrapolate their +-0.1 px of noise to 0.24 px
    at the corners, which says nothing about the model)."""
    cols, rows, cam = 6, 6, CAMERAS["barrel"]
    R, t = PC.pose("near", cols, rows)
    full = PC.exact_table(cols, rows, range(36), cam, R, t, noise=0.1, seed=11)
    truth = PC.project(cam, R, t, PC.board_points(cols, rows, tag_size=TAG_SIZE))
    ring = outer_ring(cols, rows)
    fit_all = A.board_fit(full, cols, rows, PC.SIZE)
    assert len(ring) == 20 and fit_all["rms"] > 1.0
    seen = []
    for g in range(5):
        miss = ring[g::5]
        keep = np.array([i for i in range(36) if i not in miss])
        fit = A.board_fit(full[keep], cols, rows, PC.SIZE, predict_missing=True)
        pose = A.board_pose(full[keep], cols, rows, cam, tag_size=TAG_SIZE, predict_missing=True)
        assert fit["status"] in (OK, LOOSE) and pose["status"] == OK and fit["pred"]["id"].tolist() == pose["pred"]["id"].tolist() == miss
        d_fit = np.linalg.norm(fit["pred"]["xy"].reshape(-1, 4, 2) - truth[miss], axis=-1).max(axis=1)
        d_pose = np.linalg.norm(pose["pred"]["xy"].reshape(-1, 4, 2) - truth[miss], axis=-1).max(axis=1)
        print("barrel, tags %s: board_fit's predictions %s px off; board_pose rms %.4f px, predictions %s px off" % (miss, d_fit.round(1), pose["rms"], d_pose.round(3)))
        assert (d_fit > 3.0).all()  # detect_recovered's default max_dist: none of them would snap
        assert pose["rms"] < 0.1 and d_pose.max() < 0.2  # the noise is +-0.1 px a coordinate: an rms of 0.058 px
        seen += miss
    assert sorted(seen) == ring
    print("barrel: board_fit rms %.3f px over the whole board" % fit_all["rms"])


def test_without_distortion_the_pose_predicts_what_the_homography_predicts():
    for cols, rows in LAYOUTS:
        for p in sorted(POSES):
            table, got, _, _ = solved(cols, rows, p, "pinhole", 0.0)
            fit = A.board_fit(table, cols, rows, PC.SIZE)
            d = np.abs(fit["pred"]["xy"].astype(np.float64) - got["pred"]["xy"]).max()
            assert d <= EXACT_BOUND, (cols, rows, p, d)


@pytest.mark.parametrize("k", (0, 1, 2))
def test_on_rendered_frames_the_rms_is_the_homographys(k):
    """The renderer draws the board through a homography of its own, not through a camera, so the test takes a zero-skew pinhole
    under which that homography is a rigid view (board_pose_cases.camera_of: the principal point is free, and with it at the
    image's centre frames 0 and 1 have no real focal length).  The pose has 6 unknowns against the homography's 8."""
    img, gt, tags, (w, h, rows, cols) = BC.frame(k)
    table = BC.tag_rows(tags)
    fit = A.board_fit(table, cols, rows, (w, h))
    K = PC.camera_of(fit["H"], w, h)
    assert K is not None
    got = A.board_pose(table, cols, rows, A.Camera(*K))
    print("frame %d: board_fit rms %.4f px, board_pose rms %.4f px at fx %.0f fy %.0f cx %.0f cy %.0f" % ((k, fit["rms"], got["rms"]) + K))
    assert got["status"] == OK and abs(got["rms"] - fit["rms"]) <= 0.02


def test_on_a_warped_frame_the_camera_recovers_strictly_more_tags():
    """The strict inequality of tests/test_gpu_board_pose.py established on the host forms: the rendered 6 x 6 frame seen through
    the strong barrel, four outer-ring tags taken out of the oracle's table; the homography brings back two of them, the pose all
    four (the same counts at k1 / k2 = -0.1 / 0.01 and -0.2 / 0.05: a margin in the strength)."""
    luma, cam, saddles, tags, (w, h, rows, cols) = PC.warped_frame()
    assert len(tags) == 36
    less = {t: xy for t, xy in tags.items() if t not in PC.WARP_MISSING}
    plain, fit = PC.recovered_host(luma, saddles, less, cols, rows)
    with_cam, pose = PC.recovered_host(luma, saddles, less, cols, rows, camera=cam)
    print("warped frame: %d tags with board_fit (rms %.3f px), %d with board_pose (rms %.3f px)" % (len(plain), fit["rms"], len(with_cam), pose["rms"]))
    assert len(with_cam) == 36 and len(plain) == 34 and pose["rms"] < 0.1 < fit["rms"]
    for t in PC.WARP_MISSING:  # and they come back where the oracle found them
        assert np.array_equal(with_cam[t].view(np.uint32), np.asarray(tags[t], np.float32).view(np.uint32))


def test_on_a_rendered_board_whose_ids_start_at_100_the_missing_tags_come_back():
    """first_id through the recovery restated over the host forms, with and without a camera: the renderer prints ids 100 .. 135,
    the oracle detects all of them, three leave the table and return with the oracle's corners bit for bit."""
    luma, saddles, tags, cam = PC.frame_from_100()
    assert sorted(tags) == list(range(100, 136))
    gone = (100, 114, 135)
    less = {t: xy for t, xy in tags.items() if t not in gone}
    for camera in (None, cam):
        got, fit = PC.recovered_host(luma, saddles, less, 6, 6, camera=camera, first_id=PC.FRAME_FIRST_ID)
        assert fit["status"] == OK and fit["n_inliers"] == 33 and fit["pred"]["id"].tolist() == list(gone)
        assert list(got) == list(less) + list(gone)
        for t in tags:
            assert np.array_equal(got[t].view(np.uint32), np.asarray(tags[t], np.float32).view(np.uint32)), t
    # under first_id = 0 only the ids 100 .. 135 that a 6 x 6 layout from 0 holds are on the board: none
    assert PC.recovered_host(luma, saddles, less, 6, 6, camera=cam)[1]["status"] == FEW


def base36(cam="mild", noise=0.1):
    R, t = PC.pose("tilt40", 6, 6)
    return PC.exact_table(6, 6, range(36), CAMERAS[cam], R, t, noise=noise, seed=3)


def test_a_wrong_id_is_dropped_in_one_round_and_max_drop_limits():
    t = PC._wrong(base36(), 1)
    got = A.board_pose(t, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, max_drop=1)
    assert got["status"] == OK and got["n_inliers"] == 34 and got["row_status"].tolist() == [1 if r == 2 else 0 for r in range(35)]
    assert got["rms"] < 0.1 and got["err_sq"][2] > 100.0
    clean = A.board_pose(np.delete(t, 2), 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE)
    assert np.abs(clean["pose"] - got["pose"]).max() < 1e-6  # the second round starts from the first one's answer, not from the seed
    loose = A.board_pose(t, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, max_drop=0)
    assert loose["status"] == LOOSE and loose["n_inliers"] == 35 and not loose["row_status"].any()
    two = PC._wrong(base36(), 2)
    assert A.board_pose(two, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, max_drop=1)["status"] == LOOSE
    got = A.board_pose(two, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, max_drop=2)
    assert got["status"] == OK and sorted(np.flatnonzero(got["row_status"]).tolist()) == [2, 4]


def test_a_byte_equal_residual_tie_goes_to_the_lower_row():
    t = PC._wrong(base36(), 1)
    tie = np.concatenate([t[:9], t[2:3], t[9:]])  # the wrong row twice: rows 2 and 9
    got = A.board_pose(tie, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, max_drop=1)
    assert got["row_status"][2] == PC.OUTLIER and got["row_status"][9] == PC.INLIER and got["status"] == LOOSE
    got = A.board_pose(tie, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, max_drop=2)
    assert got["row_status"][2] == got["row_status"][9] == PC.OUTLIER and got["status"] == OK


def test_refused_frames_write_their_status_and_two_zero_counts_only():
    t = base36()
    for name, table, kw, status in (("few", t[:0], {}, FEW), ("min_tags", t, dict(min_tags=37), FEW), ("flat", PC.flat_row(t), {}, SINGULAR),
                                    ("nan", PC.nan_row(t), {}, INPUT), ("tag_status", t, dict(tag_status=[_ffi.AGX_TAGS_CAPACITY]), INPUT),
                                    ("count", t, dict(counts=[37], tpf=36), INPUT),
                                    ("few_after_drop", PC._wrong(t, 1), dict(max_drop=1, min_tags=35), FEW)):
        b = PC.PoseBatch(name, [table], 6, 6, CAMERAS["mild"], **dict(dict(tpf=40), **kw))
        out = b.host()
        assert out["status"][0] == status and out["n_inliers"][0] == 0 and out["n_pred"][0] == 0, name
        assert all(BC.untouched(out[k]) for k in ("pose", "err_sq", "row_status", "rms", "best_iter", "pred")), name


def test_off_board_rows_are_marked_and_never_fitted():
    t = base36()
    off = t[:4].copy()
    off["id"] = [36, 100, 0xFFFFFFFF, 40]
    off["xy"][2, 3] = np.nan  # never read: the row is not on the board
    mixed = np.concatenate([off[:2], t, off[2:]])
    got, want = A.board_pose(mixed, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE), A.board_pose(t, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE)
    assert got["status"] == OK and got["n_inliers"] == 36 and got["pose"].tobytes() == want["pose"].tobytes()
    assert got["row_status"].tolist() == [2, 2] + [0] * 36 + [2, 2] and np.isnan(got["err_sq"][[0, 1, 38, 39]]).all()


def test_a_single_tag_gives_a_pose_and_iterations_0_returns_the_seed():
    R, t = PC.pose("tilt40", 6, 6)
    one = PC.exact_table(6, 6, [14], CAMERAS["mild"], R, t)
    got = A.board_pose(one, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE)
    assert got["status"] == OK and got["rms"] < 1e-3 and np.abs(got["t"] - t).max() < 0.02 * t[2]
    is_rotation(got["R"])
    seed = A.board_pose(base36(), 6, 6, CAMERAS["barrel"], tag_size=TAG_SIZE, iterations=0, return_iter_sums=True)
    assert seed["best_iter"] == 0 and seed["status"] in (OK, LOOSE) and len(seed["iter_sums"]) == 1
    is_rotation(seed["R"])
    full = A.board_pose(base36(), 6, 6, CAMERAS["barrel"], tag_size=TAG_SIZE, iterations=3, return_iter_sums=True)
    assert full["iter_sums"][0] == seed["iter_sums"][0] and full["best_iter"] > 0  # iterate 0 is the seed


def test_the_best_iterate_rule_on_the_recorded_sums():
    """The answer is the iterate with the lowest finite sum, the earliest at equal bits -- asserted on the sums the host form
    records, over every case and over a lone far tag seen at a grazing angle, where Gauss-Newton steps overshoot."""
    seen_not_last = 0
    tables = [(solved(c, r, p, k, 0.1)[0], c, r, k) for c, r, p, k in CASES]
    R, t = PC.rotation(0.0, 84.0, 0.0), np.array([0.0, 0.0, 60.0 * TAG_SIZE])
    for cam in sorted(CAMERAS):
        tables.append((PC.exact_table(6, 6, [35], CAMERAS[cam], R, t, noise=0.3, seed=5), 6, 6, cam))
    for table, cols, rows, cam in tables:
        for it in (1, 10, 64):
            got = A.board_pose(table, cols, rows, CAMERAS[cam], tag_size=TAG_SIZE, iterations=it, max_err_sq=1e30, return_iter_sums=True)
            if got["status"] != OK:
                continue
            sums = got["iter_sums"]
            finite = np.isfinite(sums)
            want = int(np.flatnonzero(finite & (sums == sums[finite].min()))[0]) if finite.any() else 0
            assert got["best_iter"] == want, (cam, it, sums)
            seen_not_last += want != it
            assert float(got["rms"]) ** 2 <= (sums[0] / (4 * got["n_inliers"])) * (1 + 1e-6) + 1e-12  # never worse than the seed
    assert seen_not_last > 0  # the rule was exercised: some answer is not the last iterate


@pytest.mark.parametrize("n", (63, 64, 65, 128, 129, 587))
def test_row_counts_around_the_lane_stride(n):
    b, _ = PC.gpu_batches()["64x64_barrel_it10_drop2_missing"]
    full = b.tables[7]
    table = full[:n] if n <= len(full) else None
    got = A.board_pose(table, 64, 64, CAMERAS["barrel"], tag_size=0.01, first_id=5)
    Ry, ty, ssq = PC.yardstick(table, 64, 64, CAMERAS["barrel"], *PC.pose("tilt40", 64, 64, 0.01), tag_size=0.01, first_id=5)
    mine = float(np.sum((PC.project(CAMERAS["barrel"], got["R"], got["t"], PC.board_points(64, 64, tag_size=0.01)[table["id"].astype(int) - 5]) -
                         table["xy"].astype(np.float64).reshape(-1, 4, 2)) ** 2))
    assert got["status"] == OK and got["n_inliers"] == n and (mine - ssq) / ssq <= 1e-6


def test_layouts_1x1_and_64x64_and_a_prediction_behind_the_camera():
    b, status = PC.gpu_batches()["1x1"]
    out = b.host()
    assert out["status"][:3].tolist() == status and out["n_pred"][0] == 0  # the only tag is an inlier: nothing is missing
    # a board seen at 85 degrees whose far end passes behind the camera: the table holds the near tags, the far ones have no projection
    R, t = PC.rotation(0.0, 85.0, 0.0), np.array([0.0, 0.0, 0.2])
    ids = [r * 64 + c for r in (30, 31, 32) for c in range(24, 30)]
    P = PC.board_points(64, 64, tag_size=0.01)
    z = (P @ R.T + t)[..., 2]
    assert (z[ids] > 0).all() and (z < 0).any()
    table = PC.exact_table(64, 64, ids, CAMERAS["pinhole"], R, t, 0.01)
    got = A.board_pose(table, 64, 64, CAMERAS["pinhole"], tag_size=0.01)
    assert got["status"] == OK and len(got["pred"]) == 4096
    xy = got["pred"]["xy"].reshape(4096, 4, 2)
    zz = (P @ got["R"].T + got["t"])[..., 2]
    assert np.isnan(xy[zz <= 0]).all() and np.isfinite(xy[zz > 1e-9]).all() and np.isnan(xy).any()


def test_argument_rules():
    t = base36()
    good = PC.camera_args(CAMERAS["mild"])
    for kw in (dict(tag_size=0.0), dict(tag_size=np.nan), dict(tag_size=np.inf), dict(iterations=65), dict(cols=0), dict(cols=65, rows=64),
               dict(spacing_ratio=-1.0), dict(max_err_sq=-1.0), dict(min_tags=0)):
        args = dict(cols=6, rows=6, tag_size=TAG_SIZE)
        args.update(kw)
        cols, rows = args.pop("cols"), args.pop("rows")
        with pytest.raises(A.AgxError) as e:
            A.board_pose(t, cols, rows, CAMERAS["mild"], **args)
        assert e.value.status == _ffi.AGX_ERR_ARG, kw
    for i in range(9):
        for v in (np.nan, np.inf) + ((0.0, -1.0) if i < 2 else ()):
            with pytest.raises(A.AgxError):
                A.board_pose(t, 6, 6, good[:i] + [v] + good[i + 1:], tag_size=TAG_SIZE)
    with pytest.raises(A.AgxError):
        A.board_pose(t, 6, 6, None)
    assert A.board_pose(t, 6, 6, CAMERAS["mild"], tag_size=TAG_SIZE, iterations=64)["status"] == OK


def test_header_python_and_rust_agree_on_the_camera_and_the_declarations():
    hdr = open(BC.__file__.replace("tests/board_fit_cases.py", "include/aprilgrid_amd.h")).read()
    m = re.search(r"struct agx_camera \{ double ([^;]*); \};", hdr)
    assert m and [f.strip() for f in m.group(1).split(",")] == list(A.Camera._fields)
    rust = open(BC.__file__.replace("tests/board_fit_cases.py", "bindings/rust/src/lib.rs")).read()
    body = re.search(r"pub struct Camera \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): f64", body) == list(A.Camera._fields)
    assert "camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2, camera.k3" in rust
    for name in ("agx_board_pose_enqueue", "agx_board_pose_tail", "agx_debug_board_pose_sums"):
        assert name in _ffi.SYMBOLS and name in hdr and hasattr(_ffi.lib(), name)
    assert len(_ffi.SYMBOLS["agx_board_pose_enqueue"][1]) == 26 and len(_ffi.SYMBOLS["agx_board_pose_tail"][1]) == 24
    assert C.sizeof(A.Camera(1, 1, 0, 0).as_doubles()) == 72
