"""The host forms of the rectification under AGX_LENS_DOUBLE_SPHERE (agx_rectify_map_tail, agx_rectified_points_tail) against the
numpy float64 restatement of the model (tests/board_pose_ds_cases.py): the map within 1/64 px (its 1/32 px quantisation), the
points within POINTS_MEASURED (their binary32 rounding below 128 px: 2^-18 = 3.8e-6 px, measured 3.8e-6; bound 10 x), and what the
model is for -- a target turned by 60 degrees about Y, whose far columns look past the image plane (rays with Z <= 0), has map
entries there under the double-sphere camera and AGX_MAP_NONE under the equidistant one."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A

from tests import board_pose_cases as PC
from tests import board_pose_ds_cases as DC
from tests import rectify_cases as RC
from tests.rectify_cases import DST, NEW_CAMERA, NONE, SRC

POINTS_MEASURED = 3.9e-6  # px
TURN = PC.rotation(0.0, 60.0, 0.0)
# "wide": fx = 18 on the 83 x 59 source -- a ray 104 degrees off the axis still lands inside the image.  "tele": fx = 48, the target's
# corners look past the source.  Both (xi, alpha) = (-0.2, 0.59).
CAMERAS = {"wide": DC.camera(-0.2, 0.59, 18.0, 18.5, 41.3, 28.7), "tele": DC.camera(-0.2, 0.59, 48.0, 49.0, 41.3, 28.7)}


def numpy_map(cam, src, dst, new_camera, rotation):
    """rectify_cases.numpy_map under the restated double-sphere model -> (uv, valid, near a validity boundary, the rays)."""
    i, j = np.meshgrid(np.arange(dst[0]), np.arange(dst[1]))
    Q = RC.rays(new_camera, rotation, i, j)
    uv = DC.project_rays(cam, Q)
    lim = np.array([src[0] - 1, src[1] - 1], np.float64) + 1.0 / 64.0
    fin = np.isfinite(uv).all(-1)
    with np.errstate(invalid="ignore"):
        valid = fin & (uv >= -1.0 / 64.0).all(-1) & (uv < lim).all(-1)
        near = fin & ((np.abs(uv + 1.0 / 64.0) < 1e-9).any(-1) | (np.abs(uv - lim) < 1e-9).any(-1))
    d1 = np.linalg.norm(Q, axis=-1)
    near |= np.abs(Q[..., 2] + DC.cone(cam) * d1) < 1e-9 * d1
    return uv, valid, near, Q


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("lens", ["wide", "tele"])
def test_map_is_the_restatement_rounded_to_a_32nd_of_a_pixel(lens, rotated):
    cam, R = CAMERAS[lens], TURN if rotated else None
    m = A.rectify_map(cam, SRC, DST, NEW_CAMERA, R)
    assert m.shape == (DST[1], DST[0], 2) and m.dtype == np.int32
    uv, valid, near, _ = numpy_map(cam, SRC, DST, NEW_CAMERA, R)
    assert not near.any()
    ours = m[..., 0] != NONE
    assert np.array_equal(ours, m[..., 1] != NONE)
    assert np.array_equal(ours, valid) and int(ours.sum()) == int(valid.sum())
    err = np.abs(m[ours] / 32.0 - uv[ours]).max()
    print("%s rotated=%s: %d valid of %d, max |m / 32 - numpy| = %.6f px" % (lens, rotated, ours.sum(), ours.size, err))
    assert err <= 1.0 / 64.0 + 1e-9
    if lens == "tele":
        assert 0.2 < valid.mean() < 0.99  # (entries of both kinds)


def test_a_target_turned_past_the_image_plane_has_entries_where_the_equidistant_model_has_none():
    cam = CAMERAS["wide"]
    uv, valid, near, Q = numpy_map(cam, SRC, DST, NEW_CAMERA, TURN)
    behind = Q[..., 2] <= 0.0
    assert DC.valid(cam, Q).all() and not near.any()
    assert behind[:, -1].all() and not behind[:, 0].any() and 0.15 < behind.mean() < 0.4  # the far columns
    assert valid[behind].all()  # (by the restatement alone: inside the cone and inside the source)
    m = A.rectify_map(cam, SRC, DST, NEW_CAMERA, TURN)
    ours = m[..., 0] != NONE
    assert ours[behind].all() and int(ours.sum()) == int(valid.sum()) and np.array_equal(ours, valid)
    equi = A.rectify_map(A.Camera.equidistant(*cam[:4]), SRC, DST, NEW_CAMERA, TURN)
    assert (equi[behind] == NONE).all() and (equi[~behind][..., 0] != NONE).any()
    print("turned by 60 degrees: %d of %d entries have Z <= 0, all valid under double sphere, none under equidistant; farthest ray %.1f degrees" %
          (behind.sum(), behind.size, np.degrees(np.arctan2(np.hypot(Q[..., 0], Q[..., 1]), Q[..., 2])).max()))


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("lens", ["wide", "tele"])
def test_rectified_points_against_the_restatement(lens, rotated):
    cam, R = CAMERAS[lens], TURN if rotated else None
    rng = np.random.RandomState(5)
    pts = (rng.rand(500, 2) * [DST[0], DST[1]]).astype(np.float32)
    got = A.rectified_points(pts, cam, NEW_CAMERA, R)
    want = DC.project_rays(cam, RC.rays(NEW_CAMERA, R, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)))
    assert got.dtype == np.float32 and np.isfinite(want).all()
    keep = np.abs(want).max(axis=-1) < 128.0  # (the binary32 rounding the bound is worked out for)
    d = np.abs(got[keep].astype(np.float64) - want[keep]).max()
    print("%s rotated=%s: rectified_points %.3g px at worst from the restatement over %d points (recorded %.3g, bound 10 x)" %
          (lens, rotated, d, keep.sum(), POINTS_MEASURED))
    assert keep.sum() > 100 and d <= 10.0 * POINTS_MEASURED
    assert np.abs(got.astype(np.float64) / want - 1.0).max() < 1e-6
    # at integer positions the points are the map's entries before quantisation
    i, j = np.meshgrid(np.arange(DST[0]), np.arange(DST[1]))
    grid = A.rectified_points(np.stack([i, j], axis=-1).astype(np.float32), cam, NEW_CAMERA, R)
    m = A.rectify_map(cam, SRC, DST, NEW_CAMERA, R)
    ok = m[..., 0] != NONE
    assert np.abs(grid[ok].astype(np.float64) - m[ok] / 32.0).max() <= 1.0 / 64.0 + 2.0 ** -17
    # outside the cone, and not finite: (NaN, NaN)
    back = A.rectified_points(np.float32([[47.5, 30.2], [np.nan, 1.0]]), cam, NEW_CAMERA, PC.rotation(0.0, 180.0, 0.0))
    assert np.isnan(back).all()


def test_refusals_follow_the_poses_rules():
    good = PC.camera_args(CAMERAS["wide"])
    assert A.rectify_map(A.Camera(*good), SRC, (5, 3), NEW_CAMERA).shape == (3, 5, 2)  # (nine doubles read as radial-tangential)
    for i, v in ((5, -1e-9), (5, 1.0 + 1e-9), (5, np.nan), (4, -1.0), (4, 1.0 + 1e-9), (4, np.inf), (6, 5e-324), (7, 5e-324), (8, 5e-324)):
        bad = A.Camera.double_sphere(*good[:6])._replace(**{A.Camera._fields[i]: v})
        assert bad.model == DC.DS
        with pytest.raises(A.AgxError):
            A.rectify_map(bad, SRC, (5, 3), NEW_CAMERA)
        with pytest.raises(A.AgxError):
            A.rectified_points(np.zeros((1, 2), np.float32), bad, NEW_CAMERA)
