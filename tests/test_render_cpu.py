"""The board renderer's host form (agx_render_boards_tail, csrc/render.hip + csrc/render_math.h) without a GPU: against a numpy
restatement, its truth rows against the pose code's projection, the tags' orientation through the decode, the round trip
render -> detect -> board_pose, background handling and every refused argument."""
import ctypes as C

import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi
from tests import board_pose_cases as PC
from tests import render_cases as RC

TAG = A.TagDetector.TAG_DTYPE
# The oracle's corner error on synth.render_frame frames of 640 x 480 against their ground truth, frames 300 .. 307: 0.059 ..
# 0.0901 px (the README's 0.07 .. 0.10 px).  The round trip's bound is twice the largest: the box filter of S = 4 is cruder than
# synth's 3 x 3 samples plus blur.
YARDSTICK_PX = 0.0901
TRIP_BOUND_PX = 2.0 * YARDSTICK_PX


@pytest.mark.parametrize("name,layout", sorted(RC.SMALL_POSES))
def test_host_form_equals_the_numpy_restatement(name, layout):
    """Every pixel equal, except at most 4 per frame that differ by one sample's weight (measured: none differs).  The poses keep
    every sample of the restatement at least 1e-8 tag sides from an edge of the drawing, checked on the restatement alone; under
    "ds_past_90" samples beyond 90 degrees off the axis (camera-frame Z <= 0) are on the page."""
    cam, (R, t) = RC.SMALL_CAMERAS[name], RC.looking_at(RC.SMALL_POSES[(name, layout)])
    for S, dtype in ((1, np.uint8), (2, np.uint16), (4, np.uint8), (4, np.uint16)):
        black, white, bg = RC.colours(dtype)
        ref, edge_dist, behind = RC.restated(RC.SMALL, layout[0], layout[1], cam, R, t, S=S, dtype=dtype)
        assert edge_dist > 1e-8, (S, edge_dist)
        assert (behind > 0) == (name == "ds_past_90"), behind
        assert (ref != bg).sum() > 1000  # (the board fills a good part of the frame)
        got, truth, n_truth, status = A.render_boards(RC.SMALL, layout[0], layout[1], cam, (R, t), supersample=S, dtype=dtype, black=black,
                                                      white=white, background=bg)
        assert status[0] == _ffi.AGX_RENDER_OK and n_truth[0] == layout[0] * layout[1] and got.dtype == dtype
        diff = np.abs(got[0].astype(np.int64) - ref.astype(np.int64))
        weight = -(-(white - black) // (S * S))
        print(name, layout, S, np.dtype(dtype).name, "differing pixels", int((diff != 0).sum()), "largest", int(diff.max()))
        assert (diff != 0).sum() <= 4 and diff.max() <= weight, ((diff != 0).sum(), diff.max())


def _corner_rays(cols, rows, R, t, s=0.3, tag_size=1.0):
    """pose_board_point's corners by pose_project's first three statements, in their order: camera-frame points [n, 4, 3]"""
    sd = float(np.float32(s))
    pitch = 1.0 + sd
    bx, by = (cols * pitch - sd) / 2.0, (rows * pitch - sd) / 2.0
    k = np.arange(rows * cols)
    r, c = k // cols, k % cols
    X = (c[:, None] * pitch + np.array([0.0, 1.0, 1.0, 0.0]) - bx) * tag_size
    Y = (r[:, None] * pitch + np.array([0.0, 0.0, 1.0, 1.0]) - by) * tag_size
    return np.stack([R[i, 0] * X + R[i, 1] * Y + t[i] for i in range(3)], axis=-1)


@pytest.mark.parametrize("name", sorted(RC.TRIP_CAMERAS))
def test_truth_rows_are_the_pose_codes_projection(name):
    cam = RC.TRIP_CAMERAS[name]
    R, t = RC.looking_at(RC.TRIP_POSE)
    _, truth, n_truth, status = A.render_boards((8, 8), 6, 6, cam, (R, t), supersample=1, tag_size=0.7)
    assert status[0] == _ffi.AGX_RENDER_OK and n_truth[0] == 36 and list(truth[0]["id"]) == list(range(36))
    rays = np.ascontiguousarray(_corner_rays(6, 6, R, t, tag_size=0.7).reshape(-1, 3))
    uv = np.zeros((len(rays), 2))
    assert _ffi.lib().agx_debug_pose_project(cam.model, cam.as_doubles(), rays.ctypes.data, len(rays), uv.ctypes.data) == 0
    assert np.array_equal(uv.astype(np.float32).reshape(36, 8).view(np.uint32), truth[0]["xy"].view(np.uint32))
    # a table that yields a pose: the truth rows themselves; rendered from THAT pose the truth rows are the pose's pred, bit for bit
    fit = A.board_pose(truth[0], 6, 6, cam, tag_size=0.7, first_id=0)
    assert fit["status"] == _ffi.AGX_FIT_OK and fit["n_pred"] == 36
    _, again, n_again, st = A.render_boards((8, 8), 6, 6, cam, fit["pose"], supersample=1, tag_size=0.7)
    assert st[0] == _ffi.AGX_RENDER_OK and n_again[0] == 36
    assert again[0].tobytes() == fit["pred"].tobytes()
    assert np.abs(again[0]["xy"] - truth[0]["xy"]).max() < 1e-3


def test_truth_rows_without_a_projection_are_nan():
    cam = RC.TRIP_CAMERAS["radtan"]
    R, t = A.board_pose_looking_at(1.0, 0.0, 80.0, 10.0)  # a 6 x 6 board turned 80 degrees about y at distance 1: one side is behind
    _, truth, n_truth, status = A.render_boards((8, 8), 6, 6, cam, (R, t), supersample=1)
    assert status[0] == _ffi.AGX_RENDER_OK and n_truth[0] == 36
    z = _corner_rays(6, 6, R, t)[..., 2]
    xy = truth[0]["xy"].reshape(36, 4, 2)
    assert (z <= 0).any() and (z > 0).any()
    assert np.array_equal(np.isnan(xy[..., 0]), z <= 0) and np.array_equal(np.isnan(xy[..., 1]), z <= 0)
    assert (xy.view(np.uint32)[z <= 0] == 0x7fc00000).all()


@pytest.mark.parametrize("family", ["T16H5", "T25H7", "T25H9", "T36H11", "T36H11B1"])
def test_every_tag_decodes_to_its_own_id_at_quarter_turn_zero(family):
    """A 2 x 2 board of each family from first_id 5: agx_decode_quads_tail on the truth corners as quads (a quad is wound the other
    way round than a tag's corners: src/detector.rs:467-470 reverses it) gives every tag its own id with its corners in the given
    order -- quarter turn 0."""
    cam = A.Camera(600.0, 600.0, 320.0, 240.0)
    R, t = A.board_pose_looking_at(6.0, 10.0, -15.0, 20.0)
    frames, truth, n_truth, status = A.render_boards((640, 480), 2, 2, cam, (R, t), family=family, first_id=5, supersample=2)
    assert status[0] == _ffi.AGX_RENDER_OK and n_truth[0] == 4
    quads = np.ascontiguousarray(truth[0]["xy"].reshape(4, 4, 2)[:, ::-1, :])
    tags, st = A.decode_quads_tail(family, frames[0], quads)
    assert (st == 0).all(), st
    assert list(tags["id"]) == [5, 6, 7, 8]
    assert tags["xy"].tobytes() == truth[0]["xy"].tobytes()


@pytest.mark.parametrize("name", sorted(RC.TRIP_CAMERAS))
def test_round_trip_render_detect_board_pose(name):
    """What the renderer is for: a pose and a camera in, the sensor's picture out, and detect -> board_pose gives the pose back --
    the rendered face, not its mirror image.  Bound: TRIP_BOUND_PX = 2 x 0.0901 px = 0.1802 px, twice the oracle's largest corner
    error on synth.render_frame frames of this size (measured 0.059 .. 0.0901 px over frames 300 .. 307).  Measured here: detected
    corners 0.05 .. 0.08 px from the truth rows, the pose's reprojection 0.006 .. 0.015 px."""
    from oracle import oracle as O
    cam = RC.TRIP_CAMERAS[name]
    R, t = RC.looking_at(RC.TRIP_POSE)
    frames, truth, n_truth, status = A.render_boards(RC.TRIP_SIZE, 6, 6, cam, (R, t), supersample=4)
    assert status[0] == _ffi.AGX_RENDER_OK and n_truth[0] == 36
    xy = truth[0]["xy"].reshape(36, 4, 2)
    assert xy.min() > 8 and (xy[..., 0] < RC.TRIP_SIZE[0] - 8).all() and (xy[..., 1] < RC.TRIP_SIZE[1] - 8).all()
    tags = O.detect(frames[0])
    assert sorted(tags) == list(range(36))
    corner = max(float(np.abs(np.asarray(tags[i], np.float64) - xy[i]).max()) for i in tags)
    fit = A.board_pose(tags, 6, 6, cam)
    assert fit["status"] == _ffi.AGX_FIT_OK
    reproj = float(np.abs(fit["pred"]["xy"].reshape(36, 4, 2).astype(np.float64) - xy).max())
    print(name, "corner error", corner, "reprojection", reproj, "R", np.abs(fit["R"] - R).max(), "t", np.abs(fit["t"] - t).max())
    assert corner < TRIP_BOUND_PX and reproj < TRIP_BOUND_PX
    assert np.linalg.det(fit["R"]) > 0.99 and np.abs(fit["R"] - R).max() < 1e-2 and np.abs(fit["t"] - t).max() < 1e-2 * t[2]


def _padded(n, h, w, dtype, row_pad, frame_pad, edge_pad, seed=3):
    """A random buffer and the [n, h, w] view into it with padded rows and frames and guard elements around the batch"""
    rng = np.random.default_rng(seed)
    row, frame = w + row_pad, (w + row_pad) * h + frame_pad
    buf = rng.integers(0, np.iinfo(dtype).max + 1, edge_pad + n * frame + edge_pad, dtype=dtype)
    view = np.lib.stride_tricks.as_strided(buf[edge_pad:], (n, h, w), (frame * buf.itemsize, row * buf.itemsize, buf.itemsize))
    return buf, view


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_background_guard_bytes_and_statuses(dtype):
    cam = A.Camera.equidistant(22.0, 22.5, 18.3, 14.2, -0.013, 0.021, -0.013, 0.0026)
    w, h = 37, 29
    good = RC.looking_at((4.0, 20.0, -25.0, 30.0, (0.2, 0.1)))
    behind = (good[0], np.array([0.0, 0.0, -6.0]))  # the board wholly behind the camera
    bad = (good[0].copy(), good[1].copy())
    bad[1][1] = np.nan
    skew = (good[0] * 1.001, good[1])  # columns of length 1.001: not a rotation
    poses = [good, behind, bad, skew]
    black, white, bg = RC.colours(dtype)
    for keep in (False, True):
        buf, view = _padded(4, h, w, dtype, 3, 5, 11)
        before, inside = buf.copy(), view.copy()
        _, truth, n_truth, status = A.render_boards((w, h), 2, 2, cam, poses, supersample=2, black=black, white=white, background=bg,
                                                    keep_background=keep, out=view)
        assert list(status) == [_ffi.AGX_RENDER_OK, _ffi.AGX_RENDER_EMPTY, _ffi.AGX_RENDER_INPUT, _ffi.AGX_RENDER_INPUT]
        assert list(n_truth) == [4, 0, 0, 0]
        after = view.copy()
        view[...] = inside  # what is left differing is outside the frames' pixels
        assert np.array_equal(buf, before), "a guard byte was written"
        plain = A.render_boards((w, h), 2, 2, cam, [good], supersample=2, black=black, white=white, background=bg, dtype=dtype)[0][0]
        on_page = plain != bg
        assert 100 < on_page.sum() < w * h - 100
        assert np.array_equal(after[2], inside[2]) and np.array_equal(after[3], inside[3])  # AGX_RENDER_INPUT: no byte written
        if keep:
            assert np.array_equal(after[0][~on_page], inside[0][~on_page])  # no sample on the page: the pixel keeps its bytes
            full = (plain == white) | (plain == black)
            assert np.array_equal(after[0][full], plain[full]) and full.sum() > 50
            assert np.array_equal(after[1], inside[1])                      # AGX_RENDER_EMPTY: untouched
        else:
            assert np.array_equal(after[0], plain)
            assert (after[1] == bg).all()                                   # AGX_RENDER_EMPTY: all background


def _tail(**over):
    """agx_render_boards_tail's status with one argument changed"""
    frame = np.zeros((16, 24), np.uint8)
    truth = np.zeros(6, TAG)
    pose = A.pose_rows(A.board_pose_looking_at(5.0))
    a = dict(width=24, height=16, row_stride=24, format=_ffi.AGX_L8, family=3, cols=3, rows=2, first_id=0, spacing_ratio=0.3, tag_size=1.0,
             lens=_ffi.AGX_LENS_RADTAN, camera=(C.c_double * 9)(30.0, 30.0, 12.0, 8.0, 0, 0, 0, 0, 0), pose=pose.ctypes.data,
             params=_ffi.RenderParams(0, 255, 128, 0.5, 2, 0), frame=frame.ctypes.data, truth=truth.ctypes.data, n_truth=C.c_uint32(0),
             status=C.c_uint32(0))
    a.update(over)
    p = a["params"]
    return _ffi.lib().agx_render_boards_tail(a["width"], a["height"], a["row_stride"], a["format"], a["family"], a["cols"], a["rows"], a["first_id"],
                                             a["spacing_ratio"], a["tag_size"], a["lens"], a["camera"], a["pose"],
                                             None if p is None else C.addressof(p), a["frame"], a["truth"],
                                             None if a["n_truth"] is None else C.byref(a["n_truth"]),
                                             None if a["status"] is None else C.byref(a["status"]))


def test_every_refused_argument():
    ARG = _ffi.AGX_ERR_ARG
    assert _tail() == _ffi.AGX_OK
    cam = lambda *v: (C.c_double * 9)(*v)
    P = _ffi.RenderParams
    for over in (dict(camera=None), dict(params=None), dict(pose=None), dict(frame=None), dict(truth=None), dict(n_truth=None), dict(status=None),
                 dict(format=_ffi.AGX_RGB8), dict(format=7), dict(width=0), dict(height=0), dict(width=16385), dict(row_stride=23),
                 dict(format=_ffi.AGX_L16, row_stride=49, params=P(0, 255, 128, 0.5, 2, 0)),                    # an odd stride of 16-bit pixels
                 dict(cols=0), dict(rows=0), dict(cols=65, rows=64), dict(spacing_ratio=-0.1), dict(spacing_ratio=float("nan")),
                 dict(tag_size=0.0), dict(tag_size=float("inf")), dict(lens=3), dict(camera=cam(0.0, 30, 12, 8, 0, 0, 0, 0, 0)),
                 dict(camera=cam(30, 30, float("nan"), 8, 0, 0, 0, 0, 0)), dict(lens=_ffi.AGX_LENS_EQUIDISTANT, camera=cam(30, 30, 12, 8, 0, 0, 0, 0, 0.1)),
                 dict(lens=_ffi.AGX_LENS_DOUBLE_SPHERE, camera=cam(30, 30, 12, 8, 0.5, 1.5, 0, 0, 0)),
                 dict(first_id=582), dict(family=0, cols=6, rows=6),                                            # beyond the code table (587, 30)
                 dict(cols=64, rows=64),                                                                         # 4096 tags: no family has them
                 dict(params=P(0, 255, 128, 0.5, 0, 0)), dict(params=P(0, 255, 128, 0.5, 5, 0)), dict(params=P(256, 255, 128, 0.5, 2, 0)),
                 dict(params=P(0, 256, 128, 0.5, 2, 0)), dict(params=P(0, 255, 256, 0.5, 2, 0)), dict(params=P(0, 255, 128, -0.1, 2, 0)),
                 dict(params=P(0, 255, 128, float("inf"), 2, 0)), dict(params=P(0, 255, 128, 0.5, 2, 2)),
                 dict(pose=A.pose_rows(A.board_pose_looking_at(5.0)).ctypes.data + 4)):
        assert _tail(**over) == ARG, over
    assert _tail(family=9) == _ffi.AGX_ERR_FAMILY
    assert _tail(first_id=581) == _ffi.AGX_OK and _tail(format=_ffi.AGX_L16, row_stride=48, params=P(0, 65535, 300, 0.5, 4, 1)) == _ffi.AGX_OK
    with pytest.raises(A.AgxError):
        A.render_boards((24, 16), 3, 2, A.Camera(30, 30, 12, 8), A.board_pose_looking_at(5.0), supersample=5)


def test_board_pose_looking_at():
    R, t = A.board_pose_looking_at(4.0)
    assert np.array_equal(R, np.diag([1.0, -1.0, -1.0])) and list(t) == [0.0, 0.0, 4.0]
    R, t = A.board_pose_looking_at(3.0, 20.0, -35.0, 50.0, (0.5, -0.25))
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0) and list(t) == [0.5, -0.25, 3.0]
    assert np.allclose(R, PC.rotation(20.0, -35.0, 50.0) @ np.diag([1.0, -1.0, -1.0]))
