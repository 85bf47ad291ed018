"""detect_decimated end to end: one 6 x 6 board rendered at 1280 x 960 by render_boards_enqueue with its truth corners -- the pose
of tests/test_render_cpu.py's round trip (RC.TRIP_POSE) under its radtan camera with the focal lengths doubled, and the principal
point with them, since the frame has twice the round trip's sides: the same view at twice the resolution.

The yardstick is the full-resolution detector on the same frame: detect_batch_device must find all 36 tags (else the input is
wrong, not the feature) and its largest corner error against the truth rows is e_full.  detect_decimated(factor=2) must find
the same 36 ids with a largest corner error of at most 2 e_full -- the margin tests/test_render_cpu.py already gives a corner
bound, justified here because the fine refine starts from a point that may round to the neighbouring pixel.  factor=1 is
detect_staged, exactly.  Factors 3 and 4 are run and reported, not gated: at 4 the coarse error may exceed rochade_refine's
one-pixel move limit."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from tests import render_cases as RC

pytestmark = pytest.mark.gpu

SIZE = (1280, 960)


def camera():
    c = RC.TRIP_CAMERAS["radtan"]
    return A.Camera(2.0 * c.fx, 2.0 * c.fy, 2.0 * c.cx, 2.0 * c.cy, c.k1, c.k2, c.p1, c.p2, c.k3)


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def scene(det):
    """-> (frames uint8 [1, 960, 1280] on the device, truth corners float64 [36, 4, 2], the full-resolution result)"""
    import torch
    w, h = SIZE
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda:0")
    frames = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda:0")
    poses = torch.from_numpy(A.pose_rows([RC.looking_at(RC.TRIP_POSE)])).cuda()
    truth, n_truth, status = i32(1, 36, 9), i32(1), i32(1)
    det.render_boards_enqueue(frames, 6, 6, camera(), poses, truth, n_truth, status, supersample=4)
    det.sync()
    assert status.tolist() == [0] and n_truth.tolist() == [36]
    rows = truth.cpu().numpy().view(A.TagDetector.TAG_DTYPE).reshape(36)
    assert list(rows["id"]) == list(range(36))
    xy = rows["xy"].reshape(36, 4, 2).astype(np.float64)
    assert xy.min() > 16 and (xy[..., 0] < w - 16).all() and (xy[..., 1] < h - 16).all()
    full = det.detect_batch_device(frames)[0]
    return frames, xy, full


def corner_error(tags, xy):
    return max(float(np.abs(np.asarray(tags[i], np.float64) - xy[i]).max()) for i in tags)


def test_the_full_resolution_detector_finds_the_board(scene):
    _, xy, full = scene
    assert sorted(full) == list(range(36)), "the input is wrong, not the feature"
    print("e_full = %.4f px" % corner_error(full, xy))


def test_factor_2_finds_every_tag_within_twice_the_full_resolution_error(det, scene):
    frames, xy, full = scene
    assert sorted(full) == list(range(36)), "the input is wrong, not the feature"
    e_full = corner_error(full, xy)
    got = det.detect_decimated(frames, factor=2)[0]
    e_dec = corner_error(got, xy) if got else float("inf")
    same = sum(int(np.array_equal(np.asarray(got[i][c]).view(np.uint32), np.asarray(full[i][c]).view(np.uint32)))
               for i in got if i in full for c in range(4))
    print("factor 2: %d tags, e_full = %.4f px, e_decimated = %.4f px, %d of 144 corners with the full-resolution bytes" % (len(got), e_full, e_dec, same))
    assert sorted(got) == list(range(36))
    assert e_dec <= 2.0 * e_full, (e_dec, e_full)


def test_factor_1_is_detect_staged(det, scene):
    frames = scene[0]
    a, b = det.detect_decimated(frames, factor=1), det.detect_staged(frames)
    assert len(a) == len(b) == 1 and list(a[0]) == list(b[0]) and len(a[0]) == 36
    for i in a[0]:
        assert a[0][i].tobytes() == b[0][i].tobytes()


@pytest.mark.parametrize("factor", (3, 4))
def test_factors_3_and_4_run_and_report(det, scene, factor):
    """Reported, not gated: the ids found and their largest corner error."""
    frames, xy, _ = scene
    got = det.detect_decimated(frames, factor=factor)[0]
    assert all(0 <= i < 36 for i in got)  # (whatever is found is a tag of the board)
    print("factor %d: %d of 36 tags, largest corner error %s px" % (factor, len(got), "%.4f" % corner_error(got, xy) if got else "-"))


def test_the_fine_saddles_are_full_resolution_refinements(det, scene):
    """return_saddles: every listed fine saddle lies inside the frame, and the coarse stages ran on a quarter of the pixels."""
    frames = scene[0]
    out, (records, counts, status) = det.detect_decimated(frames, factor=2, return_saddles=True)
    n = int(counts[0])
    rec, st = records[0, :n].cpu().numpy(), status[0, :n].cpu().numpy()
    listed = rec[st == 0]
    assert len(out[0]) == 36 and len(listed) >= 144
    assert (listed[:, 0] >= 4).all() and (listed[:, 0] <= SIZE[0] - 5).all() and (listed[:, 1] >= 4).all() and (listed[:, 1] <= SIZE[1] - 5).all()
