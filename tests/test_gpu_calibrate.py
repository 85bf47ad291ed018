"""agx_calibrate_enqueue (k_calib_blocks, k_calib_solve) against agx_calibrate_tail: every output byte -- d_camera, d_pose,
d_frame_cost, d_frame_n, d_report -- with guard words around each array, on the smallest shapes at which the kernels can go wrong:
frame counts around the 64 lanes of the frame fold, tables around the 64 lanes of the row sums and at 587 rows, unusable frames at
both ends and in the middle, the three lenses, masks, iteration counts, damping, aliasing, the numerical cases that freeze the
state, the refused calls and the argument rules."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import calibrate_cases as CC

pytestmark = pytest.mark.gpu
GUARD = 16  # elements of guard in front of and behind every output array


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector(A.TagFamily.T36H11, None, device=0)
    yield d
    d.close()


def guarded(torch, host, fill):
    """a device tensor of host's shape and bytes inside a buffer whose other elements are `fill`"""
    flat = torch.full((host.size + 2 * GUARD,), fill, dtype=torch.from_numpy(host.reshape(-1)[:0]).dtype, device="cuda:0")
    view = flat[GUARD:GUARD + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    return flat, view


def run_device(det, batch, camera=None, alias=False, **kw):
    """calibrate_enqueue on the batch from the host form's initial output bytes -> the raw arrays, guards checked"""
    import torch
    ref = batch.host(camera, **kw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tags = dev(batch.tags.view(np.int32).reshape(batch.n, batch.tpf, 9))
    ins = (dev(batch.counts.view(np.int32)), )
    init = {"camera": np.full(9, np.nan), "pose": batch.pose.copy(), "frame_cost": np.full(batch.n, np.nan, np.float32),
            "frame_n": np.full(batch.n, -1, np.int32), "report": np.zeros(69)}
    fills = {"camera": -7.0, "pose": -7.0, "frame_cost": -7.0, "frame_n": -7, "report": -7.0}
    bufs = {k: guarded(torch, v, fills[k]) for k, v in init.items()}
    pose_in = bufs["pose"][1] if alias else dev(batch.pose)
    det.calibrate_enqueue(tags, ins[0], batch.cols, batch.rows, batch.seed if camera is None else camera, pose_in,
                          dev(batch.row_status.view(np.int32)), dev(batch.fit_status.view(np.int32)), bufs["camera"][1], bufs["pose"][1],
                          bufs["frame_cost"][1], bufs["frame_n"][1], bufs["report"][1], tag_size=batch.tag_size, **kw)
    torch.cuda.synchronize()
    out = {}
    for k, (flat, view) in bufs.items():
        f = flat.cpu().numpy()
        assert (f[:GUARD] == fills[k]).all() and (f[-GUARD:] == fills[k]).all(), "guard words of %s" % k
        out[k] = view.cpu().numpy()
    return out, ref


def assert_same_bytes(out, ref, what):
    for k, r in (("camera", "camera_raw"), ("pose", "pose_raw"), ("frame_cost", "frame_cost_raw"), ("frame_n", "frame_n_raw")):
        assert out[k].tobytes() == np.ascontiguousarray(ref[r]).tobytes(), "%s: %s differs" % (what, k)
    assert out["report"].tobytes() == ref["report_raw"].tobytes(), "%s: the report differs: %s" % (what, A.calib_report(out["report"]))


@pytest.fixture(scope="module")
def many():
    """130 frames of 4 .. 12 tags under the radial-tangential camera (noisy: no two frames alike)"""
    cam = CC.CAMERAS["radtan"]
    rng = np.random.RandomState(3)
    tabs = [CC.table(cam, p, ids=rng.permutation(36)[:4 + k % 9], noise=0.1, seed=k + 1) for k, p in enumerate(CC.poses(130))]
    return CC.Batch(tabs, CC.off_seed(cam))


@pytest.mark.parametrize("n", [1, 3, 64, 65, 130])
def test_frame_counts_around_the_fold(det, many, n):
    b = many.subset(range(n))
    out, ref = run_device(det, b, fixed=0x1f0 if n < 3 else 0x100, iterations=2, damping=1e-3)
    assert ref["status"] == CC.OK and ref["n_frames_used"] == n
    assert_same_bytes(out, ref, "n = %d" % n)


@pytest.fixture(scope="module")
def big():
    """tables of 1, 4, 64, 65 and 587 rows of a 64 x 64 layout, tags_per_frame 600; then an unusable frame first, in the middle and
    last (a refused pose, a loose one, too few inliers), and a frame whose rows are all outliers"""
    cam = CC.CAMERAS["radtan"]
    ids = np.random.RandomState(7).permutation(4096)[:587]
    ps = CC.poses(8)
    ps[:, 9:] *= 2.2  # (the board is 0.83 units wide)
    tabs = [CC.table(cam, ps[k], ids=ids[:m], noise=0.05, seed=k + 1, cols=64, rows=64, tag_size=0.01) for k, m in enumerate((1, 4, 64, 65, 587))]
    four = CC.table(cam, ps[5], ids=ids[10:14], noise=0.05, seed=9, cols=64, rows=64, tag_size=0.01)
    b = CC.Batch([tabs[1][:0]] + tabs[:3] + [tabs[2][:2]] + tabs[3:] + [four, tabs[0][:0]], cam, tpf=600, cols=64, rows=64, tag_size=0.01)
    b.fit_status[4] = _ffi.AGX_FIT_LOOSE
    b.row_status[7, :4] = _ffi.AGX_FIT_ROW_OUTLIER  # (frame 7: a 4-row table whose rows are all outliers; frame 2's 4 rows count)
    return b


def test_table_sizes_and_unusable_frames(det, big):
    out, ref = run_device(det, big, fixed=0x1f0, iterations=3, min_tags=1)
    assert ref["status"] == CC.OK and list(ref["frame_n_raw"]) == [0, 4, 16, 256, 0, 260, 2348, 0, 0]
    assert_same_bytes(out, ref, "table sizes")
    # the unusable frames contribute nothing: without them the same bytes
    keep = [1, 2, 3, 5, 6]
    sub = big.subset(keep).host(fixed=0x1f0, iterations=3, min_tags=1)
    assert sub["camera_raw"].tobytes() == ref["camera_raw"].tobytes() and sub["pose_raw"].tobytes() == ref["pose_raw"][keep].tobytes()
    assert sub["report_raw"]["cost"].tobytes() == ref["report_raw"]["cost"].tobytes()
    # AGX_FIT_LOOSE counts under the flag
    out, ref = run_device(det, big, fixed=0x1f0, iterations=1, accept_loose=True)
    assert ref["frame_n_raw"][4] == 8
    assert_same_bytes(out, ref, "accept_loose")


@pytest.mark.parametrize("lens", ["radtan", "equidistant", "double_sphere"])
@pytest.mark.parametrize("fixed,iterations,damping,alias", [(0, 7, 0.0, False), (0x1ff, 1, 1e-3, True), (0x00c, 0, 0.0, False), (0x00c, 7, 1e-3, True)])
def test_lenses_masks_iterations_damping_alias(det, lens, fixed, iterations, damping, alias):
    b = CC.exact_batch(lens, noise=0.1)
    out, ref = run_device(det, b, alias=alias, fixed=fixed | CC.FIXED[lens], iterations=iterations, damping=damping)
    # the batch's seed is CC.off_seed: for the double sphere xi = 0, where the undamped system with every double free is refused
    # at iterate 0 (test_double_sphere_steps_with_every_double_free steps from there under damping)
    refused = lens == "double_sphere" and fixed == 0 and damping == 0.0
    assert ref["status"] == (CC.SINGULAR if refused else CC.OK)
    assert ref["best_iter"] == 0 if refused or iterations == 0 else fixed == 0x1ff or ref["best_iter"] > 0  # (poses alone: already converged)
    assert_same_bytes(out, ref, "%s mask %#x" % (lens, fixed))


def test_double_sphere_steps_with_every_double_free(det):
    """the free-camera, many-iterate double-sphere path: from the zero-distortion seed under the driver's damping, and undamped
    from a seed off xi = 0"""
    b = CC.exact_batch("double_sphere", noise=0.1)
    out, ref = run_device(det, b, iterations=25, damping=1e-6)
    assert ref["status"] == CC.OK and ref["best_iter"] >= 20 and ref["rms"] < 0.081
    assert_same_bytes(out, ref, "double sphere, damped from xi = 0")
    far = A.Camera.double_sphere(175.0, 175.0, 410.0, 290.0, -0.5, 0.9)
    out, ref = run_device(det, CC.Batch([CC.table(CC.CAMERAS["double_sphere"], p, noise=0.1, seed=k + 1) for k, p in enumerate(CC.poses(8))], far),
                          iterations=20)
    assert ref["status"] == CC.OK and ref["best_iter"] >= 10 and ref["rms"] < 0.081
    assert_same_bytes(out, ref, "double sphere, undamped")


def test_numerical_cases_end_with_an_ordinary_status(det):
    cam = CC.CAMERAS["double_sphere"]
    tabs = [CC.table(cam, p) for p in CC.poses(8)]
    for seed, want in ((CC.DS_ALPHA_LEAVES, "alpha"), (CC.DS_DIVERGES, "diverges")):
        out, ref = run_device(det, CC.Batch(tabs, seed), iterations=12)
        assert ref["status"] == CC.OK and ref["best_iter"] == 0, want
        assert_same_bytes(out, ref, want)
        assert out["camera"].tobytes() == np.array(seed, np.float64).tobytes()
    cam = CC.CAMERAS["radtan"]
    b = CC.Batch([CC.table(cam, p) for p in CC.poses(8)], CC.RT_RISES)
    out, ref = run_device(det, b, iterations=12, fixed=0x100)
    c = ref["cost"][:13]
    assert np.any(np.diff(c) > 0) and ref["best_iter"] == int(np.argmin(c))
    assert_same_bytes(out, ref, "a cost that rises")


def test_few_and_singular_leave_every_array_but_the_report(det, many):
    b = many.subset(range(3))
    for bb, kw, status in ((b, dict(min_frames=4), CC.FEW), (CC.few_batch(), dict(fixed=0x100), CC.FEW)):
        out, ref = run_device(det, bb, iterations=2, **kw)
        assert ref["status"] == status
        assert_same_bytes(out, ref, str(kw))
        assert np.isnan(out["camera"]).all() and (out["frame_n"] == -1).all() and np.isnan(out["frame_cost"]).all() and np.array_equal(out["pose"], bb.pose)
    fb = CC.fronto_batch()
    out, ref = run_device(det, fb, iterations=3, fixed=0x1fc)
    assert ref["status"] == CC.SINGULAR
    assert_same_bytes(out, ref, "fronto-parallel")
    assert np.isnan(out["camera"]).all() and (out["frame_n"] == -1).all()


def test_argument_rules_keep_the_batch_in_flight(det, many):
    import torch
    b = many.subset(range(3))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    frames = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda:0")
    tags = dev(b.tags.view(np.int32).reshape(3, b.tpf, 9))
    args = dict(tags=tags, n_tags=dev(b.counts.view(np.int32)), cols=6, rows=6, camera=b.seed, pose_in=dev(b.pose),
                row_status=dev(b.row_status.view(np.int32)), fit_status=dev(b.fit_status.view(np.int32)), camera_out=torch.zeros(9, dtype=torch.float64, device="cuda:0"),
                pose=torch.zeros((3, 12), dtype=torch.float64, device="cuda:0"), frame_cost=torch.zeros(3, dtype=torch.float32, device="cuda:0"),
                frame_n=torch.zeros(3, dtype=torch.int32, device="cuda:0"), report=torch.zeros(69, dtype=torch.float64, device="cuda:0"), tag_size=CC.TAG_SIZE)
    bad = [dict(damping=-1.0), dict(damping=float("nan")), dict(iterations=65), dict(min_tags=0), dict(min_frames=0), dict(tag_size=0.0),
           dict(cols=0), dict(cols=65, rows=64), dict(spacing_ratio=-1.0), dict(camera=A.Camera(0.0, 400.0, 400.0, 300.0)),
           dict(camera=A.Camera.double_sphere(250.0, 250.0, 400.0, 300.0, 0.0, 1.5)), dict(camera=A.Camera(400.0, 400.0, float("inf"), 300.0))]
    for kw in bad:
        det.saddles_batch_enqueue(frames)
        with pytest.raises(A.AgxError) as e:
            det.calibrate_enqueue(**dict(args, **kw))
        assert e.value.status == _ffi.AGX_ERR_ARG, kw
        det.saddles_batch_fetch()  # the batch in flight stayed where it was
    with pytest.raises(A.AgxError):
        det.calibrate_enqueue(**dict(args, fixed=512))
    with pytest.raises(A.AgxError):
        det.calibrate_enqueue(**dict(args, report=torch.zeros(68, dtype=torch.float64, device="cuda:0")))
    lib, h = _ffi.lib(), det._h
    ptrs = [args[k].data_ptr() for k in ("pose_in", "row_status", "fit_status", "camera_out", "pose", "frame_cost", "frame_n", "report")]

    def raw(n=3, tpf=b.tpf, mask=0, flags=0, p=ptrs, cam=b.seed.as_doubles()):
        return lib.agx_calibrate_enqueue(h, n, tags.data_ptr(), tpf, args["n_tags"].data_ptr(), None, 6, 6, 0, 0.3, CC.TAG_SIZE, 0, cam, mask, 0.0, 1, 1, 1,
                                         flags, *p)
    assert raw() == _ffi.AGX_OK
    for kw in (dict(n=0), dict(n=65536), dict(tpf=0), dict(mask=512), dict(flags=2), dict(cam=None), dict(p=ptrs[:7] + [ptrs[7] + 4]),
               dict(p=[ptrs[0] + 4] + ptrs[1:]), dict(p=ptrs[:5] + [ptrs[5] + 2] + ptrs[6:])) + tuple(dict(p=ptrs[:i] + [None] + ptrs[i + 1:]) for i in range(8)):
        assert raw(**kw) == _ffi.AGX_ERR_ARG, kw
    det.sync()


def test_calibrate_batch_on_rendered_frames(det):
    """Render 6 frames on the device, calibrate them on the device, and compare with the composition of the host forms on the
    fetched tables.  CC.FX_MARGIN says how the margin on fx was measured on the CPU."""
    import torch
    cam, poses = CC.render_case()
    frames = torch.zeros((6, 240, 320), dtype=torch.uint8, device="cuda:0")
    truth, n_truth, status = (torch.zeros((6, 16, 9), dtype=torch.int32, device="cuda:0"), torch.zeros(6, dtype=torch.int32, device="cuda:0"),
                              torch.zeros(6, dtype=torch.int32, device="cuda:0"))
    det.render_boards_enqueue(frames, 4, 4, cam, torch.from_numpy(poses).cuda(), truth, n_truth, status, tag_size=CC.TAG_SIZE)
    kw = dict(tag_size=CC.TAG_SIZE, fixed=0x1c0, rounds=3, iterations=10)
    got, pose, report = det.calibrate_batch(frames, 4, 4, **kw)
    assert report["status"] == CC.OK and report["n_frames_used"] >= 4
    want, want_pose, want_report = CC.host_calibrate_batch(det, frames, 4, 4, (320, 240), **kw)
    assert np.array(got, np.float64).tobytes() == np.array(want, np.float64).tobytes()
    used = report["frame_n"] > 0
    assert pose.cpu().numpy()[used].tobytes() == want_pose[used].tobytes()
    assert report["cost"].tobytes() == want_report["cost"].tobytes()
    print("fx", got.fx, "rendered with", cam.fx, "rms", report["rms"])
    assert abs(got.fx - cam.fx) <= CC.FX_MARGIN
