"""agx_rig_calibrate_enqueue (k_rig_blocks, k_rig_instants, k_rig_solve) against agx_rig_calibrate_tail: every output byte --
d_extrinsics, d_rig_pose, d_frame_cost, d_frame_n, d_cam_n, d_report -- with guard words around each array, on the smallest shapes
at which the kernels can go wrong: instant counts around the 64 lanes of the instant fold, camera counts 2, 3 and 8, mixed lenses,
tables around the 64 lanes of the row sums and at 587 rows, unusable frames and instants, a held camera, iteration counts, damping,
aliasing, the refused calls and the argument rules."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import calibrate_cases as CC
from tests import rig_cases as RC

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


FILLS = {"extrinsics": -7.0, "rig_pose": -7.0, "frame_cost": -7.0, "frame_n": -7, "cam_n": -7, "report": -7.0}
RAW = {"extrinsics": "extrinsics_raw", "rig_pose": "rig_pose_raw", "frame_cost": "frame_cost_raw", "frame_n": "frame_n_raw", "cam_n": "cam_n_raw"}


def run_device(det, rig, seed, alias=False, **kw):
    """rig_calibrate_enqueue on the rig from the host form's initial output bytes -> the raw arrays, guards checked"""
    import torch
    ref = rig.host(seed, **kw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nc, ns = rig.nc, rig.ns
    init = {"extrinsics": seed.copy() if alias else np.full((nc, 12), np.nan), "rig_pose": np.full((ns, 12), np.nan),
            "frame_cost": np.full((nc, ns), np.nan, np.float32), "frame_n": np.full((nc, ns), -1, np.int32), "cam_n": np.full(nc, -1, np.int32),
            "report": np.zeros(70)}
    bufs = {k: guarded(torch, v, FILLS[k]) for k, v in init.items()}
    ext_in = bufs["extrinsics"][1] if alias else dev(seed)
    det.rig_calibrate_enqueue(dev(rig.tags.view(np.int32).reshape(nc, ns, rig.tpf, 9)), dev(rig.counts.view(np.int32)), rig.cols, rig.rows, rig.cams,
                              dev(rig.pose), dev(rig.row_status.view(np.int32)), dev(rig.fit_status.view(np.int32)), ext_in, bufs["extrinsics"][1],
                              bufs["rig_pose"][1], bufs["frame_cost"][1], bufs["frame_n"][1], bufs["cam_n"][1], bufs["report"][1],
                              tag_size=rig.tag_size, **kw)
    torch.cuda.synchronize()
    out = {}
    for k, (flat, view) in bufs.items():
        f = flat.cpu().numpy()
        assert (f[:GUARD] == FILLS[k]).all() and (f[-GUARD:] == FILLS[k]).all(), "guard words of %s" % k
        out[k] = view.cpu().numpy()
    return out, ref


def assert_same_bytes(out, ref, what, alias_seed=None):
    for k, r in RAW.items():
        want = np.ascontiguousarray(ref[r])
        if k == "extrinsics" and alias_seed is not None and ref["status"] != RC.OK:
            want = alias_seed  # (a refused call leaves the aliased seed)
        assert out[k].tobytes() == want.tobytes(), "%s: %s differs" % (what, k)
    assert out["report"].tobytes() == ref["report_raw"].tobytes(), "%s: the report differs: %s" % (what, A.rig_report(out["report"]))


@pytest.fixture(scope="module")
def many():
    """2 cameras x 130 instants of 4 .. 9 tags (noisy: no two frames alike)"""
    rng = np.random.RandomState(3)
    ids = {(c, s): rng.permutation(36)[:4 + (s + c) % 6] for c in range(2) for s in range(130)}
    return RC.Rig([CC.CAMERAS["radtan"], CC.CAMERAS["equidistant"]], RC.true_extrinsics(2), CC.poses(130), noise=0.1, ids=ids, tpf=12)


@pytest.mark.parametrize("n", [1, 2, 64, 65, 130])
def test_instant_counts_around_the_fold(det, many, n):
    rig = many.subset(instants=range(n))
    out, ref = run_device(det, rig, RC.off_extrinsics(rig.E), iterations=2, damping=1e-3)
    assert ref["status"] == RC.OK and ref["n_instants_used"] == n
    assert_same_bytes(out, ref, "n = %d" % n)


@pytest.mark.parametrize("n_cams", [2, 3, 8])
def test_camera_counts_and_mixed_lenses(det, n_cams):
    cams = [CC.CAMERAS[RC.LENSES[c % 3]] for c in range(n_cams)]
    rig = RC.Rig(cams, RC.true_extrinsics(n_cams), CC.poses(5), noise=0.1)
    out, ref = run_device(det, rig, RC.off_extrinsics(rig.E), iterations=3)
    assert ref["status"] == RC.OK and ref["n_cams_free"] == n_cams - 1 and ref["best_iter"] > 0
    assert_same_bytes(out, ref, "%d cameras" % n_cams)


def test_table_sizes(det):
    """tables of 1, 4, 64, 65 and 587 rows of a 64 x 64 layout, tags_per_frame 600, in one 2-camera call"""
    ids = np.random.RandomState(7).permutation(4096)[:587]
    sizes = (1, 4, 64, 65, 587)
    T = CC.poses(5)
    T[:, 9:] *= 2.2  # (the board is 0.83 units wide)
    table_ids = {(c, s): ids[:sizes[(s + c) % 5]] for c in range(2) for s in range(5)}
    rig = RC.Rig([CC.CAMERAS["radtan"]] * 2, RC.true_extrinsics(2), T, noise=0.05, ids=table_ids, tpf=600, cols=64, rows=64, tag_size=0.01)
    out, ref = run_device(det, rig, RC.off_extrinsics(rig.E), iterations=3)
    assert ref["status"] == RC.OK and sorted(ref["frame_n_raw"][:5]) == [4, 16, 256, 260, 2348]
    assert_same_bytes(out, ref, "table sizes")


@pytest.mark.parametrize("min_cams", [1, 2])
def test_unusable_frames_instants_and_a_held_camera(det, min_cams):
    rig = RC.three_rig(noise=0.1).subset()
    rig.fit_status = rig.fit_status.copy()
    rig.fit_status[0, 0] = _ffi.AGX_FIT_SINGULAR   # the first frame
    rig.fit_status[1, 3] = _ffi.AGX_FIT_FEW        # a middle one
    rig.fit_status[2, 7] = _ffi.AGX_FIT_SINGULAR   # the last
    rig.fit_status[:, 5] = _ffi.AGX_FIT_FEW        # a whole instant
    rig.fit_status[0, 6] = rig.fit_status[2, 6] = _ffi.AGX_FIT_FEW  # an instant seen by camera 1 only
    seed = RC.off_extrinsics(rig.E)
    out, ref = run_device(det, rig, seed, iterations=4, min_cams=min_cams)
    assert ref["status"] == RC.OK and ref["n_instants_used"] == (7 if min_cams == 1 else 6)
    assert_same_bytes(out, ref, "unusable frames, min_cams %d" % min_cams)
    rig.fit_status[2, :] = _ffi.AGX_FIT_FEW        # camera 2 is held
    out, ref = run_device(det, rig, seed, iterations=4, min_cams=min_cams)
    assert ref["status"] == RC.OK and ref["n_cams_free"] == 1 and out["extrinsics"][2].tobytes() == seed[2].tobytes() and out["cam_n"][2] == 0
    assert_same_bytes(out, ref, "a held camera, min_cams %d" % min_cams)


@pytest.mark.parametrize("iterations,damping,alias", [(0, 0.0, False), (1, 1e-3, True), (7, 0.0, True), (7, 1e-3, False)])
def test_iterations_damping_alias(det, iterations, damping, alias):
    rig = RC.three_rig(noise=0.1)
    out, ref = run_device(det, rig, RC.off_extrinsics(rig.E), alias=alias, iterations=iterations, damping=damping)
    assert ref["status"] == RC.OK and (ref["best_iter"] > 0) == (iterations > 0)
    assert_same_bytes(out, ref, "iterations %d damping %g alias %s" % (iterations, damping, alias))


@pytest.mark.parametrize("case", ["RISES_THEN_LEAVES", "RISES_FINITE"])
def test_a_cost_that_rises_keeps_the_best_iterate(det, case):
    """tests/test_rig_cpu.py's two cases: the best iterate is 1 of the 2 that ran (then +inf), and 0 of 12 (every later cost far
    above): the device keeps that iterate's extrinsics, rig poses and frame costs across the worse ones"""
    rig = RC.stereo_rig(noise=0.1)
    seed = RC.off_extrinsics(rig.E, **RC.RISES_SEED)
    out, ref = run_device(det, rig, seed, iterations=12, **getattr(RC, case))
    want = 1 if case == "RISES_THEN_LEAVES" else 0
    assert ref["status"] == RC.OK and ref["best_iter"] == want < ref["iterations_run"]
    assert_same_bytes(out, ref, case)
    at, _ = run_device(det, rig, seed, iterations=want, **getattr(RC, case))  # that iterate's bytes, by a run that ends there
    for k in ("extrinsics", "rig_pose", "frame_cost", "frame_n"):
        assert out[k].tobytes() == at[k].tobytes(), k


def test_few_and_singular_leave_every_array_but_the_report(det, many):
    rig = many.subset(instants=range(3))
    seed = RC.off_extrinsics(rig.E)
    out, ref = run_device(det, rig, seed, iterations=2, min_instants=4)
    assert ref["status"] == RC.FEW
    assert_same_bytes(out, ref, "few")
    assert np.isnan(out["extrinsics"]).all() and np.isnan(out["rig_pose"]).all() and (out["frame_n"] == -1).all() and (out["cam_n"] == -1).all()
    cams = [CC.CAMERAS["radtan"]] * 4
    groups = RC.Rig(cams, RC.true_extrinsics(4), CC.poses(6), missing={(c, s) for c in range(4) for s in range(6) if (c < 2) != (s < 3)})
    out, ref = run_device(det, groups, RC.off_extrinsics(groups.E), iterations=3)
    assert ref["status"] == RC.SINGULAR
    assert_same_bytes(out, ref, "two groups")
    assert np.isnan(out["extrinsics"]).all() and np.isnan(out["rig_pose"]).all() and np.isnan(out["frame_cost"]).all() and (out["frame_n"] == -1).all()


def test_argument_rules_keep_the_batch_in_flight(det, many):
    import torch
    rig = many.subset(instants=range(3))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")
    frames = z((1, 64, 64), torch.uint8)
    tags = dev(rig.tags.view(np.int32).reshape(2, 3, rig.tpf, 9))
    ext = dev(RC.off_extrinsics(rig.E))
    args = dict(tags=tags, n_tags=dev(rig.counts.view(np.int32)), cols=6, rows=6, cameras=rig.cams, pose_in=dev(rig.pose),
                row_status=dev(rig.row_status.view(np.int32)), fit_status=dev(rig.fit_status.view(np.int32)), extrinsics_in=ext, extrinsics=ext,
                rig_pose=z((3, 12), torch.float64), frame_cost=z((2, 3), torch.float32), frame_n=z((2, 3), torch.int32), cam_n=z(2, torch.int32),
                report=z(70, torch.float64), tag_size=CC.TAG_SIZE)
    bad = [dict(damping=-1.0), dict(damping=float("nan")), dict(iterations=65), dict(min_tags=0), dict(min_cams=0), dict(min_instants=0), dict(tag_size=0.0),
           dict(cols=0), dict(cols=65, rows=64), dict(spacing_ratio=-1.0), dict(cameras=[rig.cams[0], A.Camera(0.0, 400.0, 400.0, 300.0)]),
           dict(cameras=[A.Camera.double_sphere(250.0, 250.0, 400.0, 300.0, 0.0, 1.5), rig.cams[1]])]
    for kw in bad:
        det.saddles_batch_enqueue(frames)
        with pytest.raises(A.AgxError) as e:
            det.rig_calibrate_enqueue(**dict(args, **kw))
        assert e.value.status == _ffi.AGX_ERR_ARG, kw
        det.saddles_batch_fetch()  # the batch in flight stayed where it was
    with pytest.raises(A.AgxError):
        det.rig_calibrate_enqueue(**dict(args, report=z(69, torch.float64)))
    with pytest.raises(A.AgxError):
        det.rig_calibrate_enqueue(**dict(args, cameras=rig.cams[:1]))
    lib, h = _ffi.lib(), det._h
    from aprilgrid_rs_amd.detector import _rig_cameras
    models, cams = _rig_cameras(rig.cams, 2)
    ptrs = [args[k].data_ptr() for k in ("pose_in", "row_status", "fit_status", "extrinsics_in", "extrinsics", "rig_pose", "frame_cost", "frame_n", "cam_n",
                                         "report")]

    def raw(nc=2, ns=3, tpf=rig.tpf, flags=0, p=ptrs, m=models, cam=cams):
        return lib.agx_rig_calibrate_enqueue(h, nc, ns, tags.data_ptr(), tpf, args["n_tags"].data_ptr(), None, 6, 6, 0, 0.3, CC.TAG_SIZE, m, cam, 0.0, 1, 1,
                                             2, 1, flags, *p)
    assert raw() == _ffi.AGX_OK
    for kw in (dict(nc=1), dict(nc=9), dict(ns=0), dict(nc=8, ns=8192), dict(tpf=0), dict(flags=2), dict(cam=None), dict(m=None),
               dict(p=ptrs[:9] + [ptrs[9] + 4]), dict(p=[ptrs[0] + 4] + ptrs[1:]), dict(p=ptrs[:6] + [ptrs[6] + 2] + ptrs[7:])) + \
            tuple(dict(p=ptrs[:i] + [None] + ptrs[i + 1:]) for i in range(10)):
        det.saddles_batch_enqueue(frames)
        assert raw(**kw) == _ffi.AGX_ERR_ARG, kw
        det.saddles_batch_fetch()  # the batch in flight stayed where it was
    det.sync()


def test_rig_calibrate_batch_on_rendered_frames(det):
    """Render 2 cameras x 4 instants on the device from known E_1 and T_s, calibrate the rig on the device, and compare with the
    composition of the host forms on the fetched tables, byte for byte."""
    import torch
    cam, E, T = RC.render_case()
    poses = np.array([RC.compose(E[c], T[s]) for c in range(2) for s in range(4)])
    frames = torch.zeros((8, 240, 320), dtype=torch.uint8, device="cuda:0")
    truth, n_truth, status = (torch.zeros((8, 16, 9), dtype=torch.int32, device="cuda:0"), torch.zeros(8, dtype=torch.int32, device="cuda:0"),
                              torch.zeros(8, dtype=torch.int32, device="cuda:0"))
    det.render_boards_enqueue(frames, 4, 4, cam, torch.from_numpy(poses).cuda(), truth, n_truth, status, tag_size=CC.TAG_SIZE)
    kw = dict(tag_size=CC.TAG_SIZE, rounds=2, iterations=10)
    ext, rig_pose, report = det.rig_calibrate_batch(frames.view(2, 4, 240, 320), 4, 4, [cam, cam], **kw)
    assert report["status"] == RC.OK and report["n_instants_used"] >= 3
    want, want_pose, want_report = RC.host_rig_batch(det, frames.view(2, 4, 240, 320), 4, 4, [cam, cam], **kw)
    got = ext.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    used = (report["frame_n"] > 0).all(axis=0)
    assert rig_pose.cpu().numpy()[used].tobytes() == want_pose[used].tobytes()
    assert report["cost"].tobytes() == want_report["cost"].tobytes()
    base = float(np.linalg.norm(got[1, 9:]))
    print("baseline", base, "rendered with", float(np.linalg.norm(E[1, 9:])), "rms", report["rms"])
    assert abs(base - float(np.linalg.norm(E[1, 9:]))) <= RC.BASELINE_MARGIN
