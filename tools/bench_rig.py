"""Device time of agx_rig_calibrate_enqueue (k_rig_blocks, k_rig_instants, k_rig_solve) at 2 cameras x 128 instants x 36 tags and
at 8 cameras x 32 instants, per whole call and per round of the three launches, beside agx_calibrate_enqueue with every camera
double held on the same 256 tables in the same run, for scale.  One GPU, one process.

The tables: tools/bench_board_pose.py's boards -- the 36 tags of a 6 x 6 board under one tilted pose per instant (rig from board),
seen by camera c through E_c (a baseline of 0.1 c units and a few degrees of toe-in), projected in numpy float64 through the
radial-tangential camera of that tool, moved by +-0.1 px, rounded to binary32, resident on the device.  k_board_pose runs once
per camera at 10 iterations and leaves the poses, masks and statuses the call reads in place; the seed extrinsics are
rig_seed's.  agx_rig_calibrate_enqueue is timed at iterations 1, 5 and 10; a call is 3 (iterations + 1) launches; "per_round" is
the difference of the calls at 10 and at 5 iterations over 5 -- one blocks + instants + solve round, without the call's fixed part.

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_calibrate.py takes them; the median.  The event pair's own cost is reported next to the readings and is NOT
subtracted.  Nothing is gated on these times.

  python tools/bench_rig.py [--reps 20] [--warmup 3] [--out profiles/rig.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_board_pose as BP  # the tables, the layout and the median

COLS, ROWS, T, TAG_SIZE = BP.COLS, BP.ROWS, BP.T, BP.TAG_SIZE
ITERATIONS = (1, 5, 10)
SHAPES = ((2, 128), (8, 32))


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def extrinsics(n_cams):
    out = np.zeros((n_cams, 12))
    for c in range(n_cams):
        R = rodrigues(np.radians([0.0, 3.0 * c * (1 if c % 2 else -1), 1.0 * c]))
        out[c] = np.concatenate([R.reshape(9), [-0.1 * c if c % 2 else 0.1 * c, 0.01 * c, 0.0]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    if not torch.cuda.is_available():
        sys.exit("bench_rig needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    cam = A.Camera(400.0, 400.0, 400.0, 300.0, -0.3, 0.1)
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    filler = torch.empty(1 << 28, **i32)  # 1 GiB

    def timed(call, reps=args.reps, warmup=args.warmup):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            filler.zero_()
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            us.append(1000.0 * a.elapsed_time(b))
        return us

    result = {"tool": "tools/bench_rig.py", "device": torch.cuda.get_device_name(0), "width": BP.W, "height": BP.H, "tags_per_frame": T,
              "layout": [ROWS, COLS], "reps": args.reps, "warmup": args.warmup, "damping": 0.0}
    result["event_pair_alone"] = BP.med(timed(lambda: None))
    for nc, ns in SHAPES:
        F = nc * ns
        E = extrinsics(nc)
        table = rig_tables(BP, cam, E, ns, np.random.RandomState(1))
        table = torch.from_numpy(table).to(dev)
        ntags = torch.full((F,), T, **i32)
        shared = dict(err_sq=torch.zeros((F, T), **f32), row_status=torch.zeros((F, T), **i32), n_inliers=torch.zeros(F, **i32), rms=torch.zeros(F, **f32),
                      pred=torch.zeros((F, T, 9), **i32), n_pred=torch.zeros(F, **i32), status=torch.zeros(F, **i32))
        pose_in, best = torch.zeros((F, 12), **f64), torch.zeros(F, **i32)
        det.board_pose_enqueue(table, ntags, COLS, ROWS, cam, pose=pose_in, best_iter=best, tag_size=TAG_SIZE, iterations=10, max_err_sq=1e12, **shared)
        torch.cuda.synchronize()
        seed = A.rig_seed(pose_in.cpu().numpy().reshape(nc, ns, 12), shared["status"].cpu().numpy().reshape(nc, ns))["extrinsics"]
        ext_in, ext, rig_pose = torch.from_numpy(seed).to(dev), torch.zeros((nc, 12), **f64), torch.zeros((ns, 12), **f64)
        cost, fn, cam_n, rep = torch.zeros((nc, ns), **f32), torch.zeros((nc, ns), **i32), torch.zeros(nc, **i32), torch.zeros(70, **f64)
        tag = "%dx%d" % (nc, ns)
        calls = {}
        for it in ITERATIONS:
            def call():
                det.rig_calibrate_enqueue(table.view(nc, ns, T, 9), ntags.view(nc, ns), COLS, ROWS, [cam] * nc, pose_in.view(nc, ns, 12),
                                          shared["row_status"].view(nc, ns, T), shared["status"].view(nc, ns), ext_in, ext, rig_pose, cost, fn, cam_n, rep,
                                          tag_size=TAG_SIZE, iterations=it)

            name = "rig_%s_iterations_%d" % (tag, it)
            calls[it] = result[name] = BP.med(timed(call))
            result[name]["launches"] = 3 * (it + 1)
            torch.cuda.synchronize()
            r = A.rig_report(rep.cpu().numpy())
            result[name + "_outcome"] = {k: r[k] for k in ("status", "best_iter", "iterations_run", "n_instants_used", "n_frames_used", "n_corners")}
            result[name + "_outcome"]["rms_px"] = round(r["rms"], 4)
        result["rig_%s_per_round" % tag] = {"us_median": round((calls[10]["us_median"] - calls[5]["us_median"]) / 5.0, 2)}
        if (nc, ns) == SHAPES[0]:  # for scale: the single-camera calibration with every camera double held, the same 256 tables
            cam_out, pose, c1, n1, rep1 = torch.zeros(9, **f64), torch.zeros((F, 12), **f64), torch.zeros(F, **f32), torch.zeros(F, **i32), torch.zeros(69, **f64)
            for it in ITERATIONS:
                def call():
                    det.calibrate_enqueue(table, ntags, COLS, ROWS, cam, pose_in, shared["row_status"], shared["status"], cam_out, pose, c1, n1, rep1,
                                          tag_size=TAG_SIZE, fixed=0x1ff, iterations=it)

                result["calibrate_held_%d_frames_iterations_%d" % (F, it)] = BP.med(timed(call))
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def rig_tables(BP, cam, E, ns, rng):
    """[C * ns, T, 9] int32: camera c's table at instant s is the board under E_c o T_s, T_s the poses bench_board_pose draws"""
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    nc = len(E)
    out = np.zeros((nc * ns, T), A.TagDetector.TAG_DTYPE)
    s_ratio = float(np.float32(0.3))
    pitch = 1.0 + s_ratio
    bw, bh = COLS * pitch - s_ratio, ROWS * pitch - s_ratio
    ox, oy = np.array([0.0, 1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0, 1.0])
    ids = np.arange(T)
    X = ((ids % COLS)[:, None] * pitch + ox[None, :] - bw / 2.0) * TAG_SIZE
    Y = ((ids // COLS)[:, None] * pitch + oy[None, :] - bh / 2.0) * TAG_SIZE
    P = np.stack([X, Y, np.zeros_like(X)], axis=-1).reshape(-1, 3)
    for s in range(ns):
        R, t = A.board_pose_looking_at(0.45 + 0.2 * rng.rand(), rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-90, 90),
                                       (rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)))
        for c in range(nc):
            Rc, tc = E[c, :9].reshape(3, 3), E[c, 9:]
            Q = (P @ R.T + t) @ Rc.T + tc
            uv = np.zeros((len(Q), 2))
            st = _ffi.lib().agx_debug_pose_project(cam.model, cam.as_doubles(), np.ascontiguousarray(Q).ctypes.data, len(Q), uv.ctypes.data)
            assert st == 0
            uv = uv + rng.uniform(-0.1, 0.1, uv.shape)
            out[c * ns + s]["id"] = ids
            out[c * ns + s]["xy"] = uv.reshape(T, 8).astype(np.float32)
    return out.view(np.int32).reshape(nc * ns, T, 9)


if __name__ == "__main__":
    main()
