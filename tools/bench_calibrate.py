"""Device time of agx_calibrate_enqueue (k_calib_blocks<LENS>, k_calib_solve) at 256 frames x 36 tags with 6 x 6 layouts, per
whole call and per launch pair, beside k_board_pose on the same tables in the same run.  One GPU, one process.

The tables: tools/bench_board_pose.py's -- the 36 tags of a 6 x 6 board under one tilted pose per frame, projected in numpy float64
through a strong-barrel radial-tangential camera, an equidistant camera and a double-sphere camera, moved by +-0.1 px, rounded to
binary32, resident on the device.  Per lens k_board_pose runs once at 10 iterations under a seed camera (focal lengths 5 % off,
principal point 10 px off; the lens's own distortion, so that every frame is posed) and leaves the poses, masks and statuses the
calibration reads in place; then agx_calibrate_enqueue is timed at iterations 1, 5 and 10 from that seed with every double of the
model free (radial-tangential: k3 held), damping 1e-6.  A call is 2 (iterations + 1) + 1 launches; "per_launch_pair" is the
difference of the calls at 10 and at 5 iterations over 5 -- one k_calib_blocks + k_calib_solve pair, without the call's fixed part.

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_board_pose.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time);
the median.  The event pair's own cost is reported next to the readings and is NOT subtracted.  Nothing is gated on these times.

  python tools/bench_calibrate.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/calibrate.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    if not torch.cuda.is_available():
        sys.exit("bench_calibrate needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    cams = {"radtan": A.Camera(400.0, 400.0, 400.0, 300.0, -0.3, 0.1),
            "equidistant": A.Camera.equidistant(400.0, 400.0, 400.0, 300.0, -0.013, 0.021, -0.013, 0.0026),
            "double_sphere": A.Camera.double_sphere(640.0, 640.0, 400.0, 300.0, 0.6, 0.45)}
    fixed = {"radtan": 0x100, "equidistant": 0, "double_sphere": 0}
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    ntags = torch.full((F,), T, **i32)
    shared = dict(err_sq=torch.zeros((F, T), **f32), row_status=torch.zeros((F, T), **i32), n_inliers=torch.zeros(F, **i32),
                  rms=torch.zeros(F, **f32), pred=torch.zeros((F, T, 9), **i32), n_pred=torch.zeros(F, **i32), status=torch.zeros(F, **i32))
    pose_in, best = torch.zeros((F, 12), **f64), torch.zeros(F, **i32)
    cam_out, pose, cost, fn, rep = torch.zeros(9, **f64), torch.zeros((F, 12), **f64), torch.zeros(F, **f32), torch.zeros(F, **i32), torch.zeros(69, **f64)
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

    result = {"tool": "tools/bench_calibrate.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": BP.W, "height": BP.H,
              "tags_per_frame": T, "layout": [ROWS, COLS], "reps": args.reps, "warmup": args.warmup, "damping": 1e-6}
    result["event_pair_alone"] = BP.med(timed(lambda: None))
    for k, cam in cams.items():
        table = torch.from_numpy(BP.tables(F, cam, np.random.RandomState(1))).to(dev)
        seed = type(cam)(cam[0] * 1.05, cam[1] * 0.95, cam[2] + 10.0, cam[3] - 10.0, *cam[4:])

        def pose_call():
            det.board_pose_enqueue(table, ntags, COLS, ROWS, seed, pose=pose_in, best_iter=best, tag_size=TAG_SIZE, iterations=10, max_err_sq=1e12,
                                   **shared)

        result["k_board_pose_%s_iterations_10" % k] = BP.med(timed(pose_call))
        torch.cuda.synchronize()
        calls = {}
        for it in ITERATIONS:
            def call():
                det.calibrate_enqueue(table, ntags, COLS, ROWS, seed, pose_in, shared["row_status"], shared["status"], cam_out, pose, cost, fn, rep,
                                      tag_size=TAG_SIZE, fixed=fixed[k], damping=1e-6, iterations=it)

            name = "calibrate_%s_iterations_%d" % (k, it)
            calls[it] = result[name] = BP.med(timed(call))
            result[name]["launches"] = 2 * (it + 1) + 1
            torch.cuda.synchronize()
            r = A.calib_report(rep.cpu().numpy())
            result[name + "_outcome"] = {"status": r["status"], "best_iter": r["best_iter"], "iterations_run": r["iterations_run"],
                                         "frames_used": r["n_frames_used"], "corners": r["n_corners"], "rms_px": round(r["rms"], 4),
                                         "rms_px_at_the_seed": round(float(np.sqrt(r["cost"][0] / max(r["n_corners"], 1))), 4)}
        result["calibrate_%s_per_launch_pair" % k] = {"us_median": round((calls[10]["us_median"] - calls[5]["us_median"]) / 5.0, 2)}
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
