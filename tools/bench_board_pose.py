"""Device time per launch of k_board_pose (agx_board_pose_enqueue) at 256 frames x 36 tags with 6 x 6 layouts, beside k_board_fit
on the same tables in the same run.  One GPU, one process.

The tables: the 36 tags of a 6 x 6 board (tag side 0.05, spacing 0.3) under one tilted pose per frame, projected in numpy float64
through the model -- once through a pinhole (fx = fy = 400 on 800 x 600), once through the same camera with k1 = -0.3, k2 = 0.1,
once through the same pinhole under the equidistant model with Kalibr-sized coefficients (Camera.equidistant: the kernel's
AGX_LENS_EQUIDISTANT instantiation; profiles/board_pose_equi.json holds three readings of this run beside the parent's figures),
once through a double-sphere camera of the same focal length near the axis (Camera.double_sphere, xi = 0.6, alpha = 0.45: the
AGX_LENS_DOUBLE_SPHERE instantiation; profiles/board_pose_ds.json)
-- moved by +-0.1 px and rounded to binary32; resident on the device.  k_board_pose is taken at iterations 0, 5 and 10 on
both, and at 10 with one row per frame stored under a wrong id and max_drop 1, which costs a second round; k_board_fit on the
pinhole tables with every tag predicted.

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_board_fit.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time);
the median.  The event pair's own cost is reported next to the readings and is NOT subtracted.

  python tools/bench_board_pose.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/board_pose.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, T = 800, 600, 36
COLS = ROWS = 6
TAG_SIZE, S = 0.05, 0.3


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def tables(n, cam, rng):
    """[n, 36, 9] int32 tag rows: id, then the four corners as float32 bits."""
    fx, fy, cx, cy, k1, k2 = cam[:6]
    t = np.arange(T)
    bw = COLS * (1 + S) - S
    X = ((t % COLS)[:, None] * (1 + S) + np.array([0, 1, 1, 0.0]) - bw / 2) * TAG_SIZE
    Y = ((t // COLS)[:, None] * (1 + S) + np.array([0, 0, 1, 1.0]) - bw / 2) * TAG_SIZE
    out = np.zeros((n, T, 9), np.int32)
    for f in range(n):
        a, b = np.radians(rng.uniform(-35, 35, 2))
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        R, tr = Ry @ Rx, np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.3, 0.5)])
        Q = np.stack([X, Y, np.zeros_like(X)], -1) @ R.T + tr
        x, y = Q[..., 0] / Q[..., 2], Q[..., 1] / Q[..., 2]
        r2 = x * x + y * y
        if getattr(cam, "model", 0) == 2:  # Camera.double_sphere: the model's own denominator in Z's place
            d1 = np.sqrt((Q ** 2).sum(-1))
            kk = cam[4] * d1 + Q[..., 2]
            den = cam[5] * np.sqrt(Q[..., 0] ** 2 + Q[..., 1] ** 2 + kk ** 2) + (1 - cam[5]) * kk
            x, y, rad = Q[..., 0] / den, Q[..., 1] / den, 1.0
        elif getattr(cam, "model", 0):  # Camera.equidistant: theta_d / r in rad's place
            th = np.arctan(np.sqrt(r2))
            rad = th * (1 + k1 * th ** 2 + k2 * th ** 4 + cam[6] * th ** 6 + cam[7] * th ** 8) / np.sqrt(r2)
        else:
            rad = 1 + k1 * r2 + k2 * r2 * r2
        uv = np.stack([fx * x * rad + cx, fy * y * rad + cy], -1) + rng.uniform(-0.1, 0.1, (T, 4, 2))
        out[f, :, 0] = t
        out[f, :, 1:] = uv.reshape(T, 8).astype(np.float32).view(np.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "board_pose.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    if not torch.cuda.is_available():
        sys.exit("bench_board_pose needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    cams = {"pinhole": A.Camera(400.0, 400.0, 400.0, 300.0), "barrel": A.Camera(400.0, 400.0, 400.0, 300.0, -0.3, 0.1),
            "equidistant": A.Camera.equidistant(400.0, 400.0, 400.0, 300.0, -0.013, 0.021, -0.013, 0.0026),
            "double_sphere": A.Camera.double_sphere(640.0, 640.0, 400.0, 300.0, 0.6, 0.45)}
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    table = {k: torch.from_numpy(tables(F, c, np.random.RandomState(1))).to(dev) for k, c in cams.items()}
    wrong = {k: v.clone() for k, v in table.items()}  # row 0 of every frame leaves, row 1 takes its id: one outlier a frame
    for v in wrong.values():
        v[:, 1, 0] = v[:, 0, 0]
        v[:, 0, 0] = 1000
    ntags = torch.full((F,), T, **i32)
    shared = dict(err_sq=torch.zeros((F, T), **f32), row_status=torch.zeros((F, T), **i32), n_inliers=torch.zeros(F, **i32),
                  rms=torch.zeros(F, **f32), pred=torch.zeros((F, T, 9), **i32), n_pred=torch.zeros(F, **i32), status=torch.zeros(F, **i32))
    pose, best, h = torch.zeros((F, 12), dtype=torch.float64, device=dev), torch.zeros(F, **i32), torch.zeros((F, 9), dtype=torch.float64, device=dev)
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

    def outcome():
        torch.cuda.synchronize()
        st = shared["status"].cpu().numpy()
        return {"frames_ok": int((st == 0).sum()), "frames_loose": int((st == 1).sum()), "frames_refused": int((st > 1).sum()),
                "inlier_rows": int(shared["n_inliers"].sum().item()),
                "rms_px_median": round(float(shared["rms"][shared["status"] < 2].median().item()), 4) if (st < 2).any() else None}

    result = {"tool": "tools/bench_board_pose.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "tags_per_frame": T, "layout": [ROWS, COLS], "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    for k, cam in cams.items():
        for it in (0, 5, 10):
            name = "k_board_pose_%s_iterations_%d" % (k, it)
            result[name] = med(timed(lambda: det.board_pose_enqueue(table[k], ntags, COLS, ROWS, cam, pose=pose, best_iter=best, tag_size=TAG_SIZE,
                                                                    iterations=it, **shared)))
            result[name + "_outcome"] = outcome()
        name = "k_board_pose_%s_one_wrong_id_two_rounds" % k
        result[name] = med(timed(lambda: det.board_pose_enqueue(wrong[k], ntags, COLS, ROWS, cam, pose=pose, best_iter=best, tag_size=TAG_SIZE,
                                                                iterations=10, max_drop=1, **shared)))
        result[name + "_outcome"] = outcome()
    for k in cams:
        name = "k_board_fit_%s_tables" % k
        result[name] = med(timed(lambda: det.board_fit_enqueue(table[k], ntags, COLS, ROWS, (W, H), h=h, **shared)))
        result[name + "_outcome"] = outcome()
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
