"""Device time per batch of k_render_boards (agx_render_boards_enqueue) at 256 frames of 1280 x 800 -- a 6 x 6 board at 256 poses
that fill the frame to different degrees -- per lens model at supersample 1 and 3, beside a device-to-device copy of the same batch
in the same run (the floor for one byte out per pixel is half of it) and, for orientation only and not as a gate,
synth.render_batch(device="cuda") at its supersample 3 (torch ops through a pinhole homography, blur and noise included; timed on
--synth-frames frames with wall-clock time around a synchronize, because it runs hundreds of launches a frame).  One GPU, one
process.

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_rectify.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time); the
median.  The event pair's own cost is reported next to the readings and is NOT subtracted.

  python tools/bench_render.py [--frames 256] [--reps 20] [--warmup 3] [--synth-frames 16] [--out profiles/render.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--synth-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_render needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    cameras = {"radtan": A.Camera(900.0, 900.0, 640.0, 400.0, -0.18, 0.06, 0.001, -0.0015, 0.0),
               "equidistant": A.Camera.equidistant(420.0, 420.0, 640.0, 400.0, -0.013, 0.021, -0.013, 0.0026),
               "double_sphere": A.Camera.double_sphere(672.0, 672.0, 640.0, 400.0, 0.6, 0.45)}
    # the board's distance puts it at 40 .. 90 % of the frame's height through the pinhole part of each camera
    rng = np.random.default_rng(7)
    fill = rng.uniform(0.4, 0.9, F)
    angles = rng.uniform(-25.0, 25.0, (F, 2))
    rolls = rng.uniform(-180.0, 180.0, F)

    def poses(cam, scale):
        fy = float(cam[1]) / scale
        return A.pose_rows([A.board_pose_looking_at(8.1 * fy / (fill[f] * H), angles[f, 0], angles[f, 1], rolls[f]) for f in range(F)])

    det = A.TagDetector("t36h11", None, device=0)
    filler = torch.empty(1 << 28, dtype=torch.int32, device=dev)  # 1 GiB

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

    result = {"tool": "tools/bench_render.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "layout": "6 x 6", "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    frames = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    other = torch.empty_like(frames)
    truth = torch.zeros((F, 36, 9), dtype=torch.int32, device=dev)
    n_truth, status = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    for name, cam in cameras.items():
        scale = 1.6 if name == "double_sphere" else 1.0  # (fx = f (1 + xi) near the axis)
        p = torch.from_numpy(poses(cam, scale)).to(dev)
        for S in (1, 3):
            key = "k_render_boards_%s_s%d" % (name, S)
            result[key] = med(timed(lambda: det.render_boards_enqueue(frames, 6, 6, cam, p, truth, n_truth, status, supersample=S)))
            torch.cuda.synchronize()
            assert int((status != 0).sum()) == 0, "a frame was not rendered"
            result[key]["share_of_pixels_on_the_page"] = round(float((frames != 128).float().mean().item()), 4)
            result[key]["ns_per_sample"] = round(1000.0 * result[key]["us_median"] / (F * H * W * S * S), 4)
        # two frames of the batch against the host form
        det.render_boards_enqueue(frames[:2], 6, 6, cam, p[:2], truth[:2], n_truth[:2], status[:2], supersample=2)
        torch.cuda.synchronize()
        ref = A.render_boards((W, H), 6, 6, cam, p[:2].cpu().numpy(), supersample=2)[0]
        assert frames[:2].cpu().numpy().tobytes() == ref.tobytes(), "k_render_boards differs from the host form"
    result["copy_d2d_l8"] = med(timed(lambda: other.copy_(frames)))
    del other, frames
    n = args.synth_frames
    synth.render_batch(0, 1, W, H, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    synth.render_batch(0, n, W, H, device="cuda")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    result["synth_render_batch_supersample_3"] = {"frames": n, "wall_us": round(1e6 * wall, 1), "wall_us_scaled_to_the_batch": round(1e6 * wall * F / n, 1),
                                                  "note": "orientation only: torch ops, pinhole, blur and noise included, host launch time included"}
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
