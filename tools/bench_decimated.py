"""Device time of the coarse-to-fine path at 256 frames of 1280 x 800 (the benchmark's seeded boards, 16 distinct frames tiled):

  k_decimate            per launch at factor 2, 3, 4 (AGX_L8), beside a device-to-device copy of the batch in the same run
  k_refine_windows      at 144, 1024, 4096 and 16384 points a frame, beside the existing entry on the same points --
                        refine_points_enqueue(image="blurred"): the front end, K1 with its blur plane, k_refine_points -- with
                        the bytes of the two compared; the first of these counts at which the windowed entry stops winning
  detect_decimated      at factor 2 per batch, beside detect_staged on the same frames (host wall time around the call, which
                        ends with its own synchronisation: both have host steps between their launches)

The points: the frame's own saddles (saddles_batch_fetch) moved by up to a pixel, repeated to the count.  Per figure WARMUP
runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as tools/bench_rectify.py takes them
(a 1 GiB fill queued in front of the first event, so that the reading is the device's time); the median.  The event pair's own
reading is reported and NOT subtracted.  tests/test_gpu_detect_decimated.py's scene is measured too: e_full, the error at factor
2 .. 4 and the share of corners whose bytes equal the full-resolution result.  One GPU, one process.

  python tools/bench_decimated.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/decimated.json]
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
UNIQUE = 16
POINT_COUNTS = (144, 1024, 4096, 16384)


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def accuracy(det):
    """the end-to-end test's scene: one 6 x 6 board at 1280 x 960 -> the errors against the truth rows, in px"""
    import torch
    import aprilgrid_rs_amd as A
    from tests import render_cases as RC
    from tests.test_gpu_detect_decimated import SIZE, camera, corner_error
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda:0")
    frames = torch.zeros((1, SIZE[1], SIZE[0]), dtype=torch.uint8, device="cuda:0")
    poses = torch.from_numpy(A.pose_rows([RC.looking_at(RC.TRIP_POSE)])).cuda()
    truth, n_truth, status = i32(1, 36, 9), i32(1), i32(1)
    det.render_boards_enqueue(frames, 6, 6, camera(), poses, truth, n_truth, status, supersample=4)
    det.sync()
    xy = truth.cpu().numpy().view(A.TagDetector.TAG_DTYPE).reshape(36)["xy"].reshape(36, 4, 2).astype(np.float64)
    full = det.detect_batch_device(frames)[0]
    out = {"scene": "6 x 6 board, 1280 x 960, tests/test_gpu_detect_decimated.py", "full_resolution": {"tags": len(full), "largest_corner_error_px": round(corner_error(full, xy), 4)}}
    for factor in (2, 3, 4):
        got = det.detect_decimated(frames, factor=factor)[0]
        same = sum(int(np.asarray(got[i][c]).tobytes() == np.asarray(full[i][c]).tobytes()) for i in got if i in full for c in range(4))
        out["factor_%d" % factor] = {"tags": len(got), "largest_corner_error_px": round(corner_error(got, xy), 4) if got else None,
                                     "corners_with_the_full_resolution_bytes": same, "of_corners": 4 * len(got),
                                     "share": round(same / (4 * len(got)), 4) if got else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decimated.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_decimated needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
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

    def walled(call, reps=args.reps, warmup=args.warmup):
        for _ in range(warmup):
            call()
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            us.append(1e6 * (time.perf_counter() - t0))
        return us

    result = {"tool": "tools/bench_decimated.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "distinct_frames": UNIQUE, "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    base, _ = synth.render_batch(0, UNIQUE, W, H, device="cuda:0")
    frames = base.repeat(((F + UNIQUE - 1) // UNIQUE, 1, 1))[:F].contiguous()

    # k_decimate beside a copy of the batch
    copy_dst = torch.empty_like(frames)
    result["copy_d2d_l8"] = med(timed(lambda: copy_dst.copy_(frames)))
    del copy_dst
    for factor in (2, 3, 4):
        out = torch.empty((F, H // factor, W // factor), dtype=torch.uint8, device=dev)
        t = med(timed(lambda: det.decimate_enqueue(frames, factor, out=out)))
        torch.cuda.synchronize()
        assert out[:2].cpu().numpy().tobytes() == A.decimate(frames[:2].cpu().numpy(), factor).tobytes(), "k_decimate differs from the host form"
        moved = F * (H // factor * factor) * (W // factor * factor) + out.numel()
        result["k_decimate_l8_factor_%d" % factor] = dict(t, bytes_in_and_out=moved, GBps=round(moved / t["us_median"] / 1e3, 1),
                                                          over_copy=round(t["us_median"] / result["copy_d2d_l8"]["us_median"], 3))
        del out

    # the windowed refine beside the existing entry, on the frames' own saddles moved by up to a pixel
    det.saddles_batch_enqueue(base)
    lists, _ = det.saddles_batch_fetch()
    rng = np.random.default_rng(1)
    result["saddles_per_distinct_frame"] = [int(len(l)) for l in lists]
    crossover = None
    for count in POINT_COUNTS:
        pts = np.zeros((F, count, 2), np.float32)
        for f in range(F):
            l = lists[f % UNIQUE]
            xy = np.stack([l["x"], l["y"]], axis=1) if len(l) else np.full((1, 2), 100.0, np.float32)
            pts[f] = xy[np.arange(count) % len(xy)] + rng.uniform(-1.0, 1.0, (count, 2)).astype(np.float32)
        d_pts = torch.from_numpy(pts).to(dev)
        outs = [(torch.zeros((F, count, 5), dtype=torch.float32, device=dev), torch.zeros((F, count), dtype=torch.int32, device=dev)) for _ in range(2)]
        t_win = med(timed(lambda: det.refine_windows_enqueue(frames, d_pts, outs[0][0], outs[0][1])))
        t_old = med(timed(lambda: det.refine_points_enqueue(frames, d_pts, out=outs[1][0], status=outs[1][1], image="blurred")))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), \
            "k_refine_windows differs from the blurred entry"
        result["refine_%d_points_per_frame" % count] = {
            "k_refine_windows": t_win, "blurred_entry_front_k1_k_refine_points": t_old,
            "windows_over_blurred": round(t_win["us_median"] / t_old["us_median"], 3),
            "refined_share": round(float((outs[0][1] == 0).float().mean().item()), 4)}
        if crossover is None and t_win["us_median"] >= t_old["us_median"]:
            crossover = count
        del d_pts, outs
    result["windowed_entry_stops_winning_at_points_per_frame"] = crossover  # (null: it won at every count measured)

    # the whole detect, per batch
    t_staged = med(walled(lambda: det.detect_staged(frames)))
    t_dec = med(walled(lambda: det.detect_decimated(frames, factor=2)))
    staged, dec = det.detect_staged(frames[:UNIQUE]), det.detect_decimated(frames[:UNIQUE], factor=2)
    result["detect_staged_per_batch_wall"] = t_staged
    result["detect_decimated_factor_2_per_batch_wall"] = t_dec
    result["detect_decimated_over_staged"] = round(t_dec["us_median"] / t_staged["us_median"], 3)
    result["tags_found_on_the_distinct_frames"] = {"detect_staged": [len(t) for t in staged], "detect_decimated_factor_2": [len(t) for t in dec]}
    del frames, filler
    result["accuracy"] = accuracy(det)
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
