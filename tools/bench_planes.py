"""k_gauss_blur (agx_planes_enqueue, blur only) at the benchmark's geometry: 256 L8 frames of 1280 x 800 resident on the device,
at sigma 1.5, 3.0 and 8.0 (radius 3, 6 and 16).  One GPU, one process.  Per sigma: WARMUP calls, then REPS (at least 20) calls
each between two events on the stream; the median, and the bytes the call has to move (one byte in and one float out per pixel)
over it.  Beside them K1's own time on the same batch (k_blur_hessian: the same blur at sigma 1.5 plus the Hessian, the minimum
and the candidate mask at the same traffic): the median of as many readings of agx_profile_enable(det, 1), one batch of the
whole chain each.  K1 is the library's own: the planes kernels were added beside it and K1's source and compiled code are
those of the commit before them, so no second build of the library is loaded for the yardstick.

  python tools/bench_planes.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/planes_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
SIGMAS = (1.5, 3.0, 8.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_planes needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    blur = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    nbytes = F * W * H * (1 + 4)
    result = {"tool": "tools/bench_planes.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H, "format": "L8",
              "reps": args.reps, "warmup": args.warmup, "bytes_per_batch": nbytes, "k_gauss_blur": []}
    for sigma in SIGMAS:
        for _ in range(args.warmup):
            det.planes_enqueue(frames, sigma, blur=blur)
        torch.cuda.synchronize()
        pairs = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            det.planes_enqueue(frames, sigma, blur=blur)
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        us = sorted(1000.0 * a.elapsed_time(b) for a, b in pairs)
        med = statistics.median(us)
        result["k_gauss_blur"].append({"sigma": sigma, "radius": (len(A.blur_weights(sigma)) - 1) // 2, "us_per_batch_median": round(med, 1),
                                       "us_min": round(us[0], 1), "us_max": round(us[-1], 1), "gb_per_s": round(nbytes / med / 1e3, 1)})
    # K1 of the whole chain on the same batch, timed by the library's own event pair around it
    for _ in range(args.warmup):
        det.saddles_batch_enqueue(frames)
    det.sync()
    det.profile_enable(1)
    k1_us = []
    for _ in range(args.reps):  # one batch per reading: the library's event pair around K1 of that batch
        det.profile_reset()
        det.saddles_batch_enqueue(frames)
        ms, launches = det.profile_read()["k_blur_hessian"]
        assert launches == 1
        k1_us.append(1000.0 * ms)
    det.profile_enable(0)
    k1_us.sort()
    k1 = statistics.median(k1_us)
    result["k1_blur_hessian"] = {"us_per_batch_median": round(k1, 1), "us_min": round(k1_us[0], 1), "us_max": round(k1_us[-1], 1),
                                 "gb_per_s": round(nbytes / k1 / 1e3, 1)}
    det.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
