"""The saddle chain at a blur sigma other than 1.5 (agx_detector_set_blur_sigma) at the benchmark's geometry: 256 L8 frames of
1280 x 800 from synth.render_batch, resident on the device.  One GPU, one process.  Per sigma -- 1.5 (the fused kernel K1 in
front) and 1.0, 2.0, 4.0 (k_gauss_blur + k_response_front in front) -- WARMUP batches, then REPS (at least 20) readings of

  chain     agx_saddles_batch_enqueue_to, one batch between two events on the stream, profiling off;
  blur      k_gauss_blur alone at that sigma on the same frames (agx_planes_enqueue into a tight plane: the launch the chain
            makes), between two events;
  sparse    the sparse stages of one batch of the chain, the sum of the library's own event pairs around their launches
            (agx_profile_enable(det, 2); an event pair opens a gap on the stream, so this reading is taken in batches of its own);
  k1        at sigma 1.5 only: K1, by the library's event pair (agx_profile_enable(det, 1)).

The median of each.  agx_profile_* does not time the any-sigma front's launches, so the response front's two launches are what
is left of a batch: front = chain - blur - sparse, medians, stated as a difference (it also holds the gaps between launches).

  python tools/bench_sigma.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/sigma_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
SIGMAS = (1.5, 1.0, 2.0, 4.0)
SPARSE = ("k_verify_seeds", "k_flood_refine", "k_rare_emit", "k_sparse_frame")


def med(us):
    us = sorted(us)
    return {"us_per_batch_median": round(statistics.median(us), 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1)}


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
    from aprilgrid_rs_amd import sharding, synth
    if not torch.cuda.is_available():
        sys.exit("bench_sigma needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    plane = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    out, table = sharding.alloc_result_buffers(F, dev)
    det = A.TagDetector("t36h11", None, device=0)
    result = {"tool": "tools/bench_sigma.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H, "format": "L8",
              "reps": args.reps, "warmup": args.warmup, "sigmas": []}

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        pairs = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        return [1000.0 * a.elapsed_time(b) for a, b in pairs]

    def profiled(level, names):
        det.sync()
        det.profile_enable(level)
        us = []
        for _ in range(args.reps):
            det.profile_reset()
            det.saddles_batch_enqueue_to(frames, out, table)
            r = det.profile_read()
            us.append(1000.0 * sum(r[n][0] for n in names if n in r))
        det.profile_enable(0)
        return us

    for sigma in SIGMAS:
        det.set_blur_sigma(sigma)
        row = {"sigma": sigma, "radius": (len(A.blur_weights(sigma)) - 1) // 2}
        row["chain"] = med(timed(lambda: det.saddles_batch_enqueue_to(frames, out, table)))
        torch.cuda.synchronize()
        row["front"] = det.get_option("last_chain_front")
        row["sparse_path"] = det.get_option("last_sparse_path")
        t = table.cpu().numpy()
        assert (t[:, 2] == 0).all()
        row["saddles"] = int(t[:, 0].sum())
        row["sparse"] = med(profiled(2, SPARSE))
        if row["front"] == 0:
            row["k1"] = med(profiled(1, ("k_blur_hessian",)))
        else:
            row["blur"] = med(timed(lambda: det.planes_enqueue(frames, sigma, blur=plane)))
            row["response_front_by_difference_us"] = round(row["chain"]["us_per_batch_median"] - row["blur"]["us_per_batch_median"]
                                                           - row["sparse"]["us_per_batch_median"], 1)
            # the response front reads the blur plane twice and writes the mask and cand_max: bytes per batch it has to move
            row["response_front_bytes"] = F * (2 * 4 * W * H + 4 * ((H + 31) // 32) * W + ((H + 31) // 32) * W)
        result["sigmas"].append(row)
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
