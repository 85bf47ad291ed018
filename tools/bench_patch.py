"""The saddle chain at a half_size_patch other than 2 (agx_detector_set_half_size_patch) at the benchmark's geometry: 256 L8
frames of 1280 x 800 from synth.render_batch, resident on the device, blur sigma 1.5.  One GPU, one process.  Per configuration
-- half 2 as it always ran, half 2 under "chain_refine_general" (the deferred refinement with the default's results), half 1, 3
and 4 -- WARMUP batches, then REPS (at least 20) readings of

  chain     agx_saddles_batch_enqueue_to, one batch between two events on the stream, profiling off;
  k1        the blur kernel of one batch, by the library's event pair (agx_profile_enable(det, 1)), in batches of its own.

The median of each.  agx_profile_* does not time k_generic_cluster and k_refine_clusters, so the sparse stages -- everything
behind K1: verify, flood, generic clustering, refinement, emission and the gaps between them -- are what is left of the tool's
own bracket around the batch: sparse = chain - k1, medians, stated as a difference.

  python tools/bench_patch.py [--frames 256] [--reps 20] [--warmup 3] [--out FILE] [--merge-into profiles/chain_patch.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
CONFIGS = ((2, 0), (2, 1), (1, 0), (3, 0), (4, 0))  # (half_size_patch, "chain_refine_general")


def med(us):
    us = sorted(us)
    return {"us_per_batch_median": round(statistics.median(us), 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-into", default=None, help="JSON file whose key \"bench_patch\" receives the result")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import sharding, synth
    if not torch.cuda.is_available():
        sys.exit("bench_patch needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    out, table = sharding.alloc_result_buffers(F, dev)
    det = A.TagDetector("t36h11", None, device=0)
    result = {"tool": "tools/bench_patch.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H, "format": "L8",
              "sigma": 1.5, "reps": args.reps, "warmup": args.warmup, "configs": []}

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

    def profiled_k1():
        det.sync()
        det.profile_enable(1)
        us = []
        for _ in range(args.reps):
            det.profile_reset()
            det.saddles_batch_enqueue_to(frames, out, table)
            r = det.profile_read()
            us.append(1000.0 * r["k_blur_hessian"][0])
        det.profile_enable(0)
        return us

    for half, general in CONFIGS:
        det.set_half_size_patch(half)
        det.set_option("chain_refine_general", general)
        row = {"half_size_patch": half, "chain_refine_general": general}
        row["chain"] = med(timed(lambda: det.saddles_batch_enqueue_to(frames, out, table)))
        torch.cuda.synchronize()
        row["last_chain_refine"] = det.get_option("last_chain_refine")
        row["sparse_path"] = det.get_option("last_sparse_path")
        t = table.cpu().numpy()
        assert (t[:, 2] == 0).all()
        row["saddles"] = int(t[:, 0].sum())
        row["clusters"] = int(t[:, 3].sum())
        row["k1"] = med(profiled_k1())
        row["sparse_by_difference_us"] = round(row["chain"]["us_per_batch_median"] - row["k1"]["us_per_batch_median"], 1)
        result["configs"].append(row)
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if args.merge_into:
        doc = json.load(open(args.merge_into)) if os.path.exists(args.merge_into) else {}
        doc["bench_patch"] = result
        with open(args.merge_into, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
