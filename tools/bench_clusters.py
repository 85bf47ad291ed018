"""agx_clusters_enqueue at the benchmark's geometry: 256 L8 frames of 1280 x 800 from synth.render_batch, their Hessian response
at sigma 1.5 by agx_planes_enqueue, resident on the device.  One GPU, one process.  WARMUP batches, then REPS (at least 20)
readings, the median of each:

  entry        agx_clusters_enqueue into caller-owned arrays (rows, points, counts, statuses), one batch between two events on
               the stream, profiling off;
  plane_front  k_plane_front's two launches, and
  emit         k_emit_clusters, by the library's own event pairs (agx_profile_enable(det, 2); options "last_clusters_front_us" /
               "last_clusters_emit_us"), in batches of their own;
  chain        beside them a sigma-2.5 / half_size_patch-3 chain batch (agx_saddles_batch_enqueue_to) in the same run: the whole
               batch between the tool's events; at level 2 k_response_front's two launches by the library's event pair (option
               "last_response_front_us") and the cluster-only sparse stages as agx_profile_read times them (k_verify_seeds,
               k_flood_refine without the refinement);
  plane_front_minus_response_front
               the difference of the two fronts' medians beside the larger of their max - min in this run.

  python tools/bench_clusters.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/clusters_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
CPF = 4096


def med(us):
    us = sorted(us)
    return {"us_per_batch_median": round(statistics.median(us), 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="JSON file whose key \"bench_clusters\" receives the result (other keys are kept)")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import sharding, synth
    if not torch.cuda.is_available():
        sys.exit("bench_clusters needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    resp = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    det.planes_enqueue(frames, 1.5, response=resp)
    rows = torch.zeros((F, CPF, 4), dtype=torch.int32, device=dev)
    pts = torch.zeros((F, CPF, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    status = torch.zeros(F, dtype=torch.int32, device=dev)
    result = {"tool": "tools/bench_clusters.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "response": "agx_planes_enqueue at sigma 1.5", "clusters_per_frame": CPF, "reps": args.reps, "warmup": args.warmup}

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

    enqueue = lambda: det.clusters_enqueue(resp, clusters=rows, points=pts, counts=counts, status=status)
    result["entry"] = med(timed(enqueue))
    det.clusters_fetch()
    assert (status.cpu().numpy() == 0).all()
    result["clusters"] = int(counts.cpu().numpy().sum())
    det.profile_enable(2)
    front, emit = [], []
    for _ in range(args.reps):
        enqueue()
        det.clusters_fetch()
        front.append(float(det.get_option("last_clusters_front_us")))
        emit.append(float(det.get_option("last_clusters_emit_us")))
    det.profile_enable(0)
    result["plane_front"] = med(front)
    result["emit"] = med(emit)
    # the chain at sigma 2.5 / half_size_patch 3 in the same run: the any-sigma front and the cluster-only sparse stages
    det.set_blur_sigma(2.5)
    det.set_half_size_patch(3)
    out, table = sharding.alloc_result_buffers(F, dev)
    chain = lambda: det.saddles_batch_enqueue_to(frames, out, table)
    row = {"sigma": 2.5, "half_size_patch": 3, "chain": med(timed(chain))}
    torch.cuda.synchronize()
    row["clusters"] = int(table.cpu().numpy()[:, 3].sum())
    det.profile_enable(2)
    per, resp_front = {}, []
    for _ in range(args.reps):
        det.profile_reset()
        chain()
        det.sync()
        for name, (ms, n) in det.profile_read().items():
            if n:
                per.setdefault(name, []).append(1000.0 * ms)
        resp_front.append(float(det.get_option("last_response_front_us")))
    det.profile_enable(0)
    row["response_front"] = med(resp_front)
    row["profiled"] = {name: med(us) for name, us in per.items()}
    result["chain_sigma_2.5_half_3"] = row
    # the two fronts side by side: the difference of the medians against the spread (max - min) either one showed in this run
    a, b = result["plane_front"], row["response_front"]
    spread = max(a["us_max"] - a["us_min"], b["us_max"] - b["us_min"])
    diff = round(a["us_per_batch_median"] - b["us_per_batch_median"], 1)
    result["plane_front_minus_response_front"] = {"us": diff, "run_to_run_spread_us": round(spread, 1), "slower_beyond_spread": diff > spread}
    det.close()
    print(json.dumps(result))
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["bench_clusters"] = result
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
