"""Device time of one k_init_quads launch (agx_init_quads_enqueue: the candidate quads of seed saddles, src/detector.rs:543-586)
with ONE caller seed per frame and with the reference's own 30 seeds, each at n_nearest 8 and 50, next to -- in the same run, on
the same saddle lists -- one k_find_boards launch (the whole search) and one k_grow_boards launch fed by the 1-seed output.
One GPU, one process.

The lists: 256 L8 frames of 1280 x 800 from synth.render_batch, resident on the device, through the staged chain (planes,
clusters, refine, the k / phi filter) in this process.  The caller seed of frame f is column 0 of the first quad of the board
k_find_boards found in it; frames without a board get no seed.

Per kernel WARMUP launches, then REPS (at least 20) readings of ONE launch between two events of the tool's own on the stream, as
tools/bench_grow.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time); the
median.  The event pair's own cost is reported next to the readings and is NOT subtracted.  The frames still AGX_BOARD_PENDING
before the fetch are counted per configuration.

  python tools/bench_init_quads.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/init_quads.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
Q, C, CPF = 128, 1024, 4096


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_quads.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_init_quads needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    blur = torch.empty((F, H, W), **f32)
    resp = torch.empty_like(blur)
    rows, pts = torch.zeros((F, CPF, 4), **i32), torch.zeros((F, CPF, 2), **f32)
    counts, cstatus = torch.zeros(F, **i32), torch.zeros(F, **i32)
    records, pstatus = torch.zeros((F, CPF, 5), **f32), torch.zeros((F, CPF), **i32)
    det.planes_enqueue(frames, det.blur_sigma, blur=blur, response=resp)
    det.clusters_enqueue(resp, clusters=rows, points=pts, counts=counts, status=cstatus)
    det.refine_points_enqueue(blur, pts, counts=counts, out=records, status=pstatus, image="plane")
    det.filter_saddles_enqueue(records, pstatus, counts=counts)
    quads, nq, bst = torch.zeros((F, Q, 4), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
    det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, n_quads=nq, status=bst)
    det.find_boards_fetch()
    det.sync()
    del blur, resp
    h_bst = bst.cpu().numpy()
    one_seed = quads[:, 0, :1].contiguous()  # [F, 1]: column 0 of a row is a saddle init_quads has quads for
    one_count = torch.from_numpy((h_bst == 0).astype(np.int32)).to(dev)
    cand, ncand, cst = torch.zeros((F, C, 4), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
    gquads, gnq, gst = torch.zeros((F, Q, 4), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
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

    def init(caller, k):
        if caller:
            return lambda: det.init_quads_enqueue(records, cand, ncand, cst, seed_saddles=one_seed, seed_counts=one_count, n_nearest=k,
                                                  counts=counts, point_status=pstatus)
        return lambda: det.init_quads_enqueue(records, cand, ncand, cst, seeds_per_frame=30, n_nearest=k, counts=counts, point_status=pstatus)

    find = lambda: det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, n_quads=nq, status=bst)
    grow = lambda: det.grow_boards_enqueue(records, cand, gquads, gnq, gst, counts=counts, point_status=pstatus, seed_counts=ncand,
                                           spacing_ratio=0.3, stop_score=0, fix_missing=True)

    result = {"tool": "tools/bench_init_quads.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "candidates_per_frame": C, "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    result["k_find_boards"] = med(timed(find))
    det.find_boards_fetch()
    result["k_init_quads"] = {}
    for name, caller, k in (("30_reference_seeds_n_nearest_50", False, 50), ("30_reference_seeds_n_nearest_8", False, 8),
                            ("1_caller_seed_n_nearest_8", True, 8), ("1_caller_seed_n_nearest_50", True, 50)):
        r = med(timed(init(caller, k)))
        torch.cuda.synchronize()
        h_cst, h_n = cst.cpu().numpy(), ncand.cpu().numpy()
        r["frames_pending_before_the_fetch"] = int((h_cst == 4).sum())
        det.init_quads_fetch()
        h_cst, h_n = cst.cpu().numpy(), ncand.cpu().numpy()
        r["frames_found"] = int((h_cst == 0).sum())
        r["quads_per_frame"] = {"min": int(h_n.min()), "median": float(np.median(h_n)), "max": int(h_n.max())}
        result["k_init_quads"][name] = r
    # cand / ncand now hold the 1-seed, n_nearest 50 output: the seeded grow's input as it stands
    result["k_grow_boards_fed_by_1_seed"] = med(timed(grow))
    torch.cuda.synchronize()
    result["k_grow_boards_fed_by_1_seed"]["frames_pending_before_the_fetch"] = int((gst.cpu().numpy() == 4).sum())
    det.grow_boards_fetch()
    result["k_grow_boards_fed_by_1_seed"]["frames_with_the_searchs_quad_count"] = int((gnq.cpu().numpy() == nq.cpu().numpy()).sum())
    result["frames_with_a_board"] = int((h_bst == 0).sum())
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
