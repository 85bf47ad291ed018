"""Device time of one k_grow_boards launch (agx_grow_boards_enqueue: a board grown from ONE seed quad per frame, a quad of the
frame's own board) next to one k_find_boards launch (agx_find_boards_enqueue: the whole search, src/detector.rs:588-639) on the
same saddle lists.  One GPU, one process.

The lists: 256 L8 frames of 1280 x 800 from synth.render_batch, resident on the device, through the staged chain (planes,
clusters, refine, the k / phi filter) in this process.  The seed of frame f is the first quad of the board k_find_boards found
in it; frames without a board get no seed (AGX_BOARD_NONE in both).

Per kernel WARMUP launches, then REPS (at least 20) readings of ONE launch between two events of the tool's own on the stream, as
tools/bench_collect.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time);
the median.  The event pair's own cost is reported next to the readings and is NOT subtracted.  A launch is as long as its
slowest frame, so the per-frame distribution is reported too: each kernel on one frame at a time, for a sample of the frames.

  python tools/bench_grow.py [--frames 256] [--reps 20] [--warmup 3] [--sample 16] [--out profiles/grow_boards.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
Q, CPF = 128, 4096


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_boards.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_grow needs a GPU: nothing is measured without one")
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
    det.sync()
    find_pending = int((bst.cpu().numpy() == 4).sum())
    det.find_boards_fetch()
    det.sync()
    del blur, resp
    h_bst, h_nq = bst.cpu().numpy(), nq.cpu().numpy()
    seeds = quads[:, :1, :].contiguous()
    seed_counts = torch.from_numpy((h_bst == 0).astype(np.int32)).to(dev)
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

    def find(sl=slice(None)):
        return lambda: det.find_boards_enqueue(records[sl], counts=counts[sl], point_status=pstatus[sl], quads=quads[sl], n_quads=nq[sl], status=bst[sl])

    def grow(sl=slice(None)):
        return lambda: det.grow_boards_enqueue(records[sl], seeds[sl], gquads[sl], gnq[sl], gst[sl], counts=counts[sl], point_status=pstatus[sl],
                                               seed_counts=seed_counts[sl], spacing_ratio=0.3, stop_score=0, fix_missing=True)

    result = {"tool": "tools/bench_grow.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "quads_per_frame": Q, "seeds_per_frame": 1, "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    result["k_find_boards"] = med(timed(find()))
    result["k_grow_boards"] = med(timed(grow()))
    torch.cuda.synchronize()
    h_gst, h_gnq = gst.cpu().numpy(), gnq.cpu().numpy()
    grow_pending = int((h_gst == 4).sum())
    det.grow_boards_fetch()
    h_gst, h_gnq = gst.cpu().numpy(), gnq.cpu().numpy()
    result["find_over_grow"] = round(result["k_find_boards"]["us_median"] / result["k_grow_boards"]["us_median"], 2)
    result["frames_with_a_board"] = int((h_bst == 0).sum())
    result["frames_handed_back"] = {"k_find_boards": find_pending, "k_grow_boards": grow_pending}
    result["same_quad_count_as_the_search"] = int((h_gnq == h_nq).sum())
    result["board_quads_per_frame"] = {"min": int(h_nq.min()), "median": float(np.median(h_nq)), "max": int(h_nq.max())}
    # the slowest frame bounds a launch: each kernel on single frames
    step = max(1, F // max(1, args.sample))
    per_find, per_grow = [], []
    for f in range(0, F, step):
        sl = slice(f, f + 1)
        per_find.append(statistics.median(timed(find(sl), reps=5, warmup=1)))
        per_grow.append(statistics.median(timed(grow(sl), reps=5, warmup=1)))
    result["single_frame_launches"] = {"frames_sampled": len(per_find), "k_find_boards": med(per_find), "k_grow_boards": med(per_grow)}
    det.grow_boards_fetch()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
