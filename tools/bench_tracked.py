"""Device time of a tracked round -- k_snap_points, then k_grow_boards from the snapped rows, k_decode_quads and k_collect_tags --
next to a search round -- k_find_boards, k_decode_quads, k_collect_tags -- on the same saddle lists, and of k_snap_points alone.
One GPU, one process.

The lists: 256 L8 frames of 1280 x 800 from synth.render_batch, resident on the device, through the staged chain (planes,
clusters, refine, the k / phi filter) in this process.  The priors: every frame's own tags (detect_batch_device on the same
frames) as a device tag table, every corner shifted by 2 px in x; max_dist 5 px.  The tracked round is taken twice: with the
first prior tag of a frame as its only seed row (seeds_per_frame 1) and with all of them.  No round marks a saddle used, so every
repetition sees the same lists; the fetch that would resolve a handed-back frame is outside the readings (the number of such
frames is reported).

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_grow.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time); the
median.  The event pair's own cost is reported next to the readings and is NOT subtracted.

  python tools/bench_tracked.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/tracked.json]
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
SHIFT_PX, MAX_DIST = 2.0, 5.0


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracked.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_tracked needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    # the priors: the frames' own tags, shifted
    own = det.detect_batch_device(frames)
    T = max(max(len(t) for t in own), 1)
    table = np.zeros((F, T, 9), np.uint32)
    for f, tags in enumerate(own):
        for r, (tag_id, xy) in enumerate(tags.items()):
            table[f, r, 0] = tag_id
            table[f, r, 1:] = (np.asarray(xy, np.float32).reshape(4, 2) + np.array([SHIFT_PX, 0.0], np.float32)).reshape(8).view(np.uint32)
    prior = torch.from_numpy(table.view(np.int32)).to(dev)
    prior_counts = torch.tensor([len(t) for t in own], **i32)
    one_row = torch.clamp(prior_counts, max=1)
    # the lists
    blur = torch.empty((F, H, W), **f32)
    resp = torch.empty_like(blur)
    rows, pts = torch.zeros((F, CPF, 4), **i32), torch.zeros((F, CPF, 2), **f32)
    counts, cstatus = torch.zeros(F, **i32), torch.zeros(F, **i32)
    records, pstatus = torch.zeros((F, CPF, 5), **f32), torch.zeros((F, CPF), **i32)
    det.planes_enqueue(frames, det.blur_sigma, blur=blur, response=resp)
    det.clusters_enqueue(resp, clusters=rows, points=pts, counts=counts, status=cstatus)
    det.refine_points_enqueue(blur, pts, counts=counts, out=records, status=pstatus, image="plane")
    det.filter_saddles_enqueue(records, pstatus, counts=counts)
    det.sync()
    del blur, resp
    slots, seeds = torch.zeros((F, T, 4), **i32), torch.zeros((F, T, 4), **i32)
    nseeds, sst = torch.zeros(F, **i32), torch.zeros(F, **i32)
    quads, qpts = torch.zeros((F, Q, 4), **i32), torch.zeros((F, Q, 4, 2), **f32)
    nq, bst = torch.zeros(F, **i32), torch.zeros(F, **i32)
    qtags, qst = torch.zeros((F, Q, 9), **i32), torch.zeros((F, Q), **i32)
    n_codes = det._family_info()[3]
    tags, ntags, tst = torch.zeros((F, n_codes, 9), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
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

    def snap(row_counts):
        det.snap_points_enqueue(records, prior, slots, seeds, nseeds, sst, MAX_DIST * MAX_DIST, counts=counts, point_status=pstatus,
                                row_counts=row_counts, reverse=True)

    def decode_and_collect():
        det.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst)
        det.collect_tags_enqueue(quads, nq, bst, qtags, qst, None, tags, ntags, tst, reset=True, saddles_per_frame=CPF)

    def tracked_round(row_counts):
        snap(row_counts)
        det.grow_boards_enqueue(records, seeds, quads, nq, bst, counts=counts, point_status=pstatus, seed_counts=nseeds, spacing_ratio=0.3,
                                fix_missing=True, quad_points=qpts)
        decode_and_collect()

    def search_round():
        det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
        decode_and_collect()

    def outcome():
        torch.cuda.synchronize()
        h_bst, h_ntags = bst.cpu().numpy(), ntags.cpu().numpy()
        return {"frames_found": int((h_bst == 0).sum()), "frames_handed_back": int((h_bst == 4).sum()), "tags": int(h_ntags[h_bst == 0].sum())}

    result = {"tool": "tools/bench_tracked.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "quads_per_frame": Q, "prior_rows_per_frame": T, "prior_shift_px": SHIFT_PX, "max_dist_px": MAX_DIST, "reps": args.reps,
              "warmup": args.warmup, "prior_tags": int(sum(len(t) for t in own))}
    result["event_pair_alone"] = med(timed(lambda: None))
    result["k_snap_points_all_rows"] = med(timed(lambda: snap(prior_counts)))
    torch.cuda.synchronize()
    result["rows_snapped_whole"] = int(nseeds.sum().item())
    result["k_snap_points_one_row"] = med(timed(lambda: snap(one_row)))
    result["tracked_round_one_seed"] = med(timed(lambda: tracked_round(one_row)))
    result["tracked_round_one_seed_outcome"] = outcome()
    result["tracked_round_all_rows"] = med(timed(lambda: tracked_round(prior_counts)))
    result["tracked_round_all_rows_outcome"] = outcome()
    result["search_round"] = med(timed(search_round))
    result["search_round_outcome"] = outcome()
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
