"""Device time of the position kernels under both sampling models and of k_tag_maps -- k_decode_positions
(AGX_TAG_MAP_AFFINE), k_positions_homography (AGX_TAG_MAP_HOMOGRAPHY), k_tag_maps at either model (src/image_util.rs:5-37, :39-70,
src/detector.rs:42-72) -- at the decode benches' 256 frames x 128 quads.  One GPU, one process.  A measurement, not a gate.

The batch is tools/bench_decode_stages.py's: 256 L8 frames of 1280 x 800 from synth.render_batch through the staged chain up to
find_boards_enqueue; the rows behind a frame's board up to 128 are its quads again at half their size.  Per kernel WARMUP
launches, then REPS (at least 20) readings of ONE launch between two events of the tool's own; the median.  A fill of 1 GiB is
queued in front of the first event.  The event pair's own cost is recorded and NOT subtracted.  k_decode_positions at affine is
read three times in the run (first, in the middle, last): the spread of the three medians is the run-to-run spread its
figure is to be compared under with the parent commit's in profiles/decode_stages.json, which is recorded beside it.

  python tools/bench_tag_maps.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/tag_maps.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tag_maps.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_tag_maps needs a GPU: nothing is measured without one")
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
    quads, qpts = torch.zeros((F, Q, 4), **i32), torch.zeros((F, Q, 4, 2), **f32)
    nq, bst = torch.zeros(F, **i32), torch.zeros(F, **i32)
    det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
    det.find_boards_fetch()
    det.sync()
    del blur, resp, frames
    h_pts, h_nq, h_bst = qpts.cpu().numpy(), nq.cpu().numpy(), bst.cpu().numpy()
    for f in range(F):  # 128 quads per frame: the board's, then the same ones at half their size
        n = int(h_nq[f]) if h_bst[f] == 0 else 0
        if not n:
            h_nq[f] = 0
            continue
        for j in range(n, Q):
            src = (j - n) % n
            c = h_pts[f, src].mean(axis=0, keepdims=True)
            h_pts[f, j] = c + np.float32(0.5) * (h_pts[f, src] - c)
        h_nq[f] = Q
    qpts, nq = torch.from_numpy(h_pts).to(dev), torch.from_numpy(h_nq).to(dev)
    spts = {m: torch.zeros((F, Q, 36, 2), **f32) for m in ("affine", "homography")}
    sst = {m: torch.zeros((F, Q), **i32) for m in ("affine", "homography")}
    maps, mst = torch.zeros((F, Q, 9), **f32), torch.zeros((F, Q), **i32)
    filler = torch.empty(1 << 28, **i32)  # 1 GiB

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            filler.zero_()
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            us.append(1000.0 * a.elapsed_time(b))
        return us

    positions = lambda m: (lambda: det.decode_positions_enqueue(qpts, spts[m], sst[m], img_size=(W, H), counts=nq, model=m))
    tag_maps = lambda m: (lambda: det.tag_maps_enqueue(qpts, maps, mst, side_bits=10, margin=0.5, model=m, counts=nq))
    times = {"tool": "tools/bench_tag_maps.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
             "quads_per_frame": Q, "reps": args.reps, "warmup": args.warmup}
    times["event_pair_alone"] = med(timed(lambda: None))
    affine = [med(timed(positions("affine")))]
    times["k_positions_homography"] = med(timed(positions("homography")))
    affine.append(med(timed(positions("affine"))))
    times["k_tag_maps_affine"] = med(timed(tag_maps("affine")))
    times["k_tag_maps_homography"] = med(timed(tag_maps("homography")))
    affine.append(med(timed(positions("affine"))))
    torch.cuda.synchronize()
    medians = [a["us_median"] for a in affine]
    times["k_decode_positions"] = affine[1]
    times["k_decode_positions_three_readings_us"] = medians
    times["k_decode_positions_spread_us"] = round(max(medians) - min(medians), 2)
    parent = os.path.join(ROOT, "profiles", "decode_stages.json")
    if os.path.exists(parent):
        times["k_decode_positions_parent_us"] = json.load(open(parent)).get("device_times", {}).get("k_decode_positions", {}).get("us_median")
    live = np.arange(Q)[None, :] < h_nq[:, None]
    sa, sh = sst["affine"].cpu().numpy(), sst["homography"].cpu().numpy()
    d = (spts["affine"].cpu().numpy() - spts["homography"].cpu().numpy())[live & (sa == 0) & (sh == 0)]
    times["slots"] = int(live.sum())
    times["decoded_affine"], times["decoded_homography"] = int((sa[live] == 0).sum()), int((sh[live] == 0).sum())
    times["largest_distance_between_the_models_px"] = round(float(np.abs(d).max()), 3) if d.size else None
    det.close()
    print(json.dumps(times))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps({"device_times": times}, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
