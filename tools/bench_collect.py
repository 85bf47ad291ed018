"""Device time of one k_collect_tags launch (agx_collect_tags_enqueue, one round of detect's loop: src/detector.rs:510-539) next
to k_decode_quads over the same batch: 256 frames x 128 quads.  One GPU, one process.

The batch: 256 L8 frames of 1280 x 800 from synth.render_batch, resident on the device; the staged chain up to
find_boards_enqueue gives every frame its board's quads (36 where the whole 6 x 6 board is found); the rows behind them up to 128
are those quads again, shrunk to half their size about their centres -- quads that cost the decode its whole path and do not
decode.  Both kernels get 128 quads per frame; the JSON says how many of them decoded.

Per kernel WARMUP launches, then REPS (at least 20) readings of ONE launch between two events of the tool's own on the stream, as
tools/bench_patch.py takes them; the median.  A launch of a few microseconds is shorter than the host needs to enqueue it, so a
fill of 1 GiB is queued in front of the first event: the launch and the second event are in the queue before the device reaches
the first, and the reading is the device's time, not the host's.  The event pair's own cost (two markers, read with nothing
between them) is reported next to the readings and is NOT subtracted.

  python tools/bench_collect.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/collect_tags.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
Q, CPF, T = 128, 4096, 128  # (T >= Q: a round cannot need more rows)


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_tags.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_collect needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    # the staged chain up to the first round's boards
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
    del blur, resp
    # 128 quads per frame: the board's, then the same ones at half their size
    h_quads, h_pts, h_nq, h_bst = quads.cpu().numpy(), qpts.cpu().numpy(), nq.cpu().numpy(), bst.cpu().numpy()
    for f in range(F):
        n = int(h_nq[f]) if h_bst[f] == 0 else 0
        if not n:
            h_nq[f], h_bst[f] = 0, 1  # (AGX_BOARD_NONE: nothing of the frame is collected)
            continue
        for j in range(n, Q):
            src = (j - n) % n
            c = h_pts[f, src].mean(axis=0, keepdims=True)
            h_pts[f, j] = c + np.float32(0.5) * (h_pts[f, src] - c)
            h_quads[f, j] = h_quads[f, src]
        h_nq[f] = Q
    board_quads = nq.cpu().numpy().copy()
    quads, qpts, nq, bst = (torch.from_numpy(a).to(dev) for a in (h_quads, h_pts, h_nq, h_bst))
    qtags, qst = torch.zeros((F, Q, 9), **i32), torch.zeros((F, Q), **i32)
    tags, ntags, tst = torch.zeros((F, T, 9), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
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

    decode = lambda: det.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst)
    collect = lambda: det.collect_tags_enqueue(quads, nq, bst, qtags, qst, pstatus, tags, ntags, tst, reset=True)
    result = {"tool": "tools/bench_collect.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "quads_per_frame": Q, "tags_per_frame": T, "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    result["k_decode_quads"] = med(timed(decode))
    result["k_collect_tags"] = med(timed(collect))
    torch.cuda.synchronize()
    decoded = (qst.cpu().numpy() == 0).sum(axis=1) * (h_nq > 0)
    h_tst, h_nt = tst.cpu().numpy(), ntags.cpu().numpy()
    assert not h_tst.any(), "a frame's tag status is not AGX_TAGS_OK"
    result["frames_with_a_board"] = int((h_nq > 0).sum())
    result["board_quads_per_frame"] = {"min": int(board_quads.min()), "median": float(np.median(board_quads)), "max": int(board_quads.max())}
    result["decoded_per_frame"] = {"min": int(decoded.min()), "median": float(np.median(decoded)), "max": int(decoded.max())}
    result["tags_per_frame_found"] = {"min": int(h_nt.min()), "median": float(np.median(h_nt)), "max": int(h_nt.max())}
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
