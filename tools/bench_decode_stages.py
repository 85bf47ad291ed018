"""Device time of the decode's three stages as launches of their own -- k_decode_positions, k_bit_code, k_best_tag
(agx_decode_positions_enqueue, agx_bit_code_enqueue, agx_best_tag_enqueue: src/detector.rs:42-72, :74-122, :142-169) -- next to the
fused k_decode_quads over the same batch: 256 frames x 128 quads.  One GPU, one process.

The batch is tools/bench_collect.py's: 256 L8 frames of 1280 x 800 from synth.render_batch, resident on the device; the staged
chain up to find_boards_enqueue gives every frame its board's quads, and the rows behind them up to 128 are those quads again at
half their size (they cost the decode its whole path and do not decode).  Each stage runs on the arrays the stage before it
left, so the three see what they see when chained; the three store and load the sample points and the bits in between, which
the fused kernel keeps in registers: their sum is expected to be larger, and no ratio is asked of it.

Per kernel WARMUP launches, then REPS (at least 20) readings of ONE launch between two events of the tool's own on the stream;
the median.  A fill of 1 GiB is queued in front of the first event so that the launch and the second event are in the queue
before the device reaches the first.  The event pair's own cost is reported next to the readings and is NOT subtracted.

  python tools/bench_decode_stages.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/decode_stages.json]

The JSON file is shared with tests/test_decode_stages_cpu.py (key "points_against_oracle"); this tool writes "device_times"."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_stages.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_decode_stages needs a GPU: nothing is measured without one")
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
    h_pts, h_nq, h_bst = qpts.cpu().numpy(), nq.cpu().numpy(), bst.cpu().numpy()
    for f in range(F):
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
    qtags, qst, qbits = torch.zeros((F, Q, 9), **i32), torch.zeros((F, Q), **i32), torch.zeros((F, Q), dtype=torch.int64, device=dev)
    spts, sst, sbits = torch.zeros((F, Q, 36, 2), **f32), torch.zeros((F, Q), **i32), torch.zeros((F, Q), dtype=torch.int64, device=dev)
    bst2, ids, rots, stags = torch.zeros((F, Q), **i32), torch.zeros((F, Q), **i32), torch.zeros((F, Q), **i32), torch.zeros((F, Q, 9), **i32)
    tst = torch.zeros((F, Q), **i32)
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

    # every stage reads the arrays of the one before it and writes status arrays of its own, so a repeated launch sees the same input
    fused = lambda: det.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst, bits=qbits)
    positions = lambda: det.decode_positions_enqueue(qpts, spts, sst, img_size=(W, H), counts=nq)
    bit_code = lambda: det.bit_code_enqueue(frames, spts, sbits, bst2, counts=nq, status_in=sst)
    best_tag = lambda: det.best_tag_enqueue(sbits, ids, rots, tst, counts=nq, status_in=bst2, quads=qpts, tags=stags)
    times = {"tool": "tools/bench_decode_stages.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
             "quads_per_frame": Q, "reps": args.reps, "warmup": args.warmup}
    times["event_pair_alone"] = med(timed(lambda: None))
    times["k_decode_quads"] = med(timed(fused))
    times["k_decode_positions"] = med(timed(positions))
    times["k_bit_code"] = med(timed(bit_code))
    times["k_best_tag"] = med(timed(best_tag))
    torch.cuda.synchronize()
    live = (np.arange(Q)[None, :] < h_nq[:, None])
    same = (np.array_equal(qst.cpu().numpy()[live], tst.cpu().numpy()[live]) and np.array_equal(qbits.cpu().numpy()[live], sbits.cpu().numpy()[live])
            and np.array_equal(qtags.cpu().numpy()[live], stags.cpu().numpy()[live]))
    assert same, "the three stages and k_decode_quads disagree"
    times["stages_equal_fused"] = bool(same)
    decoded = ((qst.cpu().numpy() == 0) & live).sum(axis=1)
    times["frames_with_a_board"] = int((h_nq > 0).sum())
    times["decoded_per_frame"] = {"min": int(decoded.min()), "median": float(np.median(decoded)), "max": int(decoded.max())}
    det.close()
    print(json.dumps(times))
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["device_times"] = times
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
