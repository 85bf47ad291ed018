"""Device time per launch of k_board_fit (agx_board_fit_enqueue) at 256 frames x 36 tags with 6 x 6 layouts, beside
k_collect_tags and k_snap_points on the same tables in the same run.  One GPU, one process.

The tables: 256 L8 frames of 1280 x 800 from synth.render_batch (one 6 x 6 board each), resident on the device; their tag tables
from detect_batch_enqueue(out=...), 36 rows a frame.  The saddle lists k_snap_points reads and the board quads k_collect_tags
reads come from the staged chain (planes, clusters, refine, the k / phi filter, find boards, decode) in this process.  k_board_fit
is taken three ways: every tag of the layout predicted; only the missing ones (AGX_FIT_PREDICT_MISSING); and with one row per
frame stored under a wrong id and max_drop 1, which costs a second round.  k_snap_points snaps the 36 predicted rows per frame.

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_tracked.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time);
the median.  The event pair's own cost is reported next to the readings and is NOT subtracted.

  python tools/bench_board_fit.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/board_fit.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
Q, CPF, T = 128, 4096, 36
COLS = ROWS = 6


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "board_fit.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    if not torch.cuda.is_available():
        sys.exit("bench_board_fit needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    frames, _ = synth.render_batch(0, F, W, H, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    table, ntags, tst = torch.zeros((F, T, 9), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
    det.detect_batch_enqueue(frames, T, out=(table, ntags, tst))
    det.detect_batch_fetch(raise_on_overflow=False)
    wrong = table.clone()  # row 0 of every frame under the id of row 1: one outlier a frame
    wrong[:, 0, 0] = table[:, 1, 0]
    # the lists, the boards' quads and their decode
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
    qtags, qst = torch.zeros((F, Q, 9), **i32), torch.zeros((F, Q), **i32)
    det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
    det.find_boards_fetch()
    det.decode_quads_enqueue(frames, qpts, counts=nq, out=qtags, status=qst)
    det.sync()
    del blur, resp
    ctags, cn, cst = torch.zeros((F, T, 9), **i32), torch.zeros(F, **i32), torch.zeros(F, **i32)
    fit = dict(h=torch.zeros((F, 9), dtype=torch.float64, device=dev), err_sq=torch.zeros((F, T), **f32), row_status=torch.zeros((F, T), **i32),
               n_inliers=torch.zeros(F, **i32), rms=torch.zeros(F, **f32), pred=torch.zeros((F, COLS * ROWS, 9), **i32),
               n_pred=torch.zeros(F, **i32), status=torch.zeros(F, **i32))
    slots, seeds = torch.zeros((F, COLS * ROWS, 4), **i32), torch.zeros((F, COLS * ROWS, 4), **i32)
    nseeds, sst = torch.zeros(F, **i32), torch.zeros(F, **i32)
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

    def board_fit(tags, missing, max_drop):
        det.board_fit_enqueue(tags, ntags, COLS, ROWS, (W, H), predict_missing=missing, max_drop=max_drop, **fit)

    def outcome():
        torch.cuda.synchronize()
        st = fit["status"].cpu().numpy()
        return {"frames_ok": int((st == 0).sum()), "frames_loose": int((st == 1).sum()), "frames_refused": int((st > 1).sum()),
                "inlier_rows": int(fit["n_inliers"].sum().item()), "predicted_rows": int(fit["n_pred"].sum().item()),
                "rms_px_median": round(float(fit["rms"][fit["status"] < 2].median().item()), 4) if (st < 2).any() else None}

    result = {"tool": "tools/bench_board_fit.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "tags_per_frame": T, "layout": [ROWS, COLS], "reps": args.reps, "warmup": args.warmup, "table_rows": int(ntags.sum().item())}
    result["event_pair_alone"] = med(timed(lambda: None))
    result["k_board_fit_predict_missing"] = med(timed(lambda: board_fit(table, True, 0)))
    result["k_board_fit_predict_missing_outcome"] = outcome()
    result["k_board_fit_one_wrong_id_two_rounds"] = med(timed(lambda: board_fit(wrong, False, 1)))
    result["k_board_fit_one_wrong_id_two_rounds_outcome"] = outcome()
    result["k_board_fit_predict_all"] = med(timed(lambda: board_fit(table, False, 0)))
    result["k_board_fit_predict_all_outcome"] = outcome()
    result["k_snap_points_predicted_rows"] = med(timed(lambda: det.snap_points_enqueue(
        records, fit["pred"], slots, seeds, nseeds, sst, 9.0, counts=counts, point_status=pstatus, row_counts=fit["n_pred"], reverse=True)))
    torch.cuda.synchronize()
    result["rows_snapped_whole"] = int(nseeds.sum().item())
    result["k_collect_tags"] = med(timed(lambda: det.collect_tags_enqueue(quads, nq, bst, qtags, qst, None, ctags, cn, cst, reset=True,
                                                                          saddles_per_frame=CPF)))
    torch.cuda.synchronize()
    result["collected_tags"] = int(cn.sum().item())
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
