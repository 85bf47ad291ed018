"""Device time per batch of k_remap (agx_remap_enqueue) at 256 frames of 1280 x 800 through the map of an equidistant camera into a
target of the same size, beside a device-to-device copy of the same batch in the same run -- the floor for one byte in and one
byte out per pixel -- for AGX_L8 and AGX_L16, and k_rectify_map once; then k_rectify_map under a double-sphere camera of the same
focal length near the axis (fx = 420 (1 + xi), xi = 0.6, alpha = 0.45) and k_rectified_points under both over one point per pixel
(profiles/rectify_ds.json).  One GPU, one process.

The camera: pinhole-equidistant, fx = fy = 420 on 1280 x 800 with Kalibr-sized coefficients, rectified to the pinhole of the same
fx fy cx cy (every target pixel has a source pixel there; the share of entries without one is reported).  The frames
are noise (the remap's time does not depend on the pixels).

Per figure WARMUP runs, then REPS (at least 20) readings between two events of the tool's own on the stream, as
tools/bench_board_pose.py takes them (a 1 GiB fill queued in front of the first event, so that the reading is the device's time);
the median.  The event pair's own cost is reported next to the readings and is NOT subtracted.  Beside the times: the bytes a
batch moves (source + destination, and the map once per frame group) and the bandwidth they amount to.

  python tools/bench_rectify.py [--frames 256] [--reps 20] [--warmup 3] [--out profiles/rectify.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1280, 800
FRAMES_PER_GROUP = 16  # csrc/rectify.h: REMAP_FRAMES_PER_GROUP


def med(us):
    us = sorted(us)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    if not torch.cuda.is_available():
        sys.exit("bench_rectify needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F = args.frames
    cam = A.Camera.equidistant(420.0, 420.0, 640.0, 400.0, -0.013, 0.021, -0.013, 0.0026)
    det = A.TagDetector("t36h11", None, device=0)
    filler = torch.empty(1 << 28, dtype=torch.int32, device=dev)  # 1 GiB

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

    result = {"tool": "tools/bench_rectify.py", "device": torch.cuda.get_device_name(0), "frames": F, "width": W, "height": H,
              "frames_per_group": FRAMES_PER_GROUP, "reps": args.reps, "warmup": args.warmup}
    result["event_pair_alone"] = med(timed(lambda: None))
    m = torch.empty((H, W, 2), dtype=torch.int32, device=dev)
    result["k_rectify_map"] = med(timed(lambda: det.rectify_map_enqueue(cam, (W, H), out=m)))
    host = m.cpu().numpy()
    assert host.tobytes() == A.rectify_map(cam, (W, H)).tobytes(), "the device's map is not the host form's"
    result["map_entries_without_a_source_pixel"] = round(float((host[..., 0] == _ffi.AGX_MAP_NONE).mean()), 4)
    # the double-sphere rows: k_rectify_map and k_rectified_points (one point per pixel of the target) beside the equidistant camera's
    ds = A.Camera.double_sphere(672.0, 672.0, 640.0, 400.0, 0.6, 0.45)
    m_ds = torch.empty((H, W, 2), dtype=torch.int32, device=dev)
    result["k_rectify_map_double_sphere"] = med(timed(lambda: det.rectify_map_enqueue(ds, (W, H), out=m_ds)))
    assert m_ds.cpu().numpy().tobytes() == A.rectify_map(ds, (W, H)).tobytes(), "the device's double-sphere map is not the host form's"
    result["map_entries_without_a_source_pixel_double_sphere"] = round(float((m_ds[..., 0] == _ffi.AGX_MAP_NONE).float().mean().item()), 4)
    jj, ii = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    pts = torch.stack([ii, jj], dim=-1).contiguous()
    out = torch.empty_like(pts)
    for name, c in (("equidistant", cam), ("double_sphere", ds)):
        result["k_rectified_points_%s_%d_points" % (name, W * H)] = med(timed(lambda: det.rectified_points_enqueue(pts, c, c[:4], out=out)))
    del m_ds, pts, out
    groups = (F + FRAMES_PER_GROUP - 1) // FRAMES_PER_GROUP
    for name, dtype, px in (("l8", torch.uint8, 1), ("l16", torch.int16, 2)):
        src = torch.randint(0, 256, (F, H, W), dtype=torch.uint8, device=dev)
        src = src if px == 1 else (src.to(torch.int16) * 129)
        dst = torch.empty_like(src)
        remap = med(timed(lambda: det.remap_enqueue(src, m, out=dst)))
        copy = med(timed(lambda: dst.copy_(src)))
        det.remap_enqueue(src[:2], m, out=dst[:2])
        torch.cuda.synchronize()
        ref = A.remap(src[:2].cpu().numpy().view(np.uint8 if px == 1 else np.uint16), host)
        assert dst[:2].cpu().numpy().tobytes() == ref.tobytes(), "k_remap differs from the host form"
        frames_bytes, map_bytes = 2 * F * H * W * px, groups * H * W * 8
        result["k_remap_" + name] = remap
        result["copy_d2d_" + name] = copy
        result["k_remap_%s_over_copy" % name] = round(remap["us_median"] / copy["us_median"], 3)
        result["k_remap_%s_traffic" % name] = {
            "frames_in_and_out_bytes": frames_bytes, "map_bytes_one_read_per_frame_group": map_bytes,
            "map_bytes_per_frame_group": H * W * 8, "map_share_of_traffic": round(map_bytes / (frames_bytes + map_bytes), 4),
            "remap_GBps_frames_only": round(frames_bytes / remap["us_median"] / 1e3, 1),
            "remap_GBps_with_map": round((frames_bytes + map_bytes) / remap["us_median"] / 1e3, 1),
            "copy_GBps": round(frames_bytes / copy["us_median"] / 1e3, 1)}
        del src, dst
    det.sync()
    det.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
