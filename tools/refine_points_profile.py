"""k_refine_points (agx_refine_points_enqueue, AGX_REFINE_BLURRED) at the benchmark's geometry: 256 L8 frames of 1280 x 800,
once with 144 and once with 1024 caller-given points per frame; beside it k_refine_patch (agx_refine_points_enqueue_h) at
half_size_patch 1, 3 and 4 and, under option "refine_general_kernel", at 2 -- the same batches, in the same run.

  python tools/refine_points_profile.py            the driver: one `rocprofv3 --kernel-trace --stats` run of the step below (no
                                                   counters in that run), each GPU step under its own `timeout`; writes
                                                   profiles/refine_points.txt -- the kernel's average duration per point count,
                                                   its VGPR count from the code object, K1's time in the same run for scale
  python tools/refine_points_profile.py kernels    the profiled step: a few batches of each point count
  python tools/refine_points_profile.py events     event times of the whole enqueue (front end + K1 + k_refine_points), ms per batch
  python tools/refine_points_profile.py resources  no device needed: only the code object's figures into the file, the times marked
                                                   NOT MEASURED YET

The points are the frames' ground-truth corners jittered by up to a pixel, repeated with fresh jitter up to the count: windows
that are read are spread over the frame as a caller's guesses would be."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, W, H = int(os.environ.get("FRAMES", "256")), 1280, 800
COUNTS = (144, 1024)
BATCHES = 12  # per point count and variant in the profiled step
# (half_size_patch, option "refine_general_kernel"), in the order the step runs them for each point count
VARIANTS = ((2, 0), (2, 1), (1, 0), (3, 0), (4, 0))


def variant_name(half, general):
    return "k_refine_points" if half == 2 and not general else "k_refine_patch<%d>" % half


def gpu_step(mode):
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    dev = torch.device("cuda", 0)
    frames, gts = synth.render_batch(0, F, W, H, device=dev)
    rng = np.random.default_rng(0)
    det = A.TagDetector("t36h11", None, device=0)
    for ppf in COUNTS:
        pts = np.empty((F, ppf, 2), np.float32)
        for f in range(F):
            g = np.unique(np.concatenate([gts[f][t] for t in gts[f]]).round(6), axis=0)
            g = g[(g[:, 0] > 6) & (g[:, 0] < W - 6) & (g[:, 1] > 6) & (g[:, 1] < H - 6)]
            pts[f] = g[np.arange(ppf) % len(g)] + rng.uniform(-1, 1, (ppf, 2))
        d_pts = torch.from_numpy(pts).to(dev)
        out = torch.empty((F, ppf, 5), dtype=torch.float32, device=dev)
        status = torch.empty((F, ppf), dtype=torch.int32, device=dev)

        for half, general in VARIANTS:
            det.set_option("refine_general_kernel", general)

            def batch():
                det.refine_points_enqueue(frames, d_pts, out=out, status=status, half_size_patch=half)

            name = variant_name(half, general)
            if mode == "kernels":
                for _ in range(BATCHES):
                    batch()
                det.refine_points_fetch()
                print("%d points per frame, %s: %d batches, %.1f %% refined" % (ppf, name, BATCHES, 100.0 * float((status == 0).float().mean())), flush=True)
            else:
                for _ in range(4):
                    batch()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    batch()
                e1.record()
                torch.cuda.synchronize()
                det.refine_points_fetch()
                print("%d points per frame: enqueue (K1 + %s), %d frames resident: %.4f ms per batch" % (ppf, name, F, e0.elapsed_time(e1) / 20), flush=True)
        det.set_option("refine_general_kernel", 0)
    det.close()


def vgprs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    text = kernel_resources.notes(os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so"))
    res = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        figures = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                        for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
        if "k_refine_points" in name:
            vec = "ILb1E" in name
            res["k_refine_points, " + ("aligned 16-byte loads" if vec else "single-float loads")] = figures
        elif "k_refine_patch" in name:
            res["k_refine_patch<%s>, 16 lanes per point, 4 points per workgroup" % re.search(r"k_refine_patchILi(\d)E", name).group(1)] = figures
    return res


def write_out(lines):
    text = "\n".join(lines) + "\n"
    out = os.path.join(ROOT, "profiles", "refine_points.txt")
    open(out, "w").write(text)
    print(text)
    print("written:", out)


def resource_lines():
    lines = ["k_refine_points, AGX_REFINE_BLURRED, %d L8 frames of %d x %d resident on the device (tools/refine_points_profile.py)" % (F, W, H), ""]
    for name, (v, s, scratch, lds) in sorted(vgprs().items()):
        lines.append("code object: %s: %d VGPRs, %d SGPRs, scratch %d bytes, LDS %d bytes" % (name, v, s, scratch, lds))
    lines.append("")
    return lines


def driver():
    lines = resource_lines()
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "trace")
        r = subprocess.run(["timeout", "-k", "10", "500", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                            sys.executable, me, "kernels"], capture_output=True, text=True)
        if r.returncode != 0:  # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit("the profiled step failed (exit %d)" % r.returncode)
        lines.append("one rocprofv3 --kernel-trace --stats run, %d batches per point count and kernel:" % BATCHES)
        lines += ["  " + l for l in r.stdout.strip().split("\n") if "points per frame" in l]
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not stats or not trace:
            sys.exit("no kernel_stats.csv / kernel_trace.csv under %s" % d)
        lines.append("kernel statistics of the run (both point counts together):")
        for row in csv.DictReader(open(stats[0])):
            if "k_refine_points" in row["Name"] or "k_refine_patch" in row["Name"] or "k_blur_hessian" in row["Name"]:
                lines.append("  %-58s calls %4s  average %10.1f us  min %10.1f us  max %10.1f us" % (
                    row["Name"].split("(")[0].replace("void agx::", ""), row["Calls"], float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3,
                    float(row["MaxNs"]) / 1e3))
        # per point count and kernel, from the same run's trace: the step runs its batches of 144 first, then those of 1024,
        # each in the order of VARIANTS
        rows = sorted((r_ for r_ in csv.DictReader(open(trace[0])) if "k_refine_points" in r_["Kernel_Name"] or "k_refine_patch" in r_["Kernel_Name"]),
                      key=lambda r_: int(r_["Start_Timestamp"]))
        if len(rows) != BATCHES * len(COUNTS) * len(VARIANTS):
            sys.exit("%d refine dispatches in the trace, %d expected" % (len(rows), BATCHES * len(COUNTS) * len(VARIANTS)))
        for i, ppf in enumerate(COUNTS):
            for j, (half, general) in enumerate(VARIANTS):
                first = (i * len(VARIANTS) + j) * BATCHES
                mine = rows[first:first + BATCHES]
                want = "k_refine_points" if half == 2 and not general else "k_refine_patch<%d>" % half
                if not all(want in r_["Kernel_Name"] for r_ in mine):
                    sys.exit("dispatches %d.. of the trace are not %s" % (first, want))
                us = [(int(r_["End_Timestamp"]) - int(r_["Start_Timestamp"])) / 1e3 for r_ in mine]
                grid = mine[0].get("Grid_Size_X", mine[0].get("Grid_Size", "?"))
                lines.append("%-18s half_size_patch %d, %4d points per frame (grid x %s): average %8.1f us  min %8.1f us  max %8.1f us over %d dispatches"
                             % (variant_name(half, general) + ",", half, ppf, grid, sum(us) / len(us), min(us), max(us), len(us)))
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "events"], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit("the event-timed step failed (exit %d)" % r.returncode)
        lines += ["", "event times, no profiler attached:"] + ["  " + l for l in r.stdout.strip().split("\n") if "points per frame" in l]
    write_out(lines)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "driver"
    if mode in ("kernels", "events"):
        gpu_step(mode)
    elif mode == "resources":
        write_out(resource_lines() + ["kernel times (144 and 1024 points per frame, K1 in the same run): NOT MEASURED YET -- run "
                                      "`python tools/refine_points_profile.py` on an MI355X"])
    else:
        driver()
