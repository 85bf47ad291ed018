"""k_find_boards (agx_find_boards_enqueue) at the benchmark's geometry: 256 L8 frames of 1280 x 800 resident on the device.
Event-timed runs in one process, on the same frames and the chain's own device lists of them:

  (a) agx_find_boards_enqueue alone on the lists agx_saddles_batch_enqueue_to wrote (k_find_boards is the only kernel),
  (b) agx_refine_points_enqueue of each frame's ground-truth corners + agx_find_boards_enqueue on its device arrays (stride 20,
      point statuses) + agx_decode_quads_enqueue on the quad points, chained on the device,
  (c) k_board_tail with max_num_of_boards = 1 on the same lists: agx_detect_batch_enqueue (the chain + k_board_tail, no fetch)
      minus (d) agx_saddles_batch_enqueue_to (the chain alone), medians subtracted -- the kernel has no entry point of its own.
BLOCKS (default 5) blocks of REPS (default 20) interleaved repetitions: the median of each run over the first block, and the
spread (max - min) of the blocks' medians.

  python tools/find_boards_profile.py            the driver: the timed step under its own `timeout`; writes profiles/find_boards.txt
  python tools/find_boards_profile.py events     the timed step
  python tools/find_boards_profile.py resources  no device needed: only the code object's figures into the file, the times marked
                                                 NOT MEASURED YET"""
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, W, H = int(os.environ.get("FRAMES", "256")), 1280, 800
REPS = int(os.environ.get("REPS", "20"))
BLOCKS = int(os.environ.get("BLOCKS", "5"))
LLVM = "/opt/rocm/lib/llvm/bin"


# k_board_tail in the parent commit (its own kernel function, before the two kernels shared a body), from that commit's code object
PARENT_BOARD_TAIL = "k_board_tail before: 256 VGPRs, 106 SGPRs, scratch 224 bytes, spilled registers 31 + 202, LDS 0 bytes static + 158488 dynamic, workgroup 512"


def gpu_step():
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    dev = torch.device("cuda", 0)
    frames, gts = synth.render_batch(0, F, W, H, device=dev)
    prm = A.DetectorParams.default_params()
    prm.max_num_of_boards = 1
    det = A.TagDetector("t36h11", prm, device=0)
    det.set_option("device_tail", 1)
    Q = 64
    d_saddles = torch.zeros((F * 1024, 5), dtype=torch.float32, device=dev)
    d_table = torch.zeros((F, 4), dtype=torch.int32, device=dev)
    quads = torch.zeros((F, Q, 4), dtype=torch.int32, device=dev)
    pts = torch.zeros((F, Q, 4, 2), dtype=torch.float32, device=dev)
    n_quads = torch.zeros(F, dtype=torch.int32, device=dev)
    status = torch.zeros(F, dtype=torch.int32, device=dev)
    tags = torch.zeros((F, Q, 9), dtype=torch.int32, device=dev)
    qst = torch.zeros((F, Q), dtype=torch.int32, device=dev)
    corners = [np.concatenate([g[t] for t in sorted(g)]).astype(np.float32) for g in gts]
    P = max(len(c) for c in corners)
    points = np.full((F, P, 2), -50.0, np.float32)
    for f, c in enumerate(corners):
        points[f, :len(c)] = c
    d_points = torch.from_numpy(points).to(dev)
    rec = torch.zeros((F, P, 5), dtype=torch.float32, device=dev)
    pst = torch.zeros((F, P), dtype=torch.int32, device=dev)

    def d():
        det.saddles_batch_enqueue_to(frames, d_saddles, d_table)

    def a():
        det.find_boards_enqueue(d_saddles, frame_table=d_table, quads=quads, quad_points=pts, n_quads=n_quads, status=status)

    def b():
        det.refine_points_enqueue(frames, d_points, out=rec, status=pst)
        det.find_boards_enqueue(rec, point_status=pst, quads=quads, quad_points=pts, n_quads=n_quads, status=status)
        det.decode_quads_enqueue(frames, pts, counts=n_quads, out=tags, status=qst)

    def c():
        det.detect_batch_enqueue(frames, cap=64)

    d()
    det.sync()
    a()
    det.find_boards_fetch()
    found, back = int((status.cpu().numpy() == 0).sum()), det.get_option("last_find_boards_handed_back")
    total_quads = int(n_quads.sum().item())
    b()
    det.decode_quads_fetch()
    chain_found, chain_quads = int((status.cpu().numpy() == 0).sum()), int(n_quads.sum().item())
    d()
    det.sync()
    runs = (("(a) k_find_boards alone", a), ("(b) refine + find boards + decode, chained", b), ("(c') chain + k_board_tail, 1 board", c),
            ("(d) the chain alone", d))
    for _ in range(3):
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    med = {name: [] for name, _ in runs}
    for _ in range(BLOCKS):
        ms = {name: [] for name, _ in runs}
        for _ in range(REPS):
            for name, fn in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        for name, _ in runs:
            med[name].append(statistics.median(ms[name]))
    c()
    n_tags = sum(len(t) for t in det.detect_batch_fetch())
    det.close()
    print("%d frames: (a) finds a board in %d (%d quads, %d frames handed back); (b) in %d (%d quads); detect with one board finds %d tags"
          % (F, found, total_quads, back, chain_found, chain_quads, n_tags), flush=True)
    for name, _ in runs:
        v = med[name]
        print("%-46s median of %d %8.4f ms; medians of %d blocks: min %8.4f  max %8.4f  spread %7.4f" % (name, REPS, v[0], len(v), min(v), max(v), max(v) - min(v)), flush=True)
    tail = [x - y for x, y in zip(med["(c') chain + k_board_tail, 1 board"], med["(d) the chain alone"])]
    print("%-46s median of %d %8.4f ms; medians of %d blocks: min %8.4f  max %8.4f  spread %7.4f" % ("(c) k_board_tail, 1 board = (c') - (d)", REPS, tail[0], len(tail), min(tail), max(tail), max(tail) - min(tail)), flush=True)
    fa = med["(a) k_find_boards alone"][0]
    print("k_find_boards %.4f ms against k_board_tail %.4f ms (spread of its medians %.4f ms): %s" % (
        fa, tail[0], max(tail) - min(tail), "within it or faster" if fa <= tail[0] + (max(tail) - min(tail)) else "SLOWER than the round it is a subset of"), flush=True)


def resource_lines():
    lib = os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so")
    lines = ["k_find_boards (agx_find_boards_enqueue), %d L8 frames of %d x %d resident on the device, the chain's own saddle lists "
             "(tools/find_boards_profile.py)" % (F, W, H), "", "code object, " + PARENT_BOARD_TAIL]
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused")],
                       check=True, capture_output=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]  # one bundle per .hip file
        for i, at in enumerate(starts):
            one, co = os.path.join(tmp, "fat%d.bin" % i), os.path.join(tmp, "dev%d.co" % i)
            open(one, "wb").write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + one,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for kernel in ("k_board_tail", "k_find_boards"):
                    if kernel not in name:
                        continue
                    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                    lines.append("code object, %s now: %d VGPRs, %d SGPRs, scratch %d bytes, spilled registers %d + %d, LDS %d bytes static + 158488 dynamic, workgroup %d"
                                 % (kernel, g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("vgpr_spill_count"), g("sgpr_spill_count"),
                                    g("group_segment_fixed_size"), g("max_flat_workgroup_size")))
    lines.append("")
    return lines


def write_out(lines):
    text = "\n".join(lines) + "\n"
    out = os.path.join(ROOT, "profiles", "find_boards.txt")
    open(out, "w").write(text)
    print(text)
    print("written:", out)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "driver"
    if mode == "events":
        gpu_step()
    elif mode == "resources":
        write_out(resource_lines() + ["times of (a), (b) and (c): NOT MEASURED YET -- run `python tools/find_boards_profile.py` on an MI355X"])
    else:
        r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "events"], capture_output=True, text=True)
        if r.returncode != 0:  # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit("the timed step failed (exit %d)" % r.returncode)
        write_out(resource_lines() + ["hipEvent times, 3 warm-ups, runs interleaved, max_num_of_boards = 1:"] + ["  " + l for l in r.stdout.strip().split("\n") if l.strip()])
