"""k_decode_quads (agx_decode_quads_enqueue) at the benchmark's geometry: 256 L8 frames of 1280 x 800 resident on the device,
each with its ground-truth quads (about 36 per frame).  Three event-timed runs on the same frames:

  (a) agx_decode_quads_enqueue alone (L8: k_decode_quads is the only kernel),
  (b) agx_refine_points_enqueue into device arrays + agx_decode_quads_enqueue on those arrays (point stride 20, point statuses),
  (c) agx_detect_batch_enqueue / _fetch with the device tail -- what a caller without known quads has to run; the chain and
      k_board_tail are the parent commit's, unchanged by this one.

  python tools/decode_quads_profile.py            the driver: the timed step under its own `timeout`; writes profiles/decode_quads.txt
  python tools/decode_quads_profile.py events     the timed step: hipEvent times, 3 warm-ups, then REPS (default 20) repetitions of
                                                  each run, interleaved; median, minimum and maximum per run
  python tools/decode_quads_profile.py resources  no device needed: only the code object's figures into the file, the times marked
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
LLVM = "/opt/rocm/lib/llvm/bin"


def gpu_step():
    import numpy as np
    import torch
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import synth
    dev = torch.device("cuda", 0)
    frames, gts = synth.render_batch(0, F, W, H, device=dev)
    q = max(len(g) for g in gts)
    quads = np.zeros((F, q, 4, 2), np.float32)
    counts = np.zeros(F, np.int32)
    for f, g in enumerate(gts):
        keep = [t for t in sorted(g) if (g[t][:, 0] > 6).all() and (g[t][:, 0] < W - 6).all() and (g[t][:, 1] > 6).all() and (g[t][:, 1] < H - 6).all()]
        counts[f] = len(keep)
        quads[f, :len(keep)] = np.array([g[t] for t in keep], np.float32).reshape(-1, 4, 2)
    d_quads, d_counts = torch.from_numpy(quads).to(dev), torch.from_numpy(counts).to(dev)
    d_points = d_quads.reshape(F, q * 4, 2).contiguous()
    d_pcounts = d_counts * 4
    tags = torch.zeros((F, q, 9), dtype=torch.int32, device=dev)
    status = torch.zeros((F, q), dtype=torch.int32, device=dev)
    rec = torch.zeros((F, 4 * q, 5), dtype=torch.float32, device=dev)
    pst = torch.zeros((F, 4 * q), dtype=torch.int32, device=dev)
    det = A.TagDetector("t36h11", None, device=0)
    det.set_option("device_tail", 1)

    def a():
        det.decode_quads_enqueue(frames, d_quads, counts=d_counts, out=tags, status=status)

    def b():
        det.refine_points_enqueue(frames, d_points, counts=d_pcounts, out=rec, status=pst)
        det.decode_quads_enqueue(frames, refined=(rec, pst), counts=d_counts, out=tags, status=status)

    def c():
        det.detect_batch_enqueue(frames, cap=64)
        return det.detect_batch_fetch()

    runs = (("(a) k_decode_quads alone", a), ("(b) refine + decode chained on the device", b), ("(c) detect_batch_enqueue / _fetch, device tail", c))
    for _ in range(3):
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    a()
    det.decode_quads_fetch()
    n_quads, n_dec = int(counts.sum()), int((status.cpu().numpy()[np.arange(q)[None, :] < counts[:, None]] == 0).sum())
    n_tags = sum(len(t) for t in c())
    ms = {name: [] for name, _ in runs}
    for _ in range(REPS):
        for name, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    det.close()
    print("%d frames, %d quads (%.1f per frame), %d decoded by (a); (c) finds %d tags" % (F, n_quads, n_quads / F, n_dec, n_tags), flush=True)
    for name, _ in runs:
        v = ms[name]
        print("%-48s median %8.4f ms  min %8.4f  max %8.4f  over %d repetitions (%.0f frames/s at the median)"
              % (name, statistics.median(v), min(v), max(v), len(v), F / statistics.median(v) * 1e3), flush=True)


def resource_lines():
    lib = os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so")
    lines = ["k_decode_quads (agx_decode_quads_enqueue), %d L8 frames of %d x %d resident on the device, each frame's ground-truth quads "
             "(tools/decode_quads_profile.py)" % (F, W, H), ""]
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
                if "k_decode_quads" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                    lines.append("code object: k_decode_quads: %d VGPRs, %d SGPRs, scratch %d bytes, spilled registers %d + %d, LDS %d bytes, workgroup %d"
                                 % (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("vgpr_spill_count"), g("sgpr_spill_count"),
                                    g("group_segment_fixed_size"), g("max_flat_workgroup_size")))
    lines.append("")
    return lines


def write_out(lines):
    text = "\n".join(lines) + "\n"
    out = os.path.join(ROOT, "profiles", "decode_quads.txt")
    open(out, "w").write(text)
    print(text)
    print("written:", out)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "driver"
    if mode == "events":
        gpu_step()
    elif mode == "resources":
        write_out(resource_lines() + ["times of (a), (b) and (c): NOT MEASURED YET -- run `python tools/decode_quads_profile.py` on an MI355X"])
    else:
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "events"], capture_output=True, text=True)
        if r.returncode != 0:  # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit("the timed step failed (exit %d)" % r.returncode)
        write_out(resource_lines() + ["hipEvent times, 3 warm-ups, runs interleaved:"] + ["  " + l for l in r.stdout.strip().split("\n") if l.strip()])
