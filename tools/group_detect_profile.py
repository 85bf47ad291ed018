"""The group's tag packing beside the single detector's k_publish_tags, on configs[1]'s frames (256 x 1280 x 800 L8).

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/group_detect_profile.py
      a few agx_group_detect_enqueue / _fetch batches of a group of one, then as many agx_detect_batch_enqueue_to batches of a
      plain detector over the same frames: k_pack_scan, k_pack_tags and k_publish_tags are in the run's kernel statistics.
  python tools/group_detect_profile.py
      the same without a profiler: wall-clock time per call of either form, and that the two agree on every tag."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth

F, W, H, CAP, REPS = int(os.environ.get("FRAMES", "256")), 1280, 800, 128, int(os.environ.get("REPS", "6"))
fr, _ = synth.render_batch(0, F, W, H, device="cuda:0")
torch.cuda.synchronize()

grp = A.DetectorGroup("t36h11", [0], transport="peer")
t_grp = []
for _ in range(REPS):
    t0 = time.perf_counter()
    grp.detect_enqueue([fr], cap=CAP)
    rc, out, counts, status = grp.detect_fetch_raw()
    t_grp.append(time.perf_counter() - t0)
assert rc == 0

det = A.TagDetector("t36h11", None, device=0)
dev_out = (torch.zeros((F, CAP, 9), dtype=torch.int32, device="cuda"), torch.zeros(F, dtype=torch.int32, device="cuda"),
           torch.zeros(F, dtype=torch.int32, device="cuda"))
t_det = []
for _ in range(REPS):
    t0 = time.perf_counter()
    det.detect_batch_enqueue(fr, cap=CAP, out=dev_out)
    rc2, tags, cnt2, st2 = det.detect_batch_fetch_raw()
    t_det.append(time.perf_counter() - t0)
rows = tags.cpu().numpy().view(A.TagDetector.TAG_DTYPE).reshape(F, CAP)
assert rc2 == 0 and np.array_equal(counts.astype(np.int32), cnt2.cpu().numpy())
assert all(out[f, : counts[f]].tobytes() == rows[f, : counts[f]].tobytes() for f in range(F))
print("%d frames, %d tags; group of one: median %.3f ms per enqueue + fetch; agx_detect_batch_enqueue_to + fetch: %.3f ms"
      % (F, int(counts.sum()), 1e3 * float(np.median(t_grp[1:])), 1e3 * float(np.median(t_det[1:]))))
print("gathered per batch: %d bytes of table + %d bytes of slab (tags: %d bytes); unpacked rows [%d][%d]: %d bytes"
      % (F * 16, F * 128 * 36, int(counts.sum()) * 36, F, CAP, F * CAP * 36))
grp.close()
det.close()
