"""detect over configs[1]'s frames (1280 x 800 L8) in batches of 256 and 1024, three ways, frames/s per call (median of the
repeats, after warm-up):
  host             agx_detect_batch, frames in pageable host memory (uploaded by the call)
  host+d_frames    agx_detect_batch, frames in host memory plus their device copy (d_frames: no upload)
  device           agx_detect_batch_enqueue + agx_detect_batch_fetch, frames on the device only (host arrays)
  device_to        agx_detect_batch_enqueue_to + fetch, results in device tensors
One JSON line per batch size.  python tools/detect_device_resident.py [repeats]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth

CAP = 128


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    base, _ = synth.render_batch(0, 256, 1280, 800, device="cuda")
    det = A.TagDetector("t36h11", None, device=0)
    for n in (256, 1024):
        fr = torch.cat([base] * (n // 256)).contiguous()
        host = fr.cpu().numpy()
        out = (torch.zeros((n, CAP, 9), dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
               torch.zeros(n, dtype=torch.int32, device="cuda"))
        ref = det.detect_batch_raw(host, cap=CAP, device_frames=fr)
        assert ref[0] == 0

        def dev():
            det.detect_batch_enqueue(fr, cap=CAP)
            return det.detect_batch_fetch_raw()

        def dev_to():
            det.detect_batch_enqueue(fr, cap=CAP, out=out)
            return det.detect_batch_fetch_raw()

        got = dev()
        assert np.array_equal(got[2], ref[2]) and got[1].tobytes() == ref[1].tobytes()
        res = {"frames": n, "width": 1280, "height": 800, "cap": CAP, "host_threads": det._lib.agx_host_parallelism(),
               "repeats": reps}
        for name, fn in (("host", lambda: det.detect_batch_raw(host, cap=CAP)),
                         ("host+d_frames", lambda: det.detect_batch_raw(host, cap=CAP, device_frames=fr)),
                         ("device", dev), ("device_to", dev_to)):
            med, best = timed(fn, reps)
            res[name] = {"ms": round(med * 1e3, 3), "frames_per_s": round(n / med), "best_frames_per_s": round(n / best),
                         "tail_frames": det.get_option("last_device_tail_frames"),
                         "handed_back": det.get_option("last_device_tail_fallbacks")}
        print(json.dumps(res), flush=True)
    det.close()


if __name__ == "__main__":
    main()
