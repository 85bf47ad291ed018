"""One RGBA8 batch (the front-end kernel + the L8 chain) captured into a HIP graph with torch.cuda.CUDAGraph after eager batches
of the same geometry and format, replayed twice: the result slabs must equal the eager ones (in its own process: a failed
capture would leave the stream in an error state)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth, sharding

dev = torch.device("cuda", 0)
F = int(os.environ.get("FRAMES", "6"))
rgb, _ = synth.render_batch(40, F, 640, 480, device=dev, fmt="RGB8")
alpha = torch.randint(0, 256, (F, 480, 640, 1), dtype=torch.uint8, device=dev)
frames = torch.cat([rgb, alpha], dim=-1).contiguous()
det = A.TagDetector("t36h11", None, device=0)
buf = sharding.alloc_result_buffers(F, dev)


def lists(b):
    t, sd = b[1].cpu().numpy(), b[0].cpu().numpy()
    return t[:, [0, 2, 3]].copy(), [sd[t[f, 1]: t[f, 1] + t[f, 0]].tobytes() for f in range(F)]


s = torch.cuda.Stream(dev)
with torch.cuda.stream(s):
    for _ in range(4):  # workspace, front plane, both counter sets, stream binding -- all before the capture
        det.saddles_batch_enqueue_to(frames, *buf)
s.synchronize()
eager = lists(buf)
with torch.cuda.stream(s):  # the same pixels as RGB8: the native path
    det.saddles_batch_enqueue_to(rgb, *buf)
s.synchronize()
native = lists(buf)
print("eager RGBA8 equals native RGB8:", np.array_equal(eager[0], native[0]) and eager[1] == native[1], "saddles", int(eager[0][:, 0].sum()), flush=True)
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=s):
    det.saddles_batch_enqueue_to(frames, *buf)
print("captured", flush=True)
ok = eager[1] == native[1] and int(eager[0][:, 0].sum()) > 0
for rep in range(2):
    buf[0].zero_(); buf[1].zero_()
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    got = lists(buf)
    same = np.array_equal(got[0], eager[0]) and got[1] == eager[1]
    print("RGBA8 graph, replay", rep, "equals eager:", same, flush=True)
    ok = ok and same
sys.exit(0 if ok else 1)
