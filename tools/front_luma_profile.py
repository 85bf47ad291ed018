"""k_front_luma at the benchmark's geometry (256 x 1280 x 800), per layout.

  python tools/front_luma_profile.py              event times: the saddle-chain step per layout beside native RGB8 / L8 / L16
                                                  (frames resident), and a device-to-device copy that reads and writes as many
                                                  bytes as the front-end kernel of each layout does
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/front_luma_profile.py kernels
                                                  the same batches, a few of each: the kernel's own time per layout is in the
                                                  run's kernel statistics (one k_front_luma instantiation per layout)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import synth, sharding, _ffi

F, W, H = int(os.environ.get("FRAMES", "256")), 1280, 800
dev = torch.device("cuda", 0)
only_kernels = len(sys.argv) > 1 and sys.argv[1] == "kernels"
grey, _ = synth.render_batch(0, F, W, H, device=dev)
g16 = (grey.to(torch.int32) * 257 - 32768).to(torch.int16)  # (any 16-bit pattern: the kernel's time does not depend on it)
rgb = torch.stack([grey, grey, grey], dim=-1).contiguous()
a8 = torch.full((F, H, W, 1), 200, dtype=torch.uint8, device=dev)
LAYOUTS = [  # name, agx_format, tensor, bytes the front-end kernel reads + writes per pixel
    ("LA8", _ffi.AGX_LA8, lambda: torch.cat([grey[..., None], a8], -1).contiguous(), 2 + 1),
    ("RGBA8", _ffi.AGX_RGBA8, lambda: torch.cat([rgb, a8], -1).contiguous(), 4 + 1),
    ("BGR8", _ffi.AGX_BGR8, lambda: rgb.flip(-1).contiguous(), 3 + 1),
    ("BGRA8", _ffi.AGX_BGRA8, lambda: torch.cat([rgb.flip(-1), a8], -1).contiguous(), 4 + 1),
    ("RGB8P", _ffi.AGX_RGB8P, lambda: rgb.permute(0, 3, 1, 2).contiguous(), 3 + 1),
    ("LA16", _ffi.AGX_LA16, lambda: torch.stack([g16, g16], -1).contiguous(), 4 + 2),
    ("RGB16", _ffi.AGX_RGB16, lambda: torch.stack([g16, g16, g16], -1).contiguous(), 6 + 2),
    ("RGBA16", _ffi.AGX_RGBA16, lambda: torch.stack([g16, g16, g16, g16], -1).contiguous(), 8 + 2),
]
det = A.TagDetector("t36h11", None, device=0)
bufs = sharding.alloc_result_buffers(F, dev)


def timed(fn, reps=20, warm=4):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def chain(t, fmt=None):
    return lambda: det.saddles_batch_enqueue_to(t, *bufs, format=fmt)


if only_kernels:
    for name, fmt, make, _ in LAYOUTS:
        t = make()
        for _ in range(12):
            chain(t, fmt)()
        torch.cuda.synchronize()
        del t
    sys.exit(0)
px = F * W * H
native = {"L8": timed(chain(grey)), "RGB8": timed(chain(rgb)), "L16": timed(chain(g16))}
print("saddle-chain step, %d x %d x %d frames resident, ms per batch: native L8 %.4f  RGB8 %.4f  L16 %.4f" % (F, W, H, native["L8"], native["RGB8"], native["L16"]))
for name, fmt, make, bpp in LAYOUTS:
    t = make()
    ms = timed(chain(t, fmt))
    del t
    half = px * bpp // 2  # a copy of n bytes reads n and writes n
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    cp = timed(lambda: dst.copy_(src))
    del src, dst
    print("%-6s chain step %.4f ms (%.3f x RGB8, %.3f x L8); front end moves %.3f GB; a device-to-device copy of the same bytes: %.4f ms = %.0f GB/s"
          % (name, ms, ms / native["RGB8"], ms / native["L8"], px * bpp / 1e9, cp, px * bpp / 1e9 / (cp * 1e-3)), flush=True)
