"""Frames of tests/test_gpu_list_limits.py and the counts the per-frame list limits (agx_detector_set_limits) are set against.
The counts come from the oracle alone (tests/test_limit_cases_cpu.py holds the premises without a GPU):
  n_saddles     the length of O.refined_saddle_points(img)                         -> what max_saddles must cover
  n_clusters    the rows of its centroid table
  n_candidates  the pixels of its response plane below f32(min) * f32(0.05)         -> what max_candidates must cover where the
                                                                                      generic path clusters the frame
  n_refined     the unfiltered refine output (more than 1024: the large-list emission, AGX_FRAME_LARGE_RESULT)
What max_clusters must cover is the flood seed list, whose length is the kernel's own rule (seed_bits: a candidate pixel with no
candidate above it ... at least one per cluster): the GPU test reads it from an unlimited run."""
import functools

import numpy as np

from tests.util import synth_module

W, H = 320, 240
NAMES = ["board0", "board1", "board2", "noise", "big", "flat"]
BOARD_SEED, NOISE_SEED = 11, 3
I_NOISE, I_BIG, I_FLAT = 3, 4, 5
# the smallest pure-noise frame (seed 7, 320 rows, widths in steps of 16) whose unfiltered refine output passes 1024 records
LARGE_W, LARGE_H, LARGE_SEED = 432, 320, 7
LARGE_BELOW_W = 416


def big_frame():
    """One sine product (that of tests/test_gpu_sparse_paths.py::test_three_paths_agree_bit_for_bit at a period of 180) whose
    lobes are diamonds 71 pixels wide and high: more than either side of the 128 x 64 second-tier flood window, so the frame
    takes the generic path by itself."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (128 + 100 * np.sin(2 * np.pi / 180.0 * xx) * np.sin(2 * np.pi / 180.0 * yy)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def batch():
    """[6, H, W] uint8: three boards, pure noise, the generic-path frame, a flat frame (NAMES)."""
    synth = synth_module()
    boards = synth.render_batch(BOARD_SEED, 3, W, H, device="cpu")[0].numpy()
    noise = synth.render_batch(NOISE_SEED, 2, W, H, device="cpu", pure_noise=True)[0].numpy()[1]
    out = np.stack([boards[0], boards[1], boards[2], noise, big_frame(), np.full((H, W), 77, np.uint8)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def noise_frame(width, height=LARGE_H, seed=LARGE_SEED):
    a = synth_module().render_batch(seed, 1, width, height, device="cpu", pure_noise=True)[0].numpy()[0].copy()
    a.setflags(write=False)
    return a


def large_frame():
    return noise_frame(LARGE_W)


def component_extent(mask, first_index):
    """(width, height) of the 4-connected component of `mask` that holds pixel first_index: a lower bound of the extent of the
    reference's component, whatever its connectivity."""
    h, w = mask.shape
    seen = np.zeros_like(mask)
    y0, x0 = divmod(int(first_index), w)
    stack, xs, ys = [(y0, x0)], [x0], [y0]
    seen[y0, x0] = True
    while stack:
        y, x = stack.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not seen[yy, xx]:
                seen[yy, xx] = True
                stack.append((yy, xx))
                xs.append(xx)
                ys.append(yy)
    return max(xs) - min(xs) + 1, max(ys) - min(ys) + 1


def counts_of(ref, d):
    """largest / largest_extent: the pixels of the largest cluster and the (width, height) its component spans at least."""
    thr = np.float32(d["min_resp"]) * np.float32(0.05)
    mask = d["resp"] < thr
    out = dict(n_saddles=len(ref), n_clusters=len(d["centers"]), n_candidates=int(mask.sum()), n_refined=len(d["refined"]), largest=0,
               largest_extent=(0, 0))
    if len(d["sizes"]):
        i = int(d["sizes"].argmax())
        out.update(largest=int(d["sizes"][i]), largest_extent=component_extent(mask, d["first_index"][i]))
    return out


_cache = {}


def oracle_counts(img):
    """-> the dict of counts_of for one frame (computed once per frame: the arrays above are cached and read-only)."""
    from oracle import oracle as O
    key = (img.shape, img.tobytes())
    if key not in _cache:
        _cache[key] = counts_of(*O.refined_saddle_points(np.ascontiguousarray(img), debug=True))
    return _cache[key]


def unique_argmax(values, what):
    """The index of the largest value, which the legs need to be one frame's alone."""
    v = np.asarray(values, np.int64)
    f = int(v.argmax())
    assert int((v == v[f]).sum()) == 1, "premise: the largest %s of the batch is not unique: %s" % (what, list(v))
    return f
