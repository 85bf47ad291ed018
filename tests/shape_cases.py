"""Inputs whose candidate components sit at the limits of the flood windows, frames whose deep response minimum is found
late, and the classifier that proves it from the oracle alone (no GPU, numpy + the oracle's own pixel_bfs).

The flood stage of chain_kernels.hip measures a component from its canonical seed (sx, sy), its first pixel in raster order:
    left reach L = sx - xmin, right reach R = xmax - sx, down reach D = ymax - sy.
First tier (flood_lane):  columns [x0, x0+32), x0 = (sx - 14) & ~3, rows [sy-1, sy+30]; a component on the window's left,
right or bottom edge goes on.  Second tier (wave_flood_128x64): columns [sx-64, sx+63], rows [sy-1, sy+62]; a component on
one of its edges sends the frame to the generic path.  tests/test_shape_cases_cpu.py asserts that FLOOD_CASES reaches every
class listed in its docstring; tests/test_gpu_flood_geometry.py runs the cases.  tools/find_flood_cases.py is the search
that produced the table.
"""
import ctypes as C

import numpy as np

COMPONENT_DTYPE = np.dtype([("sx", "i4"), ("sy", "i4"), ("L", "i4"), ("R", "i4"), ("D", "i4"), ("size", "i8"),
                            ("sum_x", "i8"), ("sum_y", "i8")])


# ---- generators ---------------------------------------------------------------------------------------------------------
def _quantise(v16, fmt):
    """v16: the real-valued plane on the 16-bit scale (32768 = mid grey).  L8 scales amplitude 25000 to 100 about 128."""
    if fmt == "L16":
        return v16.astype(np.uint16)
    if fmt == "L8":
        return (128.0 + (v16 - 32768.0) * (100.0 / 25000.0)).astype(np.uint8)
    if fmt == "LF32":
        return (v16 / 65535.0).astype(np.float32)
    raise ValueError(fmt)


def _uv(h, w, theta, ox, oy):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    return c * (xx - ox) + s * (yy - oy), -s * (xx - ox) + c * (yy - oy)


def sine_frame(h, w, px, py, theta, ox=0, oy=0, fmt="L16"):
    """32768 + 25000 sin(2 pi u / px) sin(2 pi v / py), (u, v) = (x - ox, y - oy) turned by theta: the candidates are the
    blobs around the pattern's saddles -- anisotropic (px != py) and tilted, so that a blob reaches far to the left of its
    first pixel; integer ox / oy translate the pattern (and every component) by whole pixels."""
    u, v = _uv(h, w, theta, ox, oy)
    return _quantise(32768.0 + 25000.0 * np.sin(2 * np.pi * u / px) * np.sin(2 * np.pi * v / py), fmt)


# K1's tiling of a frame (plan_k1 in chain_kernels.hip, restated: the late-minimum frames aim at its segments)
def k1_tiling(h, w, rows_per_segment=32):
    """-> (strip_cols, n_strips, rows_per_segment, n_segments, index of the full segment dispatched first)."""
    n_strips = (w + 247) // 248
    strip_cols = (((w + n_strips - 1) // n_strips) + 3) & ~3
    aligned = (strip_cols + 31) & ~31
    if aligned <= 248 and (w + aligned - 1) // aligned == n_strips:
        strip_cols = aligned
    n_strips = (w + strip_cols - 1) // strip_cols
    n_segs = (h + rows_per_segment - 1) // rows_per_segment
    n_full = h // rows_per_segment
    return strip_cols, n_strips, rows_per_segment, n_segs, (n_full - 1) >> 1


LATE_MIN_WHERE = ("top_left", "middle", "bottom_right")
LATE_MIN_RATIOS = (0.15, 0.22, 0.30)
# texture periods / tilt and the patch period: chosen so that at every ratio the texture's own saddles lie around
# 0.05 * (the patch's minimum) -- tests/test_shape_cases_cpu.py checks the three conditions on the oracle's planes
LATE_TEX_PX, LATE_TEX_PY, LATE_TEX_THETA = 13.0, 19.0, 0.4
LATE_PATCH_PERIOD, LATE_PATCH_WIDTH = 24.0, 24.0
LATE_AMPLITUDE = 24000.0  # A on the 16-bit scale; A + a <= 31200 stays inside u16 about 32768 (and inside u8 about 128)


def late_min_target(h, w, where):
    """-> (cx, cy, (x_lo, x_hi, y_lo, y_hi)): the patch centre and the strip x segment (32-row tiling) it must fall in."""
    strip_cols, n_strips, rps, n_segs, mid = k1_tiling(h, w)
    if where == "top_left":
        strip, seg = 0, 0
    elif where == "middle":
        strip, seg = n_strips // 2, mid
    elif where == "bottom_right":
        strip, seg = n_strips - 1, n_segs - 1
    else:
        raise ValueError(where)
    x_lo, x_hi = strip * strip_cols, min(w, (strip + 1) * strip_cols)
    y_lo, y_hi = seg * rps, min(h, (seg + 1) * rps)
    cx = {"top_left": 14, "middle": (x_lo + x_hi) // 2, "bottom_right": w - 14}[where]
    cy = {"top_left": 14, "middle": (y_lo + y_hi) // 2, "bottom_right": (y_lo + h - 1) // 2}[where]
    return cx, cy, (x_lo, x_hi, y_lo, y_hi)


def late_min_frame(h, w, where, ratio, fmt="L16"):
    """A tilted sine texture of amplitude a = ratio * A over the whole frame plus ONE strong saddle of amplitude A: one
    period of a product of sines under a raised-cosine window (smooth: a hard edge would make minima of its own).  The
    frame's response minimum is that saddle, `where` puts it into the first segment of the first strip, the segment K1
    dispatches first, or the short last segment of the last strip; the texture's saddles are at ratio^2 (times the
    curvature ratio of the periods) of it, i.e. around the candidate threshold 0.05 * min."""
    cx, cy, _ = late_min_target(h, w, where)
    u, v = _uv(h, w, LATE_TEX_THETA, 0, 0)
    tex = np.sin(2 * np.pi * u / LATE_TEX_PX) * np.sin(2 * np.pi * v / LATE_TEX_PY)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dx, dy = xx - cx, yy - cy
    r = np.hypot(dx, dy)
    win = np.where(r < LATE_PATCH_WIDTH / 2, 0.5 + 0.5 * np.cos(2 * np.pi * r / LATE_PATCH_WIDTH), 0.0)
    patch = np.sin(2 * np.pi * dx / LATE_PATCH_PERIOD) * np.sin(2 * np.pi * dy / LATE_PATCH_PERIOD) * win
    return _quantise(32768.0 + LATE_AMPLITUDE * (ratio * tex + patch), fmt)


def late_min_conditions(d, box):
    """The issue's three conditions on the oracle planes d of a late-minimum frame -> (argmin inside box, share of interior
    pixels below the threshold, pixels per 64 k with thr * 2 < resp < thr * 0.5)."""
    resp = d["resp"]
    h, w = resp.shape
    thr = np.float32(d["min_resp"]) * np.float32(0.05)
    ay, ax = np.unravel_index(int(np.argmin(resp)), resp.shape)
    x_lo, x_hi, y_lo, y_hi = box
    inside = bool(x_lo <= ax < x_hi and y_lo <= ay < y_hi)
    interior = resp[1:h - 1, 1:w - 1]
    share = float(np.count_nonzero(interior < thr)) / interior.size
    straddle = np.count_nonzero((interior > thr * np.float32(2.0)) & (interior < thr * np.float32(0.5)))
    return inside, share, straddle * 65536.0 / interior.size


# ---- classifier ---------------------------------------------------------------------------------------------------------
def oracle_planes(img):
    from oracle import oracle as O
    return O.refined_saddle_points(img, debug=True)[1]


def components(img, d=None):
    """4-connected components of the oracle's candidate mask resp < f32(min) * f32(0.05), in raster order of their first
    pixel: COMPONENT_DTYPE records (sx, sy, L, R, D, size, sum_x, sum_y) with exact integer sums.  The flood is the oracle's
    exported pixel_bfs on a copy of its response plane; count, first pixels and sizes are asserted against the oracle's own
    cluster table (whose seeds are interior pixels), so the classifier is itself checked on every frame it sees."""
    from oracle import oracle as O
    if d is None:
        d = oracle_planes(img)
    lib = O.lib()
    h, w = d["resp"].shape
    mat = np.ascontiguousarray(d["resp"], np.float32).copy()
    thr = np.float32(d["min_resp"]) * np.float32(0.05)
    cand = np.flatnonzero(mat.reshape(-1) < thr)
    flat = mat.reshape(-1)
    buf = np.empty((max(1, len(cand)), 2), np.uint32)
    out = []
    mp, bp = mat.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    for p in cand:
        if not flat[p] < thr:  # taken by an earlier component (pixel_bfs overwrites what it visits)
            continue
        sy, sx = divmod(int(p), w)
        n = lib.orc_pixel_bfs(mp, w, h, sx, sy, C.c_float(thr), bp, len(buf))
        assert 0 < n <= len(buf)
        xs, ys = buf[:n, 0].astype(np.int64), buf[:n, 1].astype(np.int64)
        assert ys.min() == sy and xs[ys == sy].min() == sx  # the seed is the component's first pixel in raster order
        out.append((sx, sy, sx - xs.min(), xs.max() - sx, ys.max() - sy, n, int(xs.sum()), int(ys.sum())))
    comp = np.array(out, COMPONENT_DTYPE).reshape(-1)
    assert len(comp) == len(d["sizes"]), "classifier: %d components, oracle %d clusters" % (len(comp), len(d["sizes"]))
    assert np.array_equal(comp["sy"].astype(np.int64) * w + comp["sx"], d["first_index"].astype(np.int64))
    assert np.array_equal(comp["size"], d["sizes"].astype(np.int64))
    return comp


# reach classes (conservative by one on either side of the kernel's own edge rules, so that they hold whichever way a
# comparison is written): a component surely inside the first window, surely sent on and inside the second, surely beyond
def stays_first_tier(c):
    return (c["L"] <= 13) & (c["R"] <= 13) & (c["D"] <= 28)


def inside_second_tier(c):
    return ~stays_first_tier(c) & (c["L"] <= 63) & (c["R"] <= 62) & (c["D"] <= 61)


def beyond_second_tier(c):
    return (c["L"] >= 65) | (c["R"] >= 64) | (c["D"] >= 63)


def flood_classes(comp, h, w):
    """The coverage classes (keys) that one frame's components reach.  A component on the second window's edge or beyond it
    sends the whole frame to the generic path, which hides what the flood windows made of the others: the reach values below
    the limits and the alignments count only in a frame without such a component, the limits themselves (L 64, R 63, D 62)
    only in a frame without a component beyond."""
    keys = set()
    beyond = beyond_second_tier(comp)
    if len(comp) and stays_first_tier(comp).all():
        keys.add(("all_first_tier",))
    for c in comp[beyond]:
        if c["L"] >= 65 and c["R"] < 62 and c["D"] < 61:
            keys.add(("beyond", "L"))
        if c["R"] >= 64 and c["L"] < 63 and c["D"] < 61:
            keys.add(("beyond", "R"))
        if c["D"] >= 63 and c["L"] < 63 and c["R"] < 62:
            keys.add(("beyond", "D"))
    lim = comp[at_second_tier_limit(comp)]
    for f, sel in (("L", lim["L"] >= 65), ("R", lim["R"] >= 64), ("D", lim["D"] >= 63)):
        others = {"L": lim["L"] >= 64, "R": lim["R"] >= 63, "D": lim["D"] >= 62}
        del others[f]
        if len(lim) and sel.all() and not any(o.any() for o in others.values()):
            keys.add(("beyond_only", f))  # nothing else sends this frame to the generic path
    if beyond.any():
        return keys
    for f, v in (("L", 64), ("R", 63), ("D", 62)):
        if (comp[f] == v).any():
            keys.add((f, v))
    if at_second_tier_limit(comp).any():
        return keys
    for c in comp:
        for f, first, second in (("L", (13, 14, 15, 16, 17), 63), ("R", (13, 14, 15, 16, 17), 62)):
            if c[f] in first:
                keys.add((f, int(c[f])))
                keys.add((f, int(c[f]), "sx&3", int(c["sx"]) & 3))
            if c[f] == second:
                keys.add((f, int(c[f])))
        if c["D"] in (29, 30, 61):
            keys.add(("D", int(c["D"])))
    for c in comp[inside_second_tier(comp)]:
        sh = (int(c["sy"]) - 1) & 31
        if sh in (0, 31):
            keys.add(("second", "sh", sh))
        if c["sx"] < 64:
            keys.add(("second", "left_padding"))
        if c["sx"] > w - 64:
            keys.add(("second", "right_padding"))
        if c["sy"] + 62 >= h:
            keys.add(("second", "bottom_padding"))
    return keys


def at_second_tier_limit(c):
    """On the second window's edge (the kernel sends the frame to the generic path) or beyond it."""
    return (c["L"] >= 64) | (c["R"] >= 63) | (c["D"] >= 62)


def make_case(case):
    fmt, h, w, px, py, theta, ox, oy = case
    return sine_frame(h, w, px, py, theta, ox, oy, fmt)


# (fmt, h, w, px, py, theta, ox, oy) -- printed by tools/find_flood_cases.py; what each frame covers is recomputed and
# asserted by tests/test_shape_cases_cpu.py
FLOOD_CASES = [
    ("L16", 160, 256, 30.5, 73.2, 1.1, 1, 0),     # L and R 13..17 at every sx & 3; second tier at both shifts and all borders
    ("L16", 160, 256, 21.5, 86.0, -0.5, 0, 0),    # D 29 / 30, R 14..17
    ("L16", 160, 256, 107.0, 428.0, 1.1, 2, 11),  # beyond the second tier to the left, to the right and downwards at once
    ("L16", 160, 256, 80.0, 80.0, 0.3, 2, 5),     # D 61, R 62 (inside the second tier: no generic path)
    ("L16", 160, 256, 81.5, 81.5, 0.3, 0, 11),    # D 62, R 63 (on its edge)
    ("L16", 160, 256, 51.5, 123.6, 0.3, 0, 0),    # beyond it to the right only
    ("L16", 160, 256, 56.0, 224.0, 0.3, 0, 0),    # ... downwards only (tall and thin)
    ("L16", 160, 256, 107.0, 428.0, 1.1, 0, 0),   # ... to the left only
    ("L16", 160, 256, 64.25, 257.0, 1.1, 0, 0),   # L 64 (on the edge)
    ("L16", 160, 256, 64.25, 257.0, 1.1, 1, 0),   # L 63
    ("L16", 160, 256, 41.0, 41.0, 0.78, 0, 0),    # every component in the first tier (R up to 13)
    ("L16", 160, 256, 29.0, 29.0, 0.5, 0, 0),     # every component in the first tier
    # the same geometry through the other two front ends (their quantisation moves a limit by a pixel here and there)
    ("L8", 160, 256, 30.5, 73.2, 1.1, 1, 0),
    ("L8", 160, 256, 80.0, 80.0, 0.3, 2, 5),
    ("L8", 160, 256, 51.5, 123.6, 0.3, 0, 0),
    ("L8", 160, 256, 29.0, 29.0, 0.5, 0, 0),
    ("LF32", 160, 256, 21.5, 86.0, -0.5, 0, 0),
    ("LF32", 160, 256, 64.25, 257.0, 1.1, 1, 0),
    ("LF32", 160, 256, 107.0, 428.0, 1.1, 0, 0),
    ("LF32", 160, 256, 29.0, 29.0, 0.5, 0, 0),
]

# frames whose largest cluster has a coordinate sum of 2^24 or more (AGX_FRAME_CENTROID_INEXACT): (h, w, px, py, theta)
CENTROID_CASES = [(128, 2048, 64.0, 64.0, 0.0), (96, 3000, 64.0, 64.0, 0.0)]
