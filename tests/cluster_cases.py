"""Hand-built response planes for agx_clusters_enqueue, and what the oracle makes of them.

Planes of 160 x 96 -- three word rows of 32 image rows, the wave seams at columns 64 and 128 inside --, three to a batch.  A
plane is +0.0 with one pixel at MIN (the frame minimum, so thr = 0.05 * MIN = -5) and pixels at LOW (-10, below thr) drawn on it;
what each plane is meant to reach is in CASES, and tests/test_cluster_cases_cpu.py asserts it from the oracle alone.

expected(plane) is src/detector.rs:414-429 by the oracle: orc_min_response, thr = min * 0.05f, orc_cluster_centers.  A plane with
a ring pixel below thr is one agx_clusters_enqueue refuses (AGX_CLUSTERS_BORDER, count 0)."""
import ctypes as C
import functools

import numpy as np

W, H = 160, 96
MIN, LOW = np.float32(-100.0), np.float32(-10.0)
OK, CAPACITY, BORDER, OVERFLOW, INEXACT = 0, 1, 2, 3, 0x100
CLUSTER_DTYPE = np.dtype([("first_index", "u4"), ("size", "u4"), ("cx", "f4"), ("cy", "f4")])


def _base():
    p = np.zeros((H, W), np.float32)
    p[3, 150] = MIN  # a cluster of its own in every plane built on this
    return p


def plane_small():
    """Single pixels, components across the word-row and the column seams, first pixels sharing a row, odd values."""
    p = _base()
    for x, y in ((5, 5), (70, 40), (158, 94), (1, 1), (64, 32), (127, 63)):
        p[y, x] = LOW
    p[30:34, 20] = LOW          # across rows 31 | 32
    p[63:66, 100] = LOW         # across rows 63 | 64
    p[50, 62:66] = LOW          # across columns 63 | 64
    p[70, 126:131] = LOW        # across columns 127 | 128
    p[60:63, 10] = LOW          # two components whose first pixels share row 60
    p[60, 14:17] = LOW
    p[61, 16] = LOW
    p[5, 6] = np.nan            # never below any threshold, next to a single pixel
    p[40, 71] = np.float32("inf")
    p[41, 70] = np.float32(-0.0)
    p[80, 80] = np.nan
    p[20, 120] = np.float32(-5.0)  # == thr: not below
    p[20, 122] = np.nextafter(np.float32(-5.0), np.float32(-6.0))  # just below thr
    return p


def plane_wide():
    """One component wider than the 32 x 32 window of a lane (second flood tier), inside 128 x 64."""
    p = _base()
    p[20:60, 30:70] = LOW       # 40 x 40, filled
    p[40, 70:100] = LOW         # an arm: 70 wide in all
    p[10, 10] = LOW
    p[90, 140] = LOW
    return p


def plane_beyond():
    """One component beyond the 128 x 64 window of a wave (generic path): a cross of 140 x 70."""
    p = _base()
    p[48, 10:150] = LOW
    p[10:80, 80] = LOW
    p[5, 5] = LOW
    p[90, 20:23] = LOW
    return p


def plane_zero():
    return np.zeros((H, W), np.float32)  # min = +0.0, thr = 0: nothing is below


def plane_min_positive():
    p = np.full((H, W), 1.0, np.float32)
    p[10:20, 10:20] = 0.5       # min 0.5, thr 0.025: nothing is below
    return p


def plane_border():
    """plane_small with one ring pixel at the frame minimum: refused."""
    p = plane_small()
    p[0, 77] = MIN
    return p


CASES = {"small": plane_small, "wide": plane_wide, "beyond": plane_beyond, "zero": plane_zero, "min_positive": plane_min_positive,
         "border": plane_border}
BATCHES = [("small", "zero", "wide"), ("beyond", "border", "min_positive")]  # the refused frame between two others


def _orc():
    from oracle import oracle as O
    lib = O.lib()
    lib.orc_min_response.restype = C.c_float
    lib.orc_min_response.argtypes = [C.c_void_p, C.c_size_t]
    lib.orc_cluster_centers.restype = C.c_int
    lib.orc_cluster_centers.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.orc_pixel_bfs.restype = C.c_int
    lib.orc_pixel_bfs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int]
    return lib


def threshold(plane):
    a = np.ascontiguousarray(plane, np.float32)
    m = np.float32(_orc().orc_min_response(a.ctypes.data, a.size))
    return m, np.float32(m * np.float32(0.05))


def oracle_rows(plane):
    """orc_cluster_centers on a contiguous copy -> rows CLUSTER_DTYPE in the reference's order (whatever the ring holds)."""
    a = np.ascontiguousarray(plane, np.float32).copy()
    h, w = a.shape
    _, thr = threshold(a)
    cap = max(16, a.size // 2)
    centers, first, sizes = np.zeros((cap, 2), np.float32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    n = _orc().orc_cluster_centers(a.ctypes.data, w, h, float(thr), centers.ctypes.data, first.ctypes.data, sizes.ctypes.data, cap)
    assert 0 <= n <= cap
    rows = np.zeros(n, CLUSTER_DTYPE)
    rows["first_index"], rows["size"], rows["cx"], rows["cy"] = first[:n], sizes[:n], centers[:n, 0], centers[:n, 1]
    return rows


def ring_below(plane):
    a = np.asarray(plane, np.float32)
    _, thr = threshold(a)
    if a.shape[0] < 3 or a.shape[1] < 3:
        return False
    ring = np.concatenate([a[0], a[-1], a[:, 0], a[:, -1]])
    return bool((ring < thr).any())


def expected_of(plane):
    """-> (rows, status): what agx_clusters_enqueue answers for the plane with room for every row."""
    if ring_below(plane):
        return np.zeros(0, CLUSTER_DTYPE), BORDER
    return oracle_rows(plane), OK


@functools.lru_cache(maxsize=None)
def expected(name):
    rows, status = expected_of(CASES[name]())
    rows.setflags(write=False)
    return rows, status


def members(plane, first_index):
    """The pixels (x, y) of the component the oracle's flood reaches from first_index (orc_pixel_bfs on a copy)."""
    a = np.ascontiguousarray(plane, np.float32).copy()
    h, w = a.shape
    _, thr = threshold(a)
    out = np.zeros((a.size, 2), np.uint32)
    n = _orc().orc_pixel_bfs(a.ctypes.data, w, h, int(first_index) % w, int(first_index) // w, float(thr), out.ctypes.data, a.size)
    return out[:n].astype(np.int64)


def batch(names):
    return np.stack([CASES[n]() for n in names])


# ---- coordinate sums at 2^24 and beyond 2^32 --------------------------------------------------------------------------------
# Planes of their own sizes (not BATCHES' 160 x 96): one large component -- full rows of `width` columns from (1, 1), a partial
# row below them and one more pixel below that, which tunes the sum -- whose sum of x (or, transposed, of y) is the target, and
# a small cluster (three pixels, the frame minimum among them) beside it.  Every component is far beyond a wave's 128 x 64
# window: the generic path.
def _sum_plane(target, width):
    """-> plane [rows + 4, width + 6] whose large component has sum of x == target."""
    row = width * (width + 1) // 2            # x = 1 .. width
    full, rest = divmod(target, row)
    m = int((np.sqrt(8.0 * rest + 1.0) - 1.0) / 2.0)  # the partial row: x = 1 .. m
    while m * (m + 1) // 2 > rest:
        m -= 1
    tune = rest - m * (m + 1) // 2            # the last pixel's x, below the partial row
    assert 1 <= tune <= m <= width and full >= 1, (target, width, full, m, tune)
    p = np.zeros((full + 4, width + 6), np.float32)
    p[1:1 + full, 1:1 + width] = LOW
    p[1 + full, 1:1 + m] = LOW
    p[2 + full, tune] = LOW
    p[1, width + 2] = MIN                     # the small cluster: columns width + 2 .. width + 3 (column width + 1 separates)
    p[1, width + 3] = LOW
    p[2, width + 3] = LOW
    return p


E24 = 1 << 24
WIDE_CASES = {
    "sum x 2^24 - 1": lambda: _sum_plane(E24 - 1, 1024),
    "sum x 2^24": lambda: _sum_plane(E24, 1024),
    "sum x 2^24 + 1": lambda: _sum_plane(E24 + 1, 1024),
    "sum y 2^24 - 1": lambda: np.ascontiguousarray(_sum_plane(E24 - 1, 1024).T),
    "sum y 2^24": lambda: np.ascontiguousarray(_sum_plane(E24, 1024).T),
    "sum y 2^24 + 1": lambda: np.ascontiguousarray(_sum_plane(E24 + 1, 1024).T),
    # 64 full rows of w columns from x = 1 sum to 32 w (w + 1): beyond 2^32 from w = WIDTH_32 = 11585 on (11584 * 11585 < 2^27 <
    # 11585 * 11586); the target just beyond 2^32 takes 63 full rows of that width and most of the 64th
    "sum x beyond 2^32": lambda: _sum_plane((1 << 32) + 4097, WIDTH_32),
}
WIDTH_32 = 11585
WIDE_CANDIDATES = 1 << 20  # agx_detector_set_limits: the largest plane has 741 412 pixels below thr, the default list holds half a plane


@functools.lru_cache(maxsize=None)
def wide_expected(name):
    """-> (rows, status, sums): first index and size from the oracle's components; the centre f32(exact integer sum) / f32(size)
    (DESIGN section 3), which below 2^24 is the oracle's own; AGX_CLUSTERS_INEXACT from the sums.  sums[i] = (sum x, sum y)."""
    plane = WIDE_CASES[name]()
    assert not ring_below(plane)
    rows = oracle_rows(plane).copy()
    sums = []
    for r in rows:
        m = members(plane, r["first_index"])
        assert len(m) == r["size"] and int(r["first_index"]) == int((m[:, 1] * plane.shape[1] + m[:, 0]).min())
        sx, sy = int(m[:, 0].sum()), int(m[:, 1].sum())
        sums.append((sx, sy))
        if sx >= E24 or sy >= E24:
            r["cx"] = np.float32(sx) / np.float32(r["size"])  # (an integer below 2^53 -> float32: one rounding)
            r["cy"] = np.float32(sy) / np.float32(r["size"])
    status = OK | (INEXACT if any(max(s) >= E24 for s in sums) else 0)
    rows.setflags(write=False)
    return rows, status, sums
