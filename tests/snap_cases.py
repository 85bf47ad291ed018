"""What tests/test_snap_points_cpu.py and tests/test_gpu_snap_points.py share: the numpy float32 brute force that is the yardstick
of agx_snap_points_tail, a raw call of that entry into sentinel-filled arrays, and the host composition of a tracked detect."""
import ctypes as C

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

F32 = np.float32
NONE = _ffi.AGX_SNAP_NONE
TAG = A.TagDetector.TAG_DTYPE
SENTINEL = 0xA5A5A5A5
SHIFTS = ((0.0, 0.0), (1.5, -2.0), (3.0, 3.0))


def as_records(saddles):
    """SADDLE_DTYPE rows or anything [n, 5] -> contiguous float32 [n, 5]."""
    a = np.asarray(saddles)
    if a.dtype.names:
        a = np.ascontiguousarray(a).view(F32)
    return np.ascontiguousarray(a, F32).reshape(-1, 5)


def numpy_snap(saddles, points, max_dist_sq, words=None, reverse=False):
    """The yardstick: points [R, P, 2] float32 against the listed rows of saddles, every operation a float32 numpy operation (no
    fused multiply-add).  -> (slots [R, P] uint32, dist_sq [R, P] float32, rows [K, P] uint32, row_index [K] uint32, status)."""
    s = as_records(saddles)
    pts = np.ascontiguousarray(points, F32)
    if reverse:
        pts = pts[:, ::-1]
    n_rows, ppr = pts.shape[0], pts.shape[1]
    listed = np.arange(len(s)) if words is None else np.flatnonzero(np.asarray(words) == 0)
    sx, sy = s[listed, 0], s[listed, 1]
    slots = np.full((n_rows, ppr), NONE, np.uint32)
    dist = np.full((n_rows, ppr), np.inf, F32)
    if not (np.isfinite(sx).all() and np.isfinite(sy).all()):
        return slots, dist, np.zeros((0, ppr), np.uint32), np.zeros(0, np.uint32), _ffi.AGX_SNAP_INPUT
    limit = F32(max_dist_sq)
    with np.errstate(all="ignore"):
        for r in range(n_rows):
            for p in range(ppr):
                dx, dy = sx - pts[r, p, 0], sy - pts[r, p, 1]
                d2 = dx * dx + dy * dy
                assert d2.dtype == F32
                d2 = np.where(d2 < F32(np.inf), d2, F32(np.inf))  # (+inf and NaN are no distance)
                if len(d2) and d2.min() < F32(np.inf):
                    k = int(np.argmin(d2))  # the first minimum: the lowest slot
                    dist[r, p] = d2[k]
                    if d2[k] <= limit:
                        slots[r, p] = listed[k]
    keep = [r for r in range(n_rows) if (slots[r] != NONE).all() and len(set(slots[r].tolist())) == ppr]
    return slots, dist, slots[keep].reshape(-1, ppr), np.array(keep, np.uint32), _ffi.AGX_SNAP_OK


class Raw:
    """One raw call of agx_snap_points_tail into arrays filled with SENTINEL, one row of room more than the call is told about."""

    def __init__(self, saddles, points, max_dist_sq, words=None, flags=0, n_rows=None, ppr=None, row_stride=None, point_stride=8, p_points=None,
                 with_dist=True, with_index=True, null=()):
        s = as_records(saddles)
        self.keep = (s, points, words)
        if p_points is None:
            pts = np.ascontiguousarray(points, F32)
            self.keep += (pts,)
            p_points, n_rows_d, ppr_d = pts.ctypes.data, pts.shape[0], pts.shape[1]
            n_rows = n_rows_d if n_rows is None else n_rows
            ppr = ppr_d if ppr is None else ppr
            row_stride = 8 * ppr_d if row_stride is None else row_stride
        room = (min(max(n_rows, 0), 1 << 16) + 1) * 4  # flat: the call packs [n_rows][ppr]
        self.slots, self.rows, self.dist = (np.full(room, SENTINEL, np.uint32) for _ in range(3))
        self.index = np.full(room // 4, SENTINEL, np.uint32)
        self.kept, self.status = C.c_uint32(77), C.c_uint32(77)
        w = None if words is None else np.ascontiguousarray(words, np.uint32)
        self.keep += (w,)
        arg = lambda name, value: None if name in null else value  # null: the arguments passed as NULL
        self.rc = _ffi.lib().agx_snap_points_tail(
            arg("saddles", s.ctypes.data if len(s) else None), len(s), w.ctypes.data if w is not None and len(w) else None,
            arg("points", p_points), row_stride, point_stride, n_rows, ppr, float(max_dist_sq), flags,
            arg("slots", self.slots.ctypes.data), self.dist.ctypes.data if with_dist else None, arg("rows", self.rows.ctypes.data),
            arg("kept", C.byref(self.kept)), self.index.ctypes.data if with_index else None, arg("status", C.byref(self.status)))
        self.n_rows, self.ppr, self.with_dist, self.with_index = n_rows, ppr, with_dist, with_index

    def check(self, want, what=""):
        """Equal to numpy_snap's answer bit for bit, and nothing written at or beyond the counts."""
        slots, dist, rows, index, status = want
        assert self.rc == _ffi.AGX_OK and self.status.value == status, "%s: rc %d status %d" % (what, self.rc, self.status.value)
        n, p = self.n_rows, self.ppr
        if status == _ffi.AGX_SNAP_INPUT:
            assert self.kept.value == 0
            for a in (self.slots, self.rows, self.dist, self.index):
                assert (a == SENTINEL).all(), what + ": an AGX_SNAP_INPUT list writes nothing"
            return
        assert self.kept.value == len(rows), "%s: %d rows kept, yardstick %d" % (what, self.kept.value, len(rows))
        k = len(rows)
        assert np.array_equal(self.slots[:n * p].reshape(n, p), slots), what + ": slots"
        nd, ni = (n * p if self.with_dist else 0), (k if self.with_index else 0)  # (an output that was not passed stays as it was)
        assert self.dist[:nd].tobytes() == np.ascontiguousarray(dist).view(np.uint32).reshape(-1)[:nd].tobytes(), what + ": d2 bits"
        assert np.array_equal(self.rows[:k * p].reshape(k, p), rows), what + ": compacted rows"
        assert np.array_equal(self.index[:ni], index[:ni]), what + ": row indices"
        assert (self.slots[n * p:] == SENTINEL).all() and (self.dist[nd:] == SENTINEL).all(), what + ": beyond the rows"
        assert (self.rows[k * p:] == SENTINEL).all() and (self.index[ni:] == SENTINEL).all(), what + ": beyond the kept rows"


def tag_rows(tags, shift=(0.0, 0.0)):
    """{id: 4x2 corners} -> TAG_DTYPE rows in dict order, the corners shifted in float32."""
    out = np.zeros(len(tags), TAG)
    for i, (t, xy) in enumerate(tags.items()):
        out["id"][i] = t
        out["xy"][i] = (np.asarray(xy, F32).reshape(4, 2) + np.array(shift, F32)).reshape(8)
    return out


def tracked_rounds(records, luma, prior, rounds=2, max_dist_sq=25.0, family="t36h11", spacing_ratio=0.3, tag_cap=587):
    """A tracked detect from the host forms: per round snap (corners back to front, listed slots only) -> grow_board_tail (fix
    missing) -> decode_quads_tail -> collect_tags.  records SADDLE_DTYPE [n]; prior TAG_DTYPE rows.
    -> ({id: 4x2 corners} in row order, rows snapped whole in the first round, the first round's board status)."""
    records = np.asarray(records)
    if records.dtype != A.SADDLE_DTYPE:
        records = as_records(records).view(A.SADDLE_DTYPE).reshape(-1)
    words = np.zeros(len(records), np.uint32)
    tags, n_tags, status = None, 0, _ffi.AGX_TAGS_OK
    first = None
    for _ in range(rounds):
        _slots, _dist, seeds, _index, sst = A.snap_points(records, prior, max_dist_sq, reverse=True, point_status=words)
        assert sst == _ffi.AGX_SNAP_OK
        quads, bstatus, _n, _scores, _best = A.grow_board_tail(records, seeds, spacing_ratio, 0, True, cap=1024, point_status=words)
        if first is None:
            first = (len(seeds), bstatus)
        if len(quads):
            pts = np.stack([records["x"][quads], records["y"][quads]], axis=-1)
            qtags, qstatus = A.decode_quads_tail(family, luma, pts)
        else:
            qtags, qstatus = np.zeros(0, TAG), np.zeros(0, np.uint32)
        tags, n_tags, status, words = A.collect_tags(family, quads, bstatus, qtags, qstatus, len(words), words, tags, n_tags, status, tag_cap)
    assert status == _ffi.AGX_TAGS_OK
    rows = tags[:n_tags] if tags is not None else np.zeros(0, TAG)
    return {int(t["id"]): np.array(t["xy"], F32).reshape(4, 2) for t in rows}, first[0], first[1]
