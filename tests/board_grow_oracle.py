"""The yardstick for boards grown from seed quads (agx_grow_board_tail, k_grow_boards): a numpy restatement, in binary32 step by
step, of the crate's src/board.rs:26-233 (Board::new, try_expand, try_expand_one, find_closest_potential_saddle_idxs),
try_fix_missing (:52-112) and all_tag_indexes (:49-51, cells in insertion order: the project's convention for the reference's
HashMap order), and of init_quads and try_find_best_board (src/detector.rs:543-639) -- those two only so that the restatement can
be pinned against the oracle's orc_try_find_best_board, whose board_new is not exported.

Written from the crate's text; nothing of aprilgrid_rs_amd is imported.  Every geometric decision is the oracle's exported
orc_is_valid_quad / orc_theta_distance_degree.  Nearest neighbours are brute force over the list, ordered by (binary32 squared
distance, index): where distances tie exactly the crate's k-d tree has an order of its own (tests/board_cases.py, families 3, 4).

A list is [n, 5] float32: x, y, k, theta, phi (tests/board_cases.py)."""
import ctypes as C
import sys

import numpy as np

F32 = np.float32


def _oracle():
    from oracle import oracle as O
    lib = O.lib()
    lib.orc_is_valid_quad.restype = C.c_int
    lib.orc_is_valid_quad.argtypes = [C.c_void_p] * 4
    return lib


class Yard:
    """One saddle list with what does not depend on a board: the 3-NN candidates of a pair at a ratio, is_valid_quad of four."""

    def __init__(self, saddles):
        l = np.ascontiguousarray(saddles, F32).reshape(-1, 5)
        self.l = l
        self._base = l.ctypes.data
        self.n = len(l)
        self.x, self.y, self.theta = l[:, 0].copy(), l[:, 1].copy(), l[:, 3].copy()
        self.idx = np.arange(self.n)
        self.lib = _oracle()
        self._valid = {}
        self._pair = {}

    def nearest(self, qx, qy, k):
        """tree.nearest(&[qx, qy], k, &squared_euclidean): [(dist_sq, idx)] ascending, by (dist_sq, idx)."""
        dx, dy = F32(qx) - self.x, F32(qy) - self.y  # (float32 arrays: every operation rounds to binary32)
        d2 = dx * dx + dy * dy
        order = np.lexsort((self.idx, d2))[:k]
        return [(d2[i], int(i)) for i in order]

    def theta_dist(self, t0, t1):
        return self.lib.orc_theta_distance_degree(float(t0), float(t1))

    def valid(self, i0, i1, i2, i3):
        key = (i0, i1, i2, i3)
        v = self._valid.get(key)
        if v is None:
            v = self._valid[key] = bool(self.lib.orc_is_valid_quad(*[self._base + 20 * i for i in key]))  # (20-byte records)
        return v

    def pair_candidates(self, i0, i1, spacing_ratio):
        """find_closest_potential_saddle_idxs (board.rs:177-233) before the board's own active_idxs test: the up to three
        nearest of each query point, within the radius and of the anchor's orientation, in the tree's order."""
        key = (i0, i1, F32(spacing_ratio).tobytes())
        got = self._pair.get(key)
        if got is not None:
            return got
        ratio0 = F32(F32(1.0) + F32(spacing_ratio))
        x0, y0, x1, y1 = self.x[i0], self.y[i0], self.x[i1], self.y[i1]
        ex, ey = F32(x0 - x1), F32(y0 - y1)
        radius_sq = F32(F32(0.5) * F32(F32(ex * ex) + F32(ey * ey)))
        v10x, v10y = F32(x1 - x0), F32(y1 - y0)
        out = []
        for ax, ay, at in ((x0, y0, self.theta[i0]), (x1, y1, self.theta[i1])):
            qx, qy = F32(ax + F32(v10x * ratio0)), F32(ay + F32(v10y * ratio0))
            out.append([i for d2, i in self.nearest(qx, qy, 3) if d2 <= radius_sq and self.theta_dist(at, self.theta[i]) < 5.0])
        self._pair[key] = out
        return out


class Board:
    """board.rs:18-235.  cells: {(x, y): quad or None} in insertion order."""

    def __init__(self, yard, quad, spacing_ratio):
        self.yd = yard
        self.ratio = spacing_ratio
        self.active = [True] * yard.n
        for i in quad[1:]:
            self.active[i] = False
        self.cells = {(0, 0): tuple(int(i) for i in quad)}
        self.score = 1
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 4 * yard.n + 1000))  # (try_expand recurses once per found cell)
        try:
            self.try_expand((0, 0))
        finally:
            sys.setrecursionlimit(limit)

    def closest(self, i0, i1):
        c0, c1 = self.yd.pair_candidates(i0, i1, self.ratio)
        return [i for i in c0 if self.active[i]], [i for i in c1 if self.active[i]]

    def try_expand_one(self, qs):  # :153-176
        n0, n1 = self.closest(qs[0], qs[1])
        n3, n2 = self.closest(qs[3], qs[2])
        for a in n0:
            for b in n1:
                for c in n2:
                    for d in n3:
                        if self.yd.valid(a, b, c, d):
                            return (a, b, c, d)
        return None

    def try_expand(self, at):  # :114-152
        quad = self.cells[at]
        if quad is None:
            return
        for i in range(4):
            qs = quad[i:] + quad[:i]  # rotate_left(i)
            nxt = ((at[0] + 1, at[1]), (at[0], at[1] - 1), (at[0] - 1, at[1]), (at[0], at[1] + 1))[i]
            if self.cells.get(nxt) is not None:
                continue
            new = self.try_expand_one(qs)
            if new is not None:
                v = new[4 - i:] + new[:4 - i] if i else new  # rotate_right(i)
                for vv in v:
                    self.active[vv] = False
                self.score += 1
                self.cells[nxt] = v
                self.try_expand(nxt)
            else:
                self.cells[nxt] = None

    def try_fix_missing(self):  # :52-112
        fixes = []
        for (x, y), q in self.cells.items():
            if q is not None:
                continue
            b0, b1, b2, b3 = (x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)
            if b0 in self.cells and b1 in self.cells:
                if self.cells[b0] is not None and self.cells[b1] is not None:
                    fixes.append((b0, b1))
            elif b2 in self.cells and b3 in self.cells and self.cells[b2] is not None and self.cells[b3] is not None:
                fixes.append((b2, b3))
        yd = self.yd
        for b0, b1 in fixes:
            q0, q1 = self.cells[b0], self.cells[b1]
            mid = []
            for i in range(4):
                x = F32(F32(yd.x[q0[i]] + yd.x[q1[i]]) / F32(2.0))
                y = F32(F32(yd.y[q0[i]] + yd.y[q1[i]]) / F32(2.0))
                mid.append(yd.nearest(x, y, 1)[0][1])
            if yd.valid(*mid):
                self.cells[((b0[0] + b1[0]) // 2, (b0[1] + b1[1]) // 2)] = tuple(mid)  # (between two cells two apart: exact)
        return len(fixes)

    def all_tag_indexes(self):  # :49-51, insertion order
        return [q for q in self.cells.values() if q is not None]


def init_quads(yd, s0):  # detector.rs:543-586
    near = yd.nearest(yd.x[s0], yd.y[s0], 50)
    same, diff = [], []
    for _, i in near[1:]:
        td = yd.theta_dist(yd.theta[s0], yd.theta[i])
        if td < 5.0:
            same.append(i)
        elif td > 80.0:
            diff.append(i)
    out = []
    for s1 in same:
        for a in range(len(diff)):
            for b in range(a + 1, len(diff)):
                d0, d1 = diff[a], diff[b]
                if not yd.valid(s0, d0, s1, d1):
                    continue
                v01x, v01y = F32(yd.x[d0] - yd.x[s0]), F32(yd.y[d0] - yd.y[s0])
                v02x, v02y = F32(yd.x[s1] - yd.x[s0]), F32(yd.y[s1] - yd.y[s0])
                c0 = F32(F32(v01x * v02y) - F32(v01y * v02x))
                out.append((s0, d0, s1, d1) if c0 > 0.0 else (s0, d1, s1, d0))
    return out


def _round_half_away(t):  # f32::round
    t = float(t)
    return int(np.floor(abs(t) + 0.5)) * (1 if t >= 0 else -1)


def try_find_best_board(saddles, spacing_ratio=0.3):  # detector.rs:588-639 -> [quads] or None
    yd = Yard(saddles)
    if yd.n == 0:
        return None
    bins = {}
    for i in range(yd.n):
        bins.setdefault(_round_half_away(yd.theta[i]), []).append(i)
    angle = min(bins, key=lambda a: (-len(bins[a]), a))  # the fullest bin; ties: the smallest angle (the project's rule)
    s0_idxs = list(bins[angle])
    best, best_score, count = None, 0, 0
    while s0_idxs and count < 30:
        s0 = s0_idxs.pop()
        for q in init_quads(yd, s0):
            b = Board(yd, q, spacing_ratio)
            if b.score > best_score:
                best, best_score = b, b.score
        if best_score >= 36:
            break
        count += 1
    if best is None:
        return None
    best.try_fix_missing()
    return best.all_tag_indexes()


BOARD_FOUND, BOARD_NONE, BOARD_CAPACITY, BOARD_INPUT = 0, 1, 2, 3  # include/aprilgrid_amd.h, AGX_BOARD_*


def grow(saddles, seeds, spacing_ratio=0.3, stop_score=0, fix_missing=True, point_status=None, cap=None):
    """agx_grow_board_tail's contract from the restatement above -> (quads [n, 4] uint32 -- no row unless FOUND --, status,
    n_quads, seed_scores [n_seeds] uint32 or None, best_seed or None; fixes: the length of try_fix_missing's list, None without).
    saddles [n, 5]; seeds [n_seeds, 4] indices into it; point_status: a word per saddle, 0 = listed."""
    l = np.ascontiguousarray(saddles, F32).reshape(-1, 5)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 4)
    listed = np.ones(len(l), bool) if point_status is None else (np.asarray(point_status) == 0)
    empty = np.zeros((0, 4), np.uint32)
    sub = l[listed]
    if not np.isfinite(sub[:, [0, 1, 3]]).all():
        return empty, BOARD_INPUT, 0, None, None, None
    slot_of = np.flatnonzero(listed)
    pos_of = np.full(len(l), -1, np.int64)
    pos_of[slot_of] = np.arange(len(slot_of))
    if ((seeds < 0) | (seeds >= len(l))).any() or (pos_of[seeds.clip(0, max(len(l) - 1, 0))] < 0).any() and len(seeds):
        return empty, BOARD_INPUT, 0, None, None, None
    if len(seeds) == 0:
        return empty, BOARD_NONE, 0, None, None, None
    yd = Yard(sub)
    scores = np.zeros(len(seeds), np.uint32)
    best, best_score, best_seed = None, 0, 0
    for i, s in enumerate(seeds):
        b = Board(yd, tuple(int(pos_of[j]) for j in s), F32(spacing_ratio))
        scores[i] = b.score
        if b.score > best_score:
            best, best_score, best_seed = b, b.score, i
        if stop_score and best_score >= stop_score:
            break
    fixes = best.try_fix_missing() if fix_missing else None
    quads = np.array([[slot_of[j] for j in q] for q in best.all_tag_indexes()], np.uint32).reshape(-1, 4)
    if cap is not None and len(quads) > cap:
        return empty, BOARD_CAPACITY, len(quads), scores, best_seed, fixes
    return quads, BOARD_FOUND, len(quads), scores, best_seed, fixes
