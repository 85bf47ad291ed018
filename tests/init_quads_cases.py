"""What tests/test_init_quads_cpu.py and tests/test_gpu_init_quads.py share: agx_init_quads_tail's contract stated with the
yardstick tests/board_grow_oracle.py (imported, not edited) -- its init_quads for the reference's 50 neighbours, the same dozen
lines with k as a parameter for any other n_nearest, and the first lines of its try_find_best_board for the reference's seeds.

A list is [n, 5] float32: x, y, k, theta, phi (tests/board_cases.py)."""
import numpy as np

from tests import board_grow_oracle as Y

F32 = np.float32
FOUND, NONE, CAPACITY, INPUT, PENDING = 0, 1, 2, 3, 4  # include/aprilgrid_amd.h, AGX_BOARD_*


def init_quads_k(yd, s0, k):
    """board_grow_oracle.init_quads (detector.rs:543-586) with :550's 50 as k."""
    near = yd.nearest(yd.x[s0], yd.y[s0], k)
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


def reference_seeds(yd, max_seeds=30):
    """try_find_best_board's seeds (detector.rs:601-616) in the order its loop pops them: the fullest round(theta) bin (ties: the
    smallest angle, the project's rule) from the back."""
    bins = {}
    for i in range(yd.n):
        bins.setdefault(Y._round_half_away(yd.theta[i]), []).append(i)
    if not bins:
        return []
    angle = min(bins, key=lambda a: (-len(bins[a]), a))
    return list(reversed(bins[angle]))[:max_seeds]


def yardstick(saddles, seeds=None, max_seeds=None, n_nearest=50, cap=1024, point_status=None):
    """agx_init_quads_tail's contract -> (quads [n, 4] uint32 -- no row unless FOUND --, status, n_quads, quads per seed
    [max_seeds] uint32 or None, the seeds taken uint32 or None).  seeds: indices into saddles, or None: the reference's."""
    l = np.ascontiguousarray(saddles, F32).reshape(-1, 5)
    if max_seeds is None:
        max_seeds = 30 if seeds is None else max(1, len(seeds))
    listed = np.ones(len(l), bool) if point_status is None else (np.asarray(point_status) == 0)
    empty = np.zeros((0, 4), np.uint32)
    sub = l[listed]
    if not np.isfinite(sub[:, [0, 1, 3]]).all():
        return empty, INPUT, 0, None, None
    slot_of = np.flatnonzero(listed)
    pos_of = np.full(len(l), -1, np.int64)
    pos_of[slot_of] = np.arange(len(slot_of))
    per_seed = np.zeros(max_seeds, np.uint32)
    if seeds is not None:
        seeds = [int(s) for s in list(seeds)[:max_seeds]]
        if any(s < 0 or s >= len(l) or pos_of[s] < 0 for s in seeds):
            return empty, INPUT, 0, None, None
    if len(sub) == 0:
        return empty, NONE, 0, per_seed, np.zeros(0, np.uint32)
    yd = Y.Yard(sub)
    take = reference_seeds(yd, max_seeds) if seeds is None else [int(pos_of[s]) for s in seeds]
    rows = []
    for i, s0 in enumerate(take):
        q = Y.init_quads(yd, s0) if n_nearest == 50 else init_quads_k(yd, s0, n_nearest)
        per_seed[i] = len(q)
        rows += q
    taken = np.array([slot_of[s] for s in take], np.uint32)
    quads = np.array([[slot_of[j] for j in q] for q in rows], np.uint32).reshape(-1, 4)
    if not len(quads):
        return empty, NONE, 0, per_seed, taken
    if len(quads) > cap:
        return empty, CAPACITY, len(quads), per_seed, taken
    return quads, FOUND, len(quads), per_seed, taken


def same(got, want, what=""):
    """Two answers of that contract, byte for byte."""
    assert got[1] == want[1] and got[2] == want[2], "%s: status %d count %d, expected %d %d" % (what, got[1], got[2], want[1], want[2])
    assert got[0].tobytes() == want[0].tobytes(), what + ": rows"
    for i, name in ((3, "quads per seed"), (4, "seeds taken")):
        assert (got[i] is None) == (want[i] is None) and (got[i] is None or got[i].tobytes() == want[i].tobytes()), "%s: %s" % (what, name)


def staged_board(tail_init, tail_grow, l, spacing_ratio=0.3):
    """find_boards_staged's rule on host forms: the reference's seeds and candidates, a board per candidate, the per-saddle `>= 36`
    stop (detector.rs:626) from the scores and the quads per seed, a second grow over that prefix where the first maximum moved
    -> (quads, status, n_quads) as agx_find_board_tail answers."""
    cand, st, n, per_seed, _ = tail_init(l, None, 30)
    if st != FOUND:
        return np.zeros((0, 4), np.uint32), st, 0
    q, gst, gn, scores, best = tail_grow(l, cand, spacing_ratio=spacing_ratio, stop_score=0, fix_missing=True, cap=1024)
    if gst != FOUND:
        return q, gst, gn
    best_score, best_at, done = 0, -1, 0
    for per in per_seed:
        for i in range(done, done + int(per)):
            if int(scores[i]) > best_score:
                best_score, best_at = int(scores[i]), i
        done += int(per)
        if best_score >= 36:
            break
    if best_at != best:
        q, gst, gn, _, _ = tail_grow(l, cand[:done], spacing_ratio=spacing_ratio, stop_score=0, fix_missing=True, cap=1024)
    return q, gst, gn
