"""tests/board_cases.py from the oracle and numpy alone: on every list agx_find_board_tail answers what orc_try_find_best_board
answers -- status, count, every quad and the order --, and every list is what its name says: the quad counts claimed, the
permutations, the coincident saddles, the saddles whose float32 squared distance to a 3-NN query point IS radius_sq, the two
neighbouring parameter values between which the search's answer changes, the lengths and theta bins at the list limits.  No GPU."""
import numpy as np
import pytest

from tests import board_cases as B
from tests.test_find_boards_cpu import yardstick

from aprilgrid_rs_amd import _ffi

NAMES = [c.name for c in B.CASES]


def oracle_answer(l):
    q = yardstick(l)
    return None if q is None else q.astype(np.int64).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_the_oracle_and_the_case_reaches_what_it_claims(name):
    case = B.BY_NAME[name]
    l = B.build(name)
    assert np.isfinite(l).all() and np.abs(l[:, :2]).max() < 1e6 and np.abs(l[:, 3]).max() <= 180.0, "outside the domain"
    assert (l[:, 2] == 0).all() and (l[:, 4] == 0).all()
    import aprilgrid_rs_amd as A
    quads, status, n = A.find_board_tail(l, cap=1024)
    ref = yardstick(l)  # (check_against_yardstick's comparison, with the oracle run once: it takes seconds on the longest lists)
    if ref is None:
        assert (status, n, len(quads)) == (_ffi.AGX_BOARD_NONE, 0, 0), name
    else:
        assert status == _ffi.AGX_BOARD_FOUND and n == len(ref), "%s: status %d, %d quads, the oracle %d" % (name, status, n, len(ref))
        assert np.array_equal(quads.astype(np.int64), ref.astype(np.int64)), name + ": quads or their order"
    if case.quads is None:
        assert ref is None and status == _ffi.AGX_BOARD_NONE
    elif case.quads >= 0:
        assert ref is not None and len(ref) == case.quads, "%s: the oracle finds %s quads" % (name, None if ref is None else len(ref))
    if case.family in (1, 2, 3, 4) and case.quads is not None:
        assert ref is not None and len(ref) >= 1  # (a list of these families shows a board)


def test_the_table_has_every_family_and_the_pairs_name_cases():
    assert B.FAMILIES == [1, 2, 3, 4, 5, 6]
    assert all(c.expect in ("device", "limit-pair", "any") for c in B.CASES)
    assert all(c.expect == "device" for c in B.CASES if c.family in (2, 3, 4))
    assert all(c.expect == ("device" if ": 10000 steps" in c.name else "any") for c in B.CASES if c.family == 5)
    paired = set()
    for what, small, large in B.PAIRS:
        assert len(small) >= 2 and len(large) >= 2, what  # one more size on each side of the straddling two
        for n in small + large:
            assert B.BY_NAME[n].expect == ("device" if B.BY_NAME[n].family == 3 else "limit-pair"), n  # (two and three copies: family 3's)
            paired.add(n)
    assert paired >= {c.name for c in B.CASES if c.expect == "limit-pair"}  # no limit case without its pair
    # three quarters of the table must be the kernel's even if every "any" case and every large one is handed back
    device = sum(c.expect == "device" for c in B.CASES) + sum(B.BY_NAME[n].expect == "limit-pair" for _, s, _ in B.PAIRS for n in s)
    assert 4 * device >= 3 * len(B.CASES), (device, len(B.CASES))


def test_table_rows_of_the_issue():
    want = {"lattice 2x2": None, "lattice 3x3": 1, "lattice 7x7": 9, "lattice 7x7 rows permuted": 9, "lattice 7x7 rot 30": 9, "lattice 7x7 doubled": 9,
            "lattice 7x7 theta 0/90": 4, "lattice 12x12": 30, "lattice 13x13": 36, "lattice 2x14": 6, "lattice 2x30": 14, "lattice 20x20": 90,
            "lattice 32x32": 240, "lattice 7x7 jitter 0.3": 8}
    for name, q in want.items():
        assert B.BY_NAME[name].quads == q, name  # (and the test above asserts the count from the oracle)
    assert len(B.build("lattice 32x32")) == 1024 and len(B.build("lattice 32x32 and a far saddle")) == 1025


def test_exact_lattices_are_exact():
    l = B.build("lattice 7x7")
    assert np.array_equal(l[:, 0].reshape(7, 7)[0], 100 + 20 * np.arange(7)) and np.array_equal(l[:, 1].reshape(7, 7)[:, 0], 60 + 20 * np.arange(7))
    assert set(l[:, 3]) == {45.0, -45.0} and l[0, 3] == 45.0 and l[1, 3] == -45.0
    r90 = B.build("lattice 7x7 rot 90")
    assert np.abs(r90[:, 0] - (300.0 - (l[:, 1] - 60.0))).max() < 1e-4 and set(np.round(r90[:, 3])) == {135.0, 45.0}
    # a non-integer spacing: the float32 products are not the float64 ones (they round)
    s = B.build("lattice 9x9 spacing 33.333")
    x64 = 0.1 + np.arange(9) * 33.333
    assert (s[:9, 0].astype(np.float64) != x64).any() and np.abs(s[:9, 0] - x64).max() < 1e-4
    p = B.build("lattice 9x9 projective 0").reshape(9, 9, 5)
    d = np.diff(p[0, :, 0])
    assert d.max() - d.min() > 0.05  # the spacing changes along a row: not an affine map


@pytest.mark.parametrize("name", sorted(B.PERMS))
def test_permuted_lists_are_permutations_of_their_base(name):
    base_name, perm = B.PERMS[name]
    base, l = B.build(base_name), B.build(name)
    assert sorted(perm.tolist()) == list(range(len(base))) and not np.array_equal(perm, np.arange(len(base)))
    assert l.tobytes() == base[perm].tobytes()
    # the oracle's quads of the permuted list name the same saddles as SOME quads of the lattice: a set of valid cells
    q = yardstick(l)
    cols = int(round(len(base) ** 0.5))
    for quad in perm[q]:
        r, c = np.divmod(np.sort(quad), cols)
        assert r.max() - r.min() == 1 and c.max() - c.min() == 1, (name, quad)
    assert len({tuple(sorted(x)) for x in perm[q].tolist()}) == len(q)
    assert len({p.tobytes() for _, p in B.PERMS.values()}) == len(B.PERMS)
    assert sum(b == "lattice 7x7" for b, _ in B.PERMS.values()) >= 9 and sum(b == "lattice 13x13" for b, _ in B.PERMS.values()) >= 9


def multiplicities(l):
    _, counts = np.unique(l[:, :2].copy().view(np.uint64).ravel(), return_counts=True)
    return sorted(counts.tolist())


def test_coincident_saddles_are_coincident():
    for k in (2, 3, 4, 5, 6, 8):
        assert multiplicities(B.build("7x7 every saddle %d times" % k)) == [k] * 49
    m = multiplicities(B.build("7x7 centre saddle 60 times"))
    assert m == [1] * 48 + [60] and 60 > 50  # more than the 50-NN at distance 0
    l = B.build("7x7 doubled, copies one ulp off")
    assert multiplicities(l) == [1] * 98
    a, b = l[:49], l[49:]
    assert (b[:, 0] == np.nextafter(a[:, 0], np.float32(np.inf))).all() and (b[:, 1] == np.nextafter(a[:, 1], np.float32(-np.inf))).all()
    for name in ("7x7 doubled with the other theta", "7x7 doubled with the other theta, interleaved"):
        l = B.build(name)
        assert multiplicities(l) == [2] * 49
        order = np.lexsort((l[:, 3], l[:, 0], l[:, 1]))
        assert (l[order][0::2, 3] == -l[order][1::2, 3]).all() and (np.abs(l[:, 3]) == 45.0).all()


@pytest.mark.parametrize("dy", B.RADIUS_DY)
def test_the_saddle_on_the_radius_decides_the_board(dy):
    """The moved saddle's float32 squared distance to the query point IS radius_sq; it is the query's only candidate of the
    anchor's orientation; and the oracle's board has the second quad on the radius and inside it, not outside."""
    lists = {}
    for steps, what, quads in B.RADIUS_STEPS:
        l, (qx, qy, rsq) = B.on_radius(dy, steps)
        assert l.tobytes() == B.build("radius dy %g: %s" % (dy, what)).tobytes()
        lists[what] = l
        assert rsq == np.float32(512.0)
        d2 = B.dist_sq(qx, qy, l[B.RADIUS_AT])
        if steps == 0:
            assert np.array([d2]).view(np.uint32)[0] == np.array([rsq]).view(np.uint32)[0]  # bit for bit
        else:
            assert (d2 < rsq) if steps < 0 else (d2 > rsq)
        assert abs(float(d2) - 512.0) < 1e-2
        # among the query's three nearest, the moved saddle alone has the anchor's orientation (the anchor is saddle (0, 1))
        all_d2 = np.array([B.dist_sq(qx, qy, p) for p in l])
        near = np.argsort(all_d2, kind="stable")[:3]
        assert B.RADIUS_AT in near
        same = [i for i in near if abs(l[i, 3] - l[1, 3]) < 5.0 and (all_d2[i] <= rsq or i == B.RADIUS_AT)]  # (no other one within the radius)
        assert same == [B.RADIUS_AT]
        # one seed: the fullest theta bin holds saddle (1, 1) and the far saddle
        vals, cnt = np.unique(np.round(l[:, 3]), return_counts=True)
        assert cnt.max() == 2 and vals[cnt.argmax()] == 45.0 and (cnt == 2).sum() == 1
    on, inside, outside = (oracle_answer(lists[w]) for w in ("on", "one step inside", "one step outside"))
    assert on == inside and on != outside
    q_on, q_out = yardstick(lists["on"]), yardstick(lists["one step outside"])
    assert len(q_on) == 2 and len(q_out) == 1 and B.RADIUS_AT in q_on[1] and np.array_equal(q_on[0], q_out[0])
    assert lists["on"][B.RADIUS_AT, 0] != lists["one step inside"][B.RADIUS_AT, 0] != lists["one step outside"][B.RADIUS_AT, 0]


def test_with_the_other_theta_the_saddle_on_the_radius_is_no_candidate():
    l = B.build("radius dy 4: on, other theta")
    base = B.build("radius dy 4: on")
    assert np.array_equal(np.flatnonzero((l != base).any(1)), [B.RADIUS_AT]) and l[B.RADIUS_AT, 3] == 42.0
    assert len(yardstick(l)) == 1 and len(yardstick(base)) == 2


@pytest.mark.parametrize("key", sorted(B.THRESHOLDS), ids=lambda k: "%s %s" % k)
def test_the_answer_changes_between_the_two_neighbours(key):
    name, which = key
    vals = dict(B.threshold_values(name, which))
    lo, hi = vals["0 steps below"], vals["0 steps above"]
    assert np.nextafter(lo, np.float32(np.inf)) == hi
    a, b = oracle_answer(B.sweep_list(name, lo)), oracle_answer(B.sweep_list(name, hi))
    assert a != b, "%s: the oracle answers the same on both sides of %r" % (key, lo)
    _, low_end, high_end, _ = B.SWEEPS[name]
    assert low_end < lo < hi < high_end or (which == "first" and low_end <= lo)
    end = oracle_answer(B.sweep_list(name, low_end if which == "first" else high_end))
    assert end == (a if which == "first" else b)  # the end's answer reaches up to the change
    assert oracle_answer(B.sweep_list(name, low_end)) != oracle_answer(B.sweep_list(name, high_end))
    for what, v in B.threshold_values(name, which):
        assert B.build("%s, %s change: %s" % (name, which, what)).tobytes() == B.sweep_list(name, v).tobytes()
    steps = sorted(int(np.array([v]).view(np.int32)[0]) - int(np.array([lo]).view(np.int32)[0]) for v in vals.values())
    assert steps == [-10000, -100, -10, -1, 0, 1, 2, 11, 101, 10001]


def test_the_sweeps_are_the_white_block_thresholds():
    """dtheta 30 on a diagonal at 45 degrees is |angle| = 60; shear tan(60 degrees) - 1 makes a diagonal meet theta at 60."""
    for (name, which), bits in B.THRESHOLDS.items():
        v = float(np.array([bits], np.uint32).view(np.float32)[0])
        if name.startswith("dtheta"):
            assert (abs(v - 30.0) < 1e-4) or which == "last", (name, which, v)
    assert abs(float(np.array([B.THRESHOLDS[("shear+", "last")]], np.uint32).view(np.float32)[0]) - (np.tan(np.deg2rad(60.0)) - 1.0)) < 1e-5


def test_tie_lists_in_other_orders_hold_the_same_saddles():
    more = [c for c in B.CASES if c.family in (3, 4) and (", perm " in c.name or c.name.endswith(", reversed"))]
    assert len(more) == 5 * sum(1 for c in B.CASES if c.family in (3, 4)) // 6 >= 60
    for c in more:
        base = B.build(c.name.rsplit(", ", 1)[0])
        l = B.build(c.name)
        order = lambda a: a[np.lexsort(a.T[::-1])]
        assert l.tobytes() != base.tobytes() and order(l).tobytes() == order(base).tobytes(), c.name


def test_lists_at_the_limits_are_what_they_say():
    for n in (1023, 1024, 1025, 1100):
        l = B.build("7x7 and far saddles, %d in all" % n)
        assert len(l) == n and l[:49].tobytes() == B.build("lattice 7x7").tobytes() and l[49:, 0].min() > 2000
    for w, quads in ((27, 9), (28, 9), (29, 1), (30, 1)):  # the 30th seed is the last that counts
        l = B.build("30 seeds: %d spent before the lattice's" % w)
        assert not (np.abs(l[:, 3] - np.round(l[:, 3])) == 0.5).any()
        vals, cnt = np.unique(np.round(l[:, 3]), return_counts=True)
        assert vals[cnt.argmax()] == 45.0 and (cnt == cnt.max()).sum() == 1
        in_bin = np.flatnonzero(np.round(l[:, 3]) == 45.0)
        assert (in_bin >= 49).sum() == w and l[:49].tobytes() == B.build("lattice 7x7").tobytes()
        q = yardstick(l)
        assert len(q) == quads and (q.max() < 49) == (quads == 9), w
    for m in (20, 24, 26, 28, 30, 40):
        l = B.build("strip 2x%d" % m if m != 30 else "lattice 2x30")
        q = yardstick(l)
        assert len(l) == 2 * m and len(q) == (m - 2) // 2  # a row of quads: every other cell
    for n in (14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24):
        assert len(B.build("lattice %dx%d" % (n, n))) == n * n
    # more than TA3 = 512 pairs of other-orientation saddles among the 50 nearest of saddles the search seeds from: the (at
    # most 30) highest positions of the fullest bin; the 50 nearest include the seed itself
    for m in (3, 4):
        l = B.build("unbalanced 11x11, every %d. diagonal" % m)
        vals, cnt = np.unique(np.round(l[:, 3]), return_counts=True)
        assert vals[cnt.argmax()] == -45.0 and (cnt == cnt.max()).sum() == 1
        seeds = np.flatnonzero(l[:, 3] == -45.0)[::-1][:30]
        beyond = 0
        for seed in seeds:
            d2 = ((l[:, :2].astype(np.float64) - l[seed, :2]) ** 2).sum(1)
            near = np.argsort(d2, kind="stable")[:50]
            others = int((l[near, 3] > 0).sum())
            beyond += others * (others - 1) // 2 > 512
        assert beyond >= 10, (m, beyond)
        assert np.ptp(l[l[:, 3] > 0, 3]) < 5.0  # every pair of them passes the pair list's own theta test
    # copies: k^3 times the candidate quads of a seed (9 of them in the plain lattice's 50-NN at least)
    assert len(B.build("7x7 every saddle 8 times")) == 392
