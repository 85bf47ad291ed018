"""tests/cluster_cases.py from the oracle alone: every hand-built plane is what its name says (sizes and bounding boxes of the
oracle's components), no coordinate sum of the 160 x 96 planes reaches 2^24, the planes of K.WIDE_CASES have the sums they name
and the centres of the exact integer sums, and the host form of the k / phi filter (agx_filter_saddles_tail) is
src/detector.rs:432-445."""
import numpy as np

from tests import cluster_cases as K
from tests.util import bits_equal


def boxes(name):
    plane = K.CASES[name]()
    out = []
    for r in K.oracle_rows(plane):
        m = K.members(plane, r["first_index"])
        assert len(m) == r["size"]
        out.append((int(r["first_index"]), int(r["size"]), m[:, 0].min(), m[:, 0].max(), m[:, 1].min(), m[:, 1].max(), int(m[:, 0].sum()), int(m[:, 1].sum())))
    return out


def test_geometry_covers_three_word_rows_and_both_column_seams():
    assert K.H == 3 * 32 and K.W > 128 and K.W % 64 != 0
    assert sorted(n for b in K.BATCHES for n in b) == sorted(K.CASES) and all(len(b) == 3 for b in K.BATCHES)


def test_small_plane_has_single_pixels_seam_crossers_and_a_shared_row():
    b = boxes("small")
    singles = [c for c in b if c[1] == 1]
    assert len(singles) >= 7  # the six drawn ones, the minimum and the pixel just below thr
    assert any(c[4] <= 31 and c[5] >= 32 for c in b) and any(c[4] <= 63 and c[5] >= 64 for c in b)      # across word rows
    assert any(c[2] <= 63 and c[3] >= 64 for c in b) and any(c[2] <= 127 and c[3] >= 128 for c in b)    # across column seams
    rows_of_first = [c[0] // K.W for c in b]
    assert any(rows_of_first.count(r) >= 2 for r in set(rows_of_first))  # two components first met in one row
    first = [c[0] for c in b]
    assert first == sorted(first) and len(set(first)) == len(first)
    plane = K.CASES["small"]()
    m, thr = K.threshold(plane)
    assert m == K.MIN and thr == np.float32(-5.0)
    assert np.isnan(plane).sum() == 2 and np.isinf(plane).sum() == 1 and (np.signbit(plane) & (plane == 0)).sum() == 1
    at = {c[0] for c in b}
    assert 20 * K.W + 122 in at and 20 * K.W + 120 not in at  # just below thr / equal to thr
    assert all(c[3] - c[2] < 32 and c[5] - c[4] < 32 for c in b)  # everything fits a lane's window


def test_wide_plane_needs_the_second_flood_tier_only():
    b = boxes("wide")
    big = max(b, key=lambda c: c[1])
    assert big[1] == 40 * 40 + 30
    assert big[3] - big[2] + 1 > 32 and big[5] - big[4] + 1 > 32
    assert big[3] - big[2] + 1 <= 128 and big[5] - big[4] + 1 <= 64
    assert len(b) == 4


def test_beyond_plane_needs_the_generic_path():
    b = boxes("beyond")
    big = max(b, key=lambda c: c[1])
    assert big[3] - big[2] + 1 > 128 and big[5] - big[4] + 1 > 64
    assert big[1] == 140 + 70 - 1 and len(b) == 4


def test_empty_planes_have_no_cluster():
    for name, want_min in (("zero", 0.0), ("min_positive", 0.5)):
        rows, status = K.expected(name)
        assert len(rows) == 0 and status == K.OK
        m, thr = K.threshold(K.CASES[name]())
        assert m == np.float32(want_min) and not (K.CASES[name]() < thr).any()
    assert K.threshold(K.CASES["min_positive"]())[1] > 0


def test_border_plane_is_refused_and_only_for_its_ring_pixel():
    plane = K.CASES["border"]()
    assert K.ring_below(plane) and K.expected("border")[1] == K.BORDER and len(K.expected("border")[0]) == 0
    plane[0, 77] = 0.0
    assert bits_equal(plane, K.CASES["small"]()) and not K.ring_below(plane)
    for name in ("small", "wide", "beyond", "zero", "min_positive"):
        assert not K.ring_below(K.CASES[name]())


def test_no_coordinate_sum_reaches_2_to_24_and_centroids_are_the_quotients():
    for name in ("small", "wide", "beyond"):
        rows = K.expected(name)[0]
        for r, c in zip(rows, boxes(name)):
            assert c[6] < 1 << 24 and c[7] < 1 << 24
            assert r["cx"] == np.float32(c[6]) / np.float32(c[1]) and r["cy"] == np.float32(c[7]) / np.float32(c[1])


# ---- sums at 2^24 and beyond 2^32 (K.WIDE_CASES) -----------------------------------------------------------------------------
def test_wide_planes_have_the_sums_they_name_and_the_centres_of_the_exact_sums():
    want = {"sum x 2^24 - 1": (0, K.E24 - 1), "sum x 2^24": (0, K.E24), "sum x 2^24 + 1": (0, K.E24 + 1),
            "sum y 2^24 - 1": (1, K.E24 - 1), "sum y 2^24": (1, K.E24), "sum y 2^24 + 1": (1, K.E24 + 1),
            "sum x beyond 2^32": (0, (1 << 32) + 4097)}
    assert sorted(want) == sorted(K.WIDE_CASES)
    for name, (axis, total) in want.items():
        plane = K.WIDE_CASES[name]()
        rows, status, sums = K.wide_expected(name)
        orc = K.oracle_rows(plane)
        assert len(rows) == 2 and rows["first_index"].tobytes() == orc["first_index"].tobytes() and rows["size"].tobytes() == orc["size"].tobytes()
        big, small = (0, 1) if rows["size"][0] > rows["size"][1] else (1, 0)
        assert sums[big][axis] == total, (name, sums)                       # the sum the name says, exactly
        m = K.members(plane, rows["first_index"][big])
        assert np.ptp(m[:, 0]) + 1 > 128 or np.ptp(m[:, 1]) + 1 > 64          # beyond a wave's window: the generic path
        assert rows["size"][small] == 3 and max(sums[small]) < K.E24
        assert rows[small].tobytes() == orc[small].tobytes()                 # the small cluster: the oracle's centre, always
        m, thr = K.threshold(plane)
        assert m == K.MIN and thr == np.float32(-5.0) and not K.ring_below(plane)
        if max(sums[big]) < K.E24:
            assert status == K.OK and rows.tobytes() == orc.tobytes()        # below 2^24: the oracle's rows bit for bit
        else:
            assert status == K.OK | K.INEXACT
            assert rows["cx"][big] == np.float32(sums[big][0]) / np.float32(rows["size"][big])
            assert rows["cy"][big] == np.float32(sums[big][1]) / np.float32(rows["size"][big])
            # the reference's f32 running sums: near the exact centre, not on it
            assert abs(float(rows["cx"][big]) - float(orc["cx"][big])) < 0.5 and abs(float(rows["cy"][big]) - float(orc["cy"][big])) < 0.5
    # the other sum of the three planes around 2^24 stays below it: the flag comes from the named sum alone
    for name in list(want)[:6]:
        axis = want[name][0]
        assert K.wide_expected(name)[2][0][1 - axis] < K.E24
    # 2^32: the smallest width at which 64 full rows pass it, and a sum that no 32-bit word holds
    w = K.WIDTH_32
    assert 64 * (w - 1) * w // 2 < 1 << 32 <= 64 * w * (w + 1) // 2
    plane = K.WIDE_CASES["sum x beyond 2^32"]()
    assert plane.shape[1] == w + 6 and plane.nbytes < 3.2e6 and int((plane < -5).sum()) < K.WIDE_CANDIDATES
    rows, status, sums = K.wide_expected("sum x beyond 2^32")
    assert sums[0][0] > 0xFFFFFFFF
    saturated = np.float32(0xFFFFFFFF) / np.float32(rows["size"][0])       # what a sum saturated at 2^32 - 1 gives
    wrapped = np.float32(sums[0][0] & 0xFFFFFFFF) / np.float32(rows["size"][0])  # ... and one truncated to 32 bits
    assert rows["cx"][0] != saturated and rows["cx"][0] != wrapped


# ---- agx_filter_saddles_tail --------------------------------------------------------------------------------------------------
REFINED, OUTSIDE, NOT_SADDLE, MOVED, FILTERED = 0, 1, 2, 3, 4


def filter_reference(records, status, lo=30.0, hi=60.0):
    """src/detector.rs:432-445 over the refined slots, restated with numpy float32."""
    st = np.array(status, np.uint32)
    idx = np.flatnonzero(st == REFINED)
    if len(idx) == 0:
        return st
    acc = np.float32(np.finfo(np.float32).min)
    for i in idx:  # f32::max: a NaN k never replaces acc
        k = np.float32(records[i, 2])
        if k > acc:
            acc = k
    s_max_k = np.float32(acc / np.float32(10.0))
    for i in idx:
        k, phi = np.float32(records[i, 2]), np.float32(records[i, 4])
        if not (k >= s_max_k and phi >= np.float32(lo) and phi <= np.float32(hi)):
            st[i] = FILTERED
    return st


def filter_cases():
    """-> list of (records [n, 5], status [n]): the edges of the two comparisons, non-refined slots, nothing refined."""
    def rec(k, phi):
        return [1.0, 2.0, k, 10.0, phi]
    tenth = float(np.float32(np.float32(7.0) / np.float32(10.0)))
    below = float(np.nextafter(np.float32(tenth), np.float32(0)))
    edge = (np.array([rec(7.0, 45), rec(tenth, 45), rec(below, 45), rec(5, 30), rec(5, 60), rec(5, float(np.nextafter(np.float32(30), np.float32(0)))),
                      rec(5, float(np.nextafter(np.float32(60), np.float32(90)))), rec(float("nan"), 45), rec(5, float("nan")), rec(1000.0, 45), rec(900.0, 45)],
                     np.float32),
            np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, OUTSIDE, MOVED], np.uint32))  # the two large k are not refined: they do not enter the max
    none = (np.array([rec(3, 45), rec(4, 45)], np.float32), np.array([NOT_SADDLE, OUTSIDE], np.uint32))
    one = (np.array([rec(0.0, 45)], np.float32), np.array([0], np.uint32))
    rng = np.random.RandomState(5)
    n = 300  # several rounds of a 64-lane loop
    rand = (np.stack([rng.rand(n), rng.rand(n), rng.rand(n) * 50, rng.rand(n) * 360 - 180, rng.rand(n) * 90], 1).astype(np.float32),
            (rng.rand(n) < 0.3).astype(np.uint32) * rng.randint(1, 4, n).astype(np.uint32))
    return [edge, none, one, rand]


def test_filter_saddles_tail_is_the_references_filter():
    import aprilgrid_rs_amd as A
    for records, status in filter_cases():
        got = A.filter_saddles(records, status)
        assert np.array_equal(got, filter_reference(records, status))
    records, status = filter_cases()[0]
    got = A.filter_saddles(records, status)
    assert list(got) == [0, 0, FILTERED, 0, 0, FILTERED, FILTERED, FILTERED, FILTERED, OUTSIDE, MOVED]
    prm = A.DetectorParams(0.3, 40.0, 50.0, 2)
    assert np.array_equal(A.filter_saddles(records, status, prm), filter_reference(records, status, 40.0, 50.0))
    assert len(A.filter_saddles(np.zeros((0, 5), np.float32), np.zeros(0, np.uint32))) == 0
