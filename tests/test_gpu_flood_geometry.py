"""Parity where the other inputs of the suite never go (tests/shape_cases.py; what the tables reach is proven on the CPU by
tests/test_shape_cases_cpu.py):
  * candidate components exactly at the limits of the two flood windows, at every seed alignment, with second-tier windows
    in the mask's padding, and components that leave the second window in one direction only;
  * frames whose one deep response minimum lies in the K1 segment dispatched first, in the first, or in the short last one,
    with the rest of the frame at the candidate threshold 0.05 * min (largest superset, largest re-test volume);
  * clusters whose coordinate sums reach 2^24 (AGX_FRAME_CENTROID_INEXACT, the one documented deviation).
"""
import numpy as np
import pytest

from tests import shape_cases as S
from tests.util import bits_equal, check_centroids, check_frame, check_planes_and_tables, check_saddles, synth_module

pytestmark = pytest.mark.gpu

COUNTERS = ("flags", "clusters", "refined", "saddles", "big_seeds")


class _Oracle:
    """The oracle with its results kept per image: every leg of a test compares with the same, unchanged reference."""

    def __init__(self):
        from oracle import oracle as O
        O.lib()
        self._o, self._kept = O, {}

    def refined_saddle_points(self, img, params=None, debug=False):
        assert params is None
        key = (id(img), debug)
        if key not in self._kept:
            self._kept[key] = (img, self._o.refined_saddle_points(img, debug=debug))  # (img kept alive: its id stays its own)
        return self._kept[key][1]


@pytest.fixture(scope="module")
def oracle():
    return _Oracle()


def _device(frames):
    import torch
    a = np.stack(frames)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _run(frames_dev, host, oracle, what, options=(), expect_path=None, max_saddles=0):
    """One batch on a fresh detector -> (records as bytes, counters); every frame checked against the oracle."""
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    try:
        for k, v in options:
            d.set_option(k, v)
        if max_saddles:
            d.set_limits(max_saddles=max_saddles)
        d.saddles_batch_enqueue(frames_dev)
        res, status = d.saddles_batch_fetch()
        assert (status == 0).all(), (what, status)
        if expect_path is not None:
            assert d.get_option("last_sparse_path") == expect_path, what
        for i, img in enumerate(host):
            check_saddles(res[i], check_frame(d, oracle, img, i, "%s frame %d" % (what, i)), "%s frame %d" % (what, i))
        return [r.tobytes() for r in res], [d.debug_fetch(i, "counters") for i in range(len(host))]
    finally:
        d.close()


@pytest.fixture(scope="module")
def flood_frames():
    """fmt -> ([case], [host frame], [components]) of FLOOD_CASES."""
    out = {}
    for c in S.FLOOD_CASES:
        cases, host, comps = out.setdefault(c[0], ([], [], []))
        img = S.make_case(c)
        cases.append(c)
        host.append(img)
        comps.append(S.components(img))
    return out


@pytest.mark.parametrize("fmt", ["L16", "L8", "LF32"])
def test_components_at_the_flood_window_limits(oracle, flood_frames, fmt):
    """All cases of one format as one device batch, on the three sparse paths and on the generic path: every frame has the
    oracle's planes, minimum, cluster table (first pixel, size, centroid bit for bit) and lists; the three paths agree byte
    for byte and counter for counter.  The counters are checked in one direction only (no rule of the kernel restated): a
    frame with a component surely beyond the second window took the generic path, a frame whose components all fit the
    first window sent no seed on, and the batch as a whole used the second tier."""
    cases, host, comps = flood_frames[fmt]
    dev = _device(host)
    got = {p: _run(dev, host, oracle, "%s path %d" % (fmt, p), (("sparse_path", p),), p) for p in (1, 2, 3)}
    for p in (2, 3):
        assert got[p][0] == got[1][0], "records of path %d differ from path 1" % p
        for i, (ca, cb) in enumerate(zip(got[p][1], got[1][1])):
            for k in COUNTERS:
                assert ca[k] == cb[k], (p, cases[i], k, ca, cb)
    generic = _run(dev, host, oracle, "%s generic path" % fmt, (("force_generic", 1),))
    assert generic[0] == got[1][0], "records of the generic path differ from the flood path"
    ctr = got[1][1]
    for case, comp, c in zip(cases, comps, ctr):
        print(case, "L<=%d R<=%d D<=%d" % (comp["L"].max(), comp["R"].max(), comp["D"].max()), c)
        if S.beyond_second_tier(comp).any():
            assert c["flags"] & 16, (case, c)
        if S.stays_first_tier(comp).all():
            assert c["big_seeds"] == 0 and not (c["flags"] & 16), (case, c)
    assert sum(c["big_seeds"] for c in ctr) > 0
    assert any(S.beyond_second_tier(comp).any() for comp in comps) and any(S.stays_first_tier(comp).all() for comp in comps)


def test_flood_cases_as_single_frames(oracle, flood_frames):
    """The L16 cases one by one through refined_saddle_points: few waves, the other K1 and sparse planning."""
    import aprilgrid_rs_amd as A
    cases, host, comps = flood_frames["L16"]
    d = A.TagDetector("t36h11", None, device=0)
    for case, img, comp in zip(cases, host, comps):
        got = d.refined_saddle_points(img, as_array=True)
        check_saddles(got, check_frame(d, oracle, img, 0, str(case)), str(case))
        c = d.debug_fetch(0, "counters")
        if S.beyond_second_tier(comp).any():
            assert c["flags"] & 16, (case, c)
        if S.stays_first_tier(comp).all():
            assert c["big_seeds"] == 0 and not (c["flags"] & 16), (case, c)
    d.close()


# ---- late minima --------------------------------------------------------------------------------------------------------
def _late_frames(h, w, fmt, pairs):
    return [S.late_min_frame(h, w, where, ratio, fmt) for where, ratio in pairs]


ALL_PAIRS = [(where, ratio) for where in S.LATE_MIN_WHERE for ratio in S.LATE_MIN_RATIOS]


def _late_legs(monkeypatch, oracle, host, what, max_saddles=0):
    import torch
    import aprilgrid_rs_amd as A
    dev = _device(host)
    got = {}
    for poll in ("0", "1"):
        monkeypatch.setenv("AGX_K1_ASYNC_POLL", poll)  # (a new detector reads it)
        for path in (1, 2, 3):
            for rows in (32, 96):
                leg = "%s poll %s path %d rows %d" % (what, poll, path, rows)
                got[leg] = _run(dev, host, oracle, leg, (("sparse_path", path), ("k1_rows_per_segment", rows)), path, max_saddles)[0]
    first = next(iter(got))
    for leg in got:
        assert got[leg] == got[first], "%s differs from %s" % (leg, first)
    monkeypatch.delenv("AGX_K1_ASYNC_POLL")
    d = A.TagDetector("t36h11", None, device=0)  # (creating a detector reads the environment again: the override is gone)
    d.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", ["L8", "L16", "LF32"])
def test_late_minimum_batch_all_legs(monkeypatch, oracle, fmt):
    """200 x 320 (two strips, seven segments, the last one short): one batch of every position x ratio.  Both poll forms,
    the three sparse paths, segments of 32 and 96 rows: each leg has the oracle's planes, per-frame minimum (nine different
    ones in one batch: no frame's minimum leaks into another's threshold), cluster tables and lists, and the legs are
    byte-identical."""
    _late_legs(monkeypatch, oracle, _late_frames(200, 320, fmt, ALL_PAIRS), "late %s" % fmt)


def test_late_minimum_more_than_128_units(monkeypatch, oracle):
    """810 x 1280: 6 strips x 26 segments, so the waves publish only minima 1.5 times below the known one.  (About 16 500
    saddles per frame, more than the default list of one per 64 pixels: the limit is raised as a caller would.)"""
    host = _late_frames(810, 1280, "L16", list(zip(S.LATE_MIN_WHERE, S.LATE_MIN_RATIOS)))
    _late_legs(monkeypatch, oracle, host, "late 810x1280", max_saddles=1 << 15)


def test_late_minimum_frames_are_retested():
    """The verify kernel's statistics (debug_ablation 128): K1's superset of these frames has bits k_verify_seeds must
    re-test.  Their volume against board frames of the same size is printed, not asserted.  Measured on an MI355X, nine
    200 x 320 L8 frames each: 20 245 ... 27 449 re-tested bits per late-minimum frame (74 ... 100 % of K1's candidate bits)
    against 635 ... 3 384 per board frame (10 ... 67 %), ratio of the means 11.45."""
    import aprilgrid_rs_amd as A
    synth = synth_module()
    d = A.TagDetector("t36h11", None, device=0)
    d.set_option("debug_ablation", 128)

    def retest_bits(dev, n):
        d.saddles_batch_enqueue(dev)
        d.sync()
        st = [d.debug_fetch(i, "verify_stats").astype(np.int64) for i in range(n)]
        return [int(s[[3, 7, 11, 15]].sum()) for s in st], [int(s[[1, 5, 9, 13]].sum()) for s in st]

    late, late_all = retest_bits(_device(_late_frames(200, 320, "L8", ALL_PAIRS)), len(ALL_PAIRS))
    boards, _ = synth.render_batch(5, len(ALL_PAIRS), 320, 200, device="cuda")
    board, board_all = retest_bits(boards, len(ALL_PAIRS))
    d.close()
    print("re-tested bits per frame: late minima %s of %s candidates, boards %s of %s; ratio of the means %.2f"
          % (late, late_all, board, board_all, np.mean(late) / max(1.0, np.mean(board))))
    assert all(b > 0 for b in late), late


# ---- coordinate sums of 2^24 and more -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CENTROID_CASES, ids=["128x2048", "96x3000"])
def test_centroid_of_a_cluster_with_sums_beyond_2_to_24(oracle, case):
    """One net of candidates across the whole frame: its sum of x (29 864 986 / 61 655 144) is beyond what f32 adds exactly,
    the device adds integers and sets AGX_FRAME_CENTROID_INEXACT (8).  Planes, minimum, cluster count, first pixels and
    sizes are the oracle's; every cluster with sums below 2^24 has the oracle's centroid bit for bit; the big one has
    f32(sum) / f32(n) of the exact integer sums, exactly -- the reference's f32 running sum differs from it by
    0.0026 px (1020.5716 against 1020.5742) and 0.0185 px (1485.6304 against 1485.6119) in x, below the 0.05 px asserted.
    Both round to the same pixel, and the reference uses only initial.round(): the refined and the filtered list are
    the oracle's."""
    import aprilgrid_rs_amd as A
    h, w, px, py, th = case
    img = S.sine_frame(h, w, px, py, th)
    dev = _device([img])
    records = []
    for options in ((), (("sparse_path", 2),), (("sparse_path", 3),), (("force_generic", 1),)):
        d = A.TagDetector("t36h11", None, device=0)
        for k, v in options:
            d.set_option(k, v)
        d.saddles_batch_enqueue(dev)
        res, status = d.saddles_batch_fetch()
        assert (status == 0).all()
        what = "%dx%d %s" % (h, w, options)
        ref, dbg, c = check_planes_and_tables(d, oracle, img, 0, what)
        flags = d.debug_fetch(0, "counters")["flags"]
        assert flags & 8 and not (flags & ~(8 | 16)), (what, flags)
        comp = S.components(img, dbg)
        exact = np.maximum(comp["sum_x"], comp["sum_y"]) < 2 ** 24
        assert np.count_nonzero(~exact) == 1 and np.count_nonzero(exact) > 100
        check_centroids(c, dbg, what, np.flatnonzero(exact))
        b = int(np.flatnonzero(~exact)[0])
        cx = np.float32(comp["sum_x"][b]) / np.float32(comp["size"][b])
        cy = np.float32(comp["sum_y"][b]) / np.float32(comp["size"][b])
        print(what, "big cluster: device", c["cx"][b], c["cy"][b], "exact", cx, cy, "oracle", dbg["centers"][b])
        assert bits_equal(c["cx"][b:b + 1], cx) and bits_equal(c["cy"][b:b + 1], cy), (what, c[b], cx, cy)
        assert abs(float(c["cx"][b]) - float(dbg["centers"][b, 0])) < 0.05 and abs(float(c["cy"][b]) - float(dbg["centers"][b, 1])) < 0.05
        check_saddles(d.debug_fetch(0, "refined"), dbg["refined"], what + " (unfiltered)")
        check_saddles(res[0], ref, what)
        records.append(res[0].tobytes())
        d.close()
    assert all(r == records[0] for r in records)
