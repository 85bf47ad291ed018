"""agx_snap_points_tail -- caller points snapped to the nearest listed saddle, the host form -- against a numpy float32 brute
force (tests/snap_cases.py), its argument and status rules, and the tracked detect built from it on the golden lists and on the
GPU tests' frames against agx_detect_tail.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import snap_cases as S
from tests.test_find_boards_cpu import GPU_FIRST, GPU_FRAMES, GPU_SIZE, golden_list
from tests.util import ALL_IMAGES, ROOT, bits_equal, load_image

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

F32 = np.float32
NONE = S.NONE
SINGLE_BOARD = [n for n in ALL_IMAGES if n != "two_boards.png"]


def random_list(rng, n, span=200.0):
    s = np.zeros((n, 5), F32)
    s[:, :2] = rng.uniform(0, span, (n, 2)).astype(F32)
    s[:, 2:] = rng.uniform(-50, 50, (n, 3)).astype(F32)
    return s


def both(s, pts, max_dist_sq, words=None, reverse=False, what="", **kw):
    r = S.Raw(s, pts, max_dist_sq, words=words, flags=_ffi.AGX_SNAP_REVERSE if reverse else 0, **kw)
    r.check(S.numpy_snap(s, pts, max_dist_sq, words=words, reverse=reverse), what)
    return r


# ---- 1. the host form against the numpy brute force ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 700])
@pytest.mark.parametrize("ppr", [1, 2, 3, 4])
def test_random_lists_and_points(n, ppr):
    rng = np.random.default_rng(100 * n + ppr)
    s = random_list(rng, n)
    pts = rng.uniform(-10, 210, (37, ppr, 2)).astype(F32)
    if n:  # some points right beside a saddle: whole rows snap
        at = rng.integers(0, n, (20, ppr))
        pts[:20] = s[at, :2] + rng.uniform(-1, 1, (20, ppr, 2)).astype(F32)
    for reverse in (False, True):
        for limit in (0.0, 2.0, 150.0, np.inf):
            both(s, pts, limit, reverse=reverse, what="n %d ppr %d limit %g" % (n, ppr, limit))
    both(s, pts[:0], 4.0, what="no rows")
    both(s, pts, 4.0, with_dist=False, with_index=False, what="optional outputs absent")


def test_exact_ties_go_to_the_lowest_slot():
    g = np.arange(0, 8, dtype=F32) * 2
    s = np.zeros((64, 5), F32)
    s[:, 0], s[:, 1] = np.tile(g, 8), np.repeat(g, 8)
    s = s[np.random.default_rng(3).permutation(64)]
    pts = np.array([[[1, 1], [3, 1], [1, 3], [3, 3]], [[5, 5], [7, 5], [2, 3], [13, 13]]], F32)  # cell centres: four saddles at d2 = 2
    r = both(s, pts, 2.0, what="ties")
    slots = r.slots[:8].reshape(2, 4)
    for row, pt in zip(slots.reshape(-1), pts.reshape(-1, 2)):
        d2 = (s[:, 0] - pt[0]) ** 2 + (s[:, 1] - pt[1]) ** 2
        assert row == np.flatnonzero(d2 == d2.min())[0] and (d2 == d2.min()).sum() in (2, 4)
    # the same saddle twice in the list: the first of the two
    s2 = np.concatenate([s, s])
    r2 = both(s2, pts, 2.0, what="a list that repeats itself")
    assert (r2.slots[:8] < 64).all()


def test_the_limit_is_the_squared_distance_itself_to_the_last_bit():
    s = np.zeros((2, 5), F32)
    s[0, :2], s[1, :2] = (10, 10), (500, 500)
    pts = np.array([[[13, 14]]], F32)  # d2 = 25 exactly
    at, below, above = F32(25.0), np.nextafter(F32(25.0), F32(0)), np.nextafter(F32(25.0), F32(100))
    assert both(s, pts, at).slots[0] == 0
    assert both(s, pts, above).slots[0] == 0
    r = both(s, pts, below)
    assert r.slots[0] == NONE and r.dist.view(F32)[0] == F32(25.0) and r.kept.value == 0  # (the distance is still reported)
    # and a d2 that is not a whole number: the limit one bit either side of it
    pts = np.array([[[10.3, 11.7]]], F32)
    d2 = S.numpy_snap(s, pts, np.inf)[1][0, 0]
    assert both(s, pts, d2).slots[0] == 0 and both(s, pts, np.nextafter(d2, F32(0))).slots[0] == NONE
    assert both(s, pts, -0.0).slots[0] == NONE and both(s, np.array([[[10, 10]]], F32), -0.0).slots[0] == 0  # (-0.0 is 0)


def test_status_words_exclude_the_true_nearest():
    rng = np.random.default_rng(5)
    s = random_list(rng, 300)
    at = rng.integers(0, 300, (30, 4))
    pts = s[at, :2] + F32(0.25)
    words = np.zeros(300, np.uint32)
    words[at[:10].reshape(-1)] = rng.choice([1, 2, 3, 4, 5], 40)  # every AGX_POINT_* but REFINED
    r = both(s, pts, 100.0, words=words, what="status words")
    assert not np.isin(r.slots[:120], np.flatnonzero(words)).any()
    flat = at.reshape(-1)
    assert (r.slots[:40] != flat[:40]).all() and (r.slots[:120][words[flat] == 0] == flat[words[flat] == 0]).all()
    both(s, pts, 100.0, words=np.ones(300, np.uint32), what="nothing listed")


def test_a_row_with_two_points_on_one_slot_is_dropped_and_slots_show_both():
    s = random_list(np.random.default_rng(6), 50)
    pts = np.stack([s[[1, 2, 3, 4], :2], s[[5, 6, 5, 7], :2], s[[8, 9, 10, 11], :2], s[[8, 9, 10, 11], :2]]).astype(F32)
    r = both(s, pts, 1.0, what="a doubled slot")
    assert r.slots[4:8].tolist() == [5, 6, 5, 7] and r.kept.value == 3
    assert r.index[:3].tolist() == [0, 2, 3] and r.rows[4:8].tolist() == r.rows[8:12].tolist() == [8, 9, 10, 11]  # equal rows: both kept


def test_nan_and_inf_points_never_snap():
    s = random_list(np.random.default_rng(7), 20)
    pts = np.array([[[np.nan, 5], [5, np.nan]], [[np.inf, 5], [5, -np.inf]], [[3e38, 3e38], [-3e38, 0]], s[[0, 1], :2]], F32)
    r = both(s, pts, np.inf, what="points that are not finite")
    assert (r.slots[:6] == NONE).all() and np.isinf(r.dist.view(F32)[:6]).all() and r.kept.value == 1


def test_reverse_reads_a_row_back_to_front():
    s = random_list(np.random.default_rng(8), 40)
    pts = s[[[3, 9, 27, 5]], :2].astype(F32)
    assert both(s, pts, 1.0).slots[:4].tolist() == [3, 9, 27, 5]
    r = both(s, pts, 1.0, reverse=True)
    assert r.slots[:4].tolist() == [5, 27, 9, 3] and r.rows[:4].tolist() == [5, 27, 9, 3]
    assert both(s, pts[:, :3], 1.0, reverse=True).slots[:3].tolist() == [27, 9, 3]


def test_a_tag_table_is_read_in_place():
    rng = np.random.default_rng(9)
    s = random_list(rng, 120)
    tags = np.zeros(9, S.TAG)
    tags["id"] = rng.integers(0, 587, 9)
    at = rng.integers(0, 120, (9, 4))
    tags["xy"] = (s[at, :2] + F32(0.5)).reshape(9, 8)
    pts = tags["xy"].reshape(9, 4, 2)
    for reverse in (False, True):
        want = S.numpy_snap(s, pts, 3.0, reverse=reverse)
        r = S.Raw(s, None, 3.0, flags=int(reverse), n_rows=9, ppr=4, row_stride=tags.dtype.itemsize, point_stride=8, p_points=tags.ctypes.data + 4)
        r.check(want, "sizeof(agx_tag) rows")
        got = A.snap_points(s, tags, 3.0, reverse=reverse)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]
    # a point stride of its own: x, y in a 20-byte record
    rec = np.zeros((5, 3, 5), F32)
    rec[:, :, :2] = s[rng.integers(0, 120, (5, 3)), :2]
    r = S.Raw(s, None, 1.0, n_rows=5, ppr=3, row_stride=60, point_stride=20, p_points=rec.ctypes.data)
    r.check(S.numpy_snap(s, rec[:, :, :2], 1.0), "20-byte points")


def test_k_theta_and_phi_are_never_read():
    rng = np.random.default_rng(10)
    s = random_list(rng, 60)
    pts = rng.uniform(0, 200, (8, 4, 2)).astype(F32)
    want = S.numpy_snap(s, pts, 400.0)
    s[:, 2:] = np.nan
    S.Raw(s, pts, 400.0).check(want, "NaN in k, theta, phi")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("column", [0, 1])
def test_a_listed_saddle_that_is_not_finite_is_snap_input(column, value):
    s = random_list(np.random.default_rng(11), 33)
    pts = s[[[0, 1, 2, 3]], :2].astype(F32)
    s[32, column] = value
    r = both(s, pts, 1.0, what="a saddle that is not finite")
    assert r.status.value == _ffi.AGX_SNAP_INPUT
    words = np.zeros(33, np.uint32)
    words[32] = _ffi.AGX_POINT_FILTERED  # not listed: not looked at
    assert both(s, pts, 1.0, words=words).status.value == _ffi.AGX_SNAP_OK


def test_argument_rules():
    s = random_list(np.random.default_rng(12), 10)
    pts = s[[[0, 1, 2, 3], [4, 5, 6, 7]], :2].astype(F32)
    E = _ffi.AGX_ERR_ARG
    ok = S.Raw(s, pts, 1.0)
    assert ok.rc == _ffi.AGX_OK and ok.kept.value == 2
    for null in ("saddles", "points", "slots", "rows", "kept", "status"):
        assert S.Raw(s, pts, 1.0, null=(null,)).rc == E, null
    assert S.Raw(s[:0], pts[:0], 1.0, null=("points", "slots", "rows")).rc == _ffi.AGX_OK  # (nothing to read or write)
    for ppr in (0, 5):
        assert S.Raw(s, pts, 1.0, ppr=ppr).rc == E
    for kw in (dict(row_stride=34), dict(point_stride=10), dict(point_stride=4), dict(row_stride=28), dict(point_stride=12)):
        assert S.Raw(s, pts, 1.0, **kw).rc == E, kw  # not a multiple of 4; points that overlap; a row stride that does not cover the row
    assert S.Raw(s, pts, 1.0, row_stride=32, point_stride=8).rc == _ffi.AGX_OK
    for limit in (-1.0, -np.inf, np.nan, -1e-45):
        assert S.Raw(s, pts, limit).rc == E, limit
    assert S.Raw(s, pts, np.inf).rc == _ffi.AGX_OK
    for flags in (2, 3, -1, 1 << 30):
        assert S.Raw(s, pts, 1.0, flags=flags).rc == E
    assert S.Raw(s, None, 1.0, n_rows=2, ppr=4, row_stride=32, p_points=pts.ctypes.data + 2).rc == E  # misaligned
    assert S.Raw(s, pts, 1.0, n_rows=1 << 27).rc == E
    for r in (S.Raw(s, pts, -1.0), S.Raw(s, pts, 1.0, ppr=5)):  # a refused call writes nothing
        assert (r.slots == S.SENTINEL).all() and r.kept.value == 77 and r.status.value == 77


def test_constants_and_declarations_agree_in_header_python_and_rust():
    hdr = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name, value in (("AGX_SNAP_REVERSE", 1), ("AGX_SNAP_OK", 0), ("AGX_SNAP_INPUT", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr) and getattr(_ffi, name) == value
        assert "pub const %s: c_int = %d;" % (name, value) in ffi
    assert "#define AGX_SNAP_NONE 0xFFFFFFFFu" in hdr and _ffi.AGX_SNAP_NONE == 0xFFFFFFFF and "pub const AGX_SNAP_NONE: u32 = 0xFFFF_FFFF;" in ffi
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn snap_points_tail<const N: usize>(" in lib_rs and "ffi::agx_snap_points_tail(" in lib_rs
    for name in ("agx_snap_points_enqueue", "agx_snap_points_tail"):
        assert name in _ffi.SYMBOLS and hasattr(_ffi.lib(), name)
    assert _ffi.lib().agx_abi_version() == 1  # (a new entry does not change the version: the earlier ones did not)


# ---- 2. a tracked detect from the host forms against agx_detect_tail -------------------------------------------------------------
def same_tags(got, ref, what):
    assert sorted(got) == sorted(ref), "%s: ids %s missing, %s extra" % (what, sorted(set(ref) - set(got)), sorted(set(got) - set(ref)))
    for t in ref:
        assert bits_equal(got[t], ref[t]), "%s: corners of tag %d" % (what, t)


@pytest.mark.parametrize("name", SINGLE_BOARD)
def test_tracking_a_golden_list_from_its_own_tags_equals_detect_tail(name):
    s = golden_list(name)
    luma = A.TagDetector.luma8(load_image(name))
    ref = A.TagDetector.detect_tail("t36h11", s, luma)
    assert len(ref) >= 36
    for shift in S.SHIFTS:
        got, seeds, board = S.tracked_rounds(s, luma, S.tag_rows(ref, shift))
        assert seeds == len(ref) and board == _ffi.AGX_BOARD_FOUND
        same_tags(got, ref, "%s shifted by %s" % (name, shift))


def test_tracking_two_boards_pins_what_the_composition_gives():
    """The image with two boards: detect finds 72 tags, the tracked composition 71 -- every tag but id 66, with detect's corner
    bits -- at each of the three shifts.  All 72 prior rows are seeds of the first round, so the board it grows is chosen among
    seeds of both boards, and the rounds do not split the saddles as detect's search does.  Pinned, not claimed equal."""
    name = "two_boards.png"
    s = golden_list(name)
    luma = A.TagDetector.luma8(load_image(name))
    ref = A.TagDetector.detect_tail("t36h11", s, luma)
    assert len(ref) == 72
    for shift in S.SHIFTS:
        got, seeds, board = S.tracked_rounds(s, luma, S.tag_rows(ref, shift))
        assert seeds == 72 and board == _ffi.AGX_BOARD_FOUND
        assert sorted(set(ref) - set(got)) == [66] and not set(got) - set(ref), shift
        for t in got:
            assert bits_equal(got[t], ref[t]), "corners of tag %d" % t


def test_tracking_the_gpu_tests_frames_equals_detect_tail():
    """synth.render_batch(0, 8, 640, 400), the frames tests/test_gpu_snap_points.py runs detect_tracked on, from the oracle's
    saddle lists: all 8 frames agree at every shift (first frame index 0; none had to be left out or moved)."""
    from oracle import oracle as O
    from aprilgrid_rs_amd import synth
    frames, _ = synth.render_batch(GPU_FIRST, GPU_FRAMES, *GPU_SIZE)
    for f in range(GPU_FRAMES):
        img = frames[f].numpy()
        s = O.refined_saddle_points(img)
        ref = A.TagDetector.detect_tail("t36h11", s, img)
        assert len(ref) >= 30
        for shift in S.SHIFTS:
            got, seeds, board = S.tracked_rounds(s, img, S.tag_rows(ref, shift))
            assert seeds == len(ref) and board == _ffi.AGX_BOARD_FOUND
            same_tags(got, ref, "synthetic frame %d shifted by %s" % (f, shift))
