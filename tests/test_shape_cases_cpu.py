"""What tests/test_gpu_flood_geometry.py reaches, proven from the oracle alone: the committed tables of tests/shape_cases.py
are classified again and every class the GPU test is there for must be present.  Editing a table so that a class is lost
fails here, without a GPU."""
import numpy as np
import pytest

from tests import shape_cases as S


@pytest.fixture(scope="module")
def flood():
    """[(case, components)] of every FLOOD_CASES entry (components() asserts itself against the oracle's cluster table)."""
    return [(c, S.components(S.make_case(c))) for c in S.FLOOD_CASES]


def _clean(flood):
    """Frames without a component on the second window's edge or beyond it: only there do the flood windows decide the
    result (such a component sends the whole frame to the generic path)."""
    return [(c, comp) for c, comp in flood if not S.at_second_tier_limit(comp).any()]


def test_flood_cases_are_small_and_of_three_formats(flood):
    assert {c[0] for c, _ in flood} == {"L8", "L16", "LF32"}
    assert all((c[1], c[2]) == (160, 256) for c, _ in flood) and len(flood) <= 24


@pytest.mark.parametrize("field,values", [("L", (13, 14, 15, 16, 17, 63, 64)), ("R", (13, 14, 15, 16, 17, 62, 63)),
                                          ("D", (29, 30, 61, 62))])
def test_every_reach_value_at_the_window_limits_occurs(flood, field, values):
    reached = np.concatenate([comp[field] for _, comp in _clean(flood)])
    # the limit itself (the last value): a frame that no component beyond the window sends to the generic path anyway
    at_limit = np.concatenate([comp[field] for _, comp in flood if not S.beyond_second_tier(comp).any()])
    for v in values[:-1]:
        assert (reached == v).any(), "no canonical component with %s = %d in a frame that stays on the flood path" % (field, v)
    assert (at_limit == values[-1]).any(), "no canonical component with %s = %d" % (field, values[-1])


@pytest.mark.parametrize("field", ["L", "R"])
def test_first_tier_limits_occur_at_three_seed_alignments(flood, field):
    comp = np.concatenate([comp for _, comp in _clean(flood)])
    for v in (13, 14, 15, 16, 17):
        classes = set((comp["sx"][comp[field] == v] & 3).tolist())
        assert len(classes) >= 3, "%s = %d only at sx & 3 in %s" % (field, v, sorted(classes))


def test_second_tier_windows_at_both_word_alignments_and_in_the_padding(flood):
    sel = [(c, comp[S.inside_second_tier(comp)]) for c, comp in _clean(flood)]
    comp = np.concatenate([k for _, k in sel])
    sh = (comp["sy"] - 1) & 31
    assert (sh == 0).any() and (sh == 31).any()
    assert (comp["sx"] < 64).any(), "no second-tier window reaches into the left padding"
    assert any((k["sx"] > c[2] - 64).any() for c, k in sel), "... into the right padding"
    assert any((k["sy"] + 62 >= c[1]).any() for c, k in sel), "... below the last row"


def test_components_beyond_the_second_tier_in_each_direction_alone(flood):
    comp = np.concatenate([comp for _, comp in flood])
    L, R, D = comp["L"], comp["R"], comp["D"]
    assert ((L >= 65) & (R < 62) & (D < 61)).any()
    assert ((R >= 64) & (L < 63) & (D < 61)).any()
    assert ((D >= 63) & (L < 63) & (R < 62)).any(), "no tall and thin component"
    # ... and each direction in a frame that nothing else sends to the generic path
    keys = set().union(*[S.flood_classes(comp, c[1], c[2]) for c, comp in flood])
    assert {("beyond_only", "L"), ("beyond_only", "R"), ("beyond_only", "D")} <= keys


def test_two_frames_stay_in_the_first_tier_next_to_frames_that_do_not(flood):
    for fmt in ("L8", "L16", "LF32"):
        batch = [comp for c, comp in flood if c[0] == fmt]
        small = [len(comp) > 0 and bool(S.stays_first_tier(comp).all()) for comp in batch]
        assert any(small) and not all(small), fmt
    assert sum(len(comp) > 0 and bool(S.stays_first_tier(comp).all()) for _, comp in flood) >= 2


def test_integer_translation_moves_every_component(flood):
    """ox / oy are whole-pixel translations: away from the borders the same components, moved."""
    fmt, h, w, px, py, th, ox, oy = S.FLOOD_CASES[11]
    a = S.components(S.sine_frame(h, w, px, py, th, 0, 0, fmt))
    b = S.components(S.sine_frame(h, w, px, py, th, 3, 5, fmt))
    inner = lambda c, x0, y0: c[(c["sx"] - c["L"] > x0 + 8) & (c["sx"] + c["R"] < w - 12 + x0) & (c["sy"] > y0 + 8) & (c["sy"] + c["D"] < h - 12 + y0)]
    a, b = inner(a, 0, 0), inner(b, 3, 5)
    assert len(a) == len(b) > 50
    assert np.array_equal(a["sx"] + 3, b["sx"]) and np.array_equal(a["sy"] + 5, b["sy"]) and np.array_equal(a["size"], b["size"])


# ---- late minima ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["L8", "L16", "LF32"])
@pytest.mark.parametrize("where", S.LATE_MIN_WHERE)
def test_late_minimum_frames_meet_their_conditions(fmt, where):
    """The response minimum lies in the intended strip x segment, the texture sits at the threshold: between 1 % and 70 % of
    the interior pixels are candidates and at least 2 000 per 64 k lie within a factor two of the threshold."""
    for ratio in S.LATE_MIN_RATIOS:
        d = S.oracle_planes(S.late_min_frame(200, 320, where, ratio, fmt))
        inside, share, straddle = S.late_min_conditions(d, S.late_min_target(200, 320, where)[2])
        assert inside and 0.01 <= share <= 0.70 and straddle >= 2000, (fmt, where, ratio, inside, share, straddle)


@pytest.mark.parametrize("where,ratio", list(zip(S.LATE_MIN_WHERE, S.LATE_MIN_RATIOS)))
def test_late_minimum_frames_of_more_than_128_units(where, ratio):
    strip_cols, n_strips, rps, n_segs, mid = S.k1_tiling(810, 1280)
    assert (n_strips, n_segs) == (6, 26) and n_strips * n_segs > 128  # K1's publish_factor 1.5
    d = S.oracle_planes(S.late_min_frame(810, 1280, where, ratio, "L16"))
    inside, share, straddle = S.late_min_conditions(d, S.late_min_target(810, 1280, where)[2])
    assert inside and 0.01 <= share <= 0.70 and straddle >= 2000, (where, ratio, inside, share, straddle)


def test_late_minimum_targets_are_the_segments_meant():
    assert S.k1_tiling(200, 320) == (160, 2, 32, 7, 2)  # two strips, seven segments, the last one short; 2 goes first
    assert S.late_min_target(200, 320, "top_left")[2] == (0, 160, 0, 32)
    assert S.late_min_target(200, 320, "middle")[2] == (160, 320, 64, 96)
    assert S.late_min_target(200, 320, "bottom_right")[2] == (160, 320, 192, 200)
    assert S.late_min_target(810, 1280, "bottom_right")[2] == (1120, 1280, 800, 810)


# ---- centroid sums of 2^24 and more ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,sum_x", list(zip(S.CENTROID_CASES, (29864986, 61655144))))
def test_centroid_cases_have_a_coordinate_sum_beyond_2_to_24(case, sum_x):
    """One frame-spanning cluster whose sum of x is 2^24 or more (the device then adds integers where the reference adds
    f32).  The exact centroid and the oracle's f32 running-sum centroid agree within 0.05 px and round to the same pixel,
    which is all the reference uses of it (detector.rs: initial.round()), so the saddle lists must equal the oracle's."""
    h, w, px, py, th = case
    d = S.oracle_planes(S.sine_frame(h, w, px, py, th))
    comp = S.components(None, d)
    big = np.flatnonzero(np.maximum(comp["sum_x"], comp["sum_y"]) >= 2 ** 24)
    assert len(big) == 1 and int(comp["sum_x"][big[0]]) == sum_x, comp[big]
    c = comp[big[0]]
    exact = (np.float32(c["sum_x"]) / np.float32(c["size"]), np.float32(c["sum_y"]) / np.float32(c["size"]))
    ref = d["centers"][big[0]]
    assert abs(float(exact[0]) - float(ref[0])) < 0.05 and abs(float(exact[1]) - float(ref[1])) < 0.05, (exact, ref)
    assert np.floor(exact[0] + 0.5) == np.floor(ref[0] + 0.5) and np.floor(exact[1] + 0.5) == np.floor(ref[1] + 0.5)  # (f32::round)
    # every other cluster: sums far below 2^24, where f32 running sums are exact
    others = np.delete(np.arange(len(comp)), big)
    assert len(others) > 100 and max(comp["sum_x"][others].max(), comp["sum_y"][others].max()) < 2 ** 24
    ex = (comp["sum_x"][others].astype(np.float32) / comp["size"][others].astype(np.float32))
    assert np.array_equal(ex.view(np.uint32), d["centers"][others, 0].view(np.uint32))
