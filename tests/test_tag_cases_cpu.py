"""The hand-painted tags of tests/tag_cases.py, proven on the CPU from the oracle and numpy alone, then given to the host form
of the decode (agx_decode_quads_tail).  Reference: decode_positions, bit_code, rotate_bits, best_tag (src/detector.rs:42-169),
try_decode_quad (:448-476).

Per family (T16H5, T25H7, T36H11, T36H11B1):
  * geometry: under orc_decode_positions alone every sample of every painted case lies at least 2 px inside a flat 8 x 8 px cell,
    the samples of a case take every cell once, and under the standard quad sample n takes the cell of row border + n / edge,
    column border + n % edge.  A coordinate is about 4e-5 px uncertain (tests/test_decode_quads_cpu.py), so no rounding can
    change a pixel read: these cases have NO knife-edge exclusion;
  * the half-integer cases: the oracle's float positions equal the exact rational ones, every coordinate is j + 1/2 with even
    and odd j, and the pixel at j + 1 differs by 255 from the three that another rounding would read;
  * every claim a case makes by construction (`intent`) holds under the yardstick of tests/test_decode_quads_cpu.py, and the
    yardstick equals the builder's expectation in every field;
  * the mutation table: a plain numpy restatement of the four functions (tag_cases.model) equals the yardstick on every case,
    and every one of its twelve mutations changes status, id, bits or corners of the number of cases recorded in CHANGED;
  * no two distinct (code, rotation) pairs of a family are closer than 2 * thres - 1, so two accepted candidates never compete
    (best_tag accepts a distance < thres): there is no tie to build a case for;
  * agx_decode_quads_tail equals the yardstick on every case and every field, nothing excluded.
And for the device tail's copy of the decode: the oracle's detect on the rendered boards with flipped code bits."""
import functools

import numpy as np
import pytest

from tests import tag_cases as T
from tests.tag_cases import AMBIGUOUS, DECODED, LOW_CONTRAST, NO_MATCH, OUTSIDE
from tests.test_decode_quads_cpu import TAG_DTYPE, check_zero_records, family, orc, yardstick

# Painted cases per family, by kind (tag_cases.KINDS), and of them the cases whose status, id, bits or corners each mutation
# of tag_cases.MUTATIONS changes (popcount_low32 cannot change a family of at most 32 bits).
N_CASES = {
    "T16H5": {"bit_order": 16, "extremes": 64, "mid": 48, "invalid": 66, "hamming": 15, "rotation": 50, "half": 20, "edge": 48},
    "T25H7": {"bit_order": 25, "extremes": 100, "mid": 48, "invalid": 70, "hamming": 35, "rotation": 140, "half": 28, "edge": 48},
    "T36H11": {"bit_order": 36, "extremes": 144, "mid": 48, "invalid": 98, "hamming": 80, "rotation": 160, "half": 32, "edge": 48},
    "T36H11B1": {"bit_order": 36, "extremes": 144, "mid": 48, "invalid": 98, "hamming": 80, "rotation": 160, "half": 32, "edge": 48},
}
CHANGED = {
    "T16H5": {"contrast_le_50": 32, "invalid_le_10": 18, "hamming_le": 10, "invalid_ge_3": 40, "bit_ge_mid": 24, "mid_truncated": 57, "round_half_even": 19, "popcount_low32": 0, "bit_order_reversed": 239, "y_outer": 227, "rotate_other_way": 32, "corners_not_reversed": 161},
    "T25H7": {"contrast_le_50": 50, "invalid_le_10": 18, "hamming_le": 18, "invalid_ge_3": 42, "bit_ge_mid": 24, "mid_truncated": 59, "round_half_even": 25, "popcount_low32": 0, "bit_order_reversed": 383, "y_outer": 371, "rotate_other_way": 68, "corners_not_reversed": 241},
    "T36H11": {"contrast_le_50": 72, "invalid_le_10": 18, "hamming_le": 24, "invalid_ge_3": 56, "bit_ge_mid": 24, "mid_truncated": 70, "round_half_even": 28, "popcount_low32": 16, "bit_order_reversed": 502, "y_outer": 484, "rotate_other_way": 76, "corners_not_reversed": 306},
    "T36H11B1": {"contrast_le_50": 72, "invalid_le_10": 18, "hamming_le": 24, "invalid_ge_3": 56, "bit_ge_mid": 24, "mid_truncated": 70, "round_half_even": 28, "popcount_low32": 16, "bit_order_reversed": 502, "y_outer": 484, "rotate_other_way": 76, "corners_not_reversed": 306},
}


def oracle_positions(quad, fam):
    """orc_decode_positions' sample positions, float32 [nb, 2], in an image too large to refuse a finite corner below 2^32."""
    edge, border, _, _ = family(fam)
    q = np.ascontiguousarray(quad, np.float32).reshape(8)
    pts = np.zeros(2 * edge * edge, np.float32)
    if not orc().orc_decode_positions(0xFFFFFFFF, 0xFFFFFFFF, q.ctypes.data, border, edge, 0.5, pts.ctypes.data):
        return None
    return pts.reshape(-1, 2)


@functools.lru_cache(None)
def yard(fam):
    """The yardstick's (status, id, xy, bits) of every case of the family, and no case is knife-edge but the half-integer ones."""
    out = []
    for c in T.family_cases(fam):
        st, tid, xy, bits, knife = yardstick(c.plane, c.quad, fam)
        # (near a half-integer are only the coordinates put there on purpose: the half-integer cases' samples, computed exactly,
        # and the edge cases' moved corners, which are the caller's own floats)
        assert not knife or c.kind in ("half", "edge"), c.name
        out.append((st, tid, xy, bits))
    return out


def same_result(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_every_sample_lies_two_pixels_inside_the_cell_it_is_meant_for(fam):
    edge, border, _, _ = family(fam)
    nb = edge * edge
    n_checked = 0
    for c in T.family_cases(fam):
        if c.kind == "half" or np.abs(c.quad).max() > 1e6:
            continue
        pts = oracle_positions(c.quad, fam).astype(np.float64)
        boxes = T.cell_boxes(fam, *c.intent["origin"])
        inside = ((pts[:, None, 0] >= boxes[None, :, 0] + 2) & (pts[:, None, 0] <= boxes[None, :, 1] - 2) &
                  (pts[:, None, 1] >= boxes[None, :, 2] + 2) & (pts[:, None, 1] <= boxes[None, :, 3] - 2))  # [sample, cell]
        assert (inside.sum(axis=1) == 1).all(), c.name
        cell = inside.argmax(axis=1)
        assert sorted(cell) == list(range(nb)), c.name
        if np.array_equal(c.quad, T.std_quad(fam, *c.intent["origin"])):
            assert np.array_equal(cell, np.arange(nb)), c.name
        for n in range(nb):  # the cell is flat
            x0, x1, y0, y1 = boxes[cell[n]]
            assert len(np.unique(c.plane[y0:y1 + 1, x0:x1 + 1])) == 1, c.name
        n_checked += 1
    assert n_checked >= len(T.family_cases(fam)) * 3 // 4


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_half_integer_cases_are_exact_under_the_oracle(fam):
    """No family is left out: T.HALF_FAMILIES is all four (T16H5 must hold, all its divisors being powers of two; side 72 and 80
    hold as well, every affine coefficient being an integer or a half)."""
    assert fam in T.HALF_FAMILIES
    cs = [c for c in T.family_cases(fam) if c.kind == "half"]
    assert len(cs) >= 16
    parities = set()
    for c in cs:
        exact = T.exact_positions(c.quad, fam)
        got = oracle_positions(c.quad, fam)
        for n, (ex, ey) in enumerate(exact):
            assert ex.denominator == 2 and ey.denominator == 2, c.name
            assert float(got[n, 0]) == ex and float(got[n, 1]) == ey, (c.name, n)  # (Fraction == float compares exactly)
            jx, jy = int(ex - ex % 1), int(ey - ey % 1)
            parities.add((jx % 2, jy % 2))
            four = c.plane[jy:jy + 2, jx:jx + 2].astype(int)
            assert abs(four[1, 1] - four[0, 0]) == abs(four[1, 1] - four[0, 1]) == abs(four[1, 1] - four[1, 0]) == 255 > 50, c.name
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_cases_land_where_intended_under_the_oracle_alone(fam):
    edge, _, thres, codes = family(fam)
    seen = set()
    for c, y in zip(T.family_cases(fam), yard(fam)):
        st, tid, xy, bits = y
        it = c.intent
        assert same_result(y, c.expect), (c.name, y, c.expect)
        if "status" in it:
            assert st == it["status"], (c.name, st)
        if "not_status" in it:
            assert st != it["not_status"], (c.name, st)
        if "id" in it and it.get("status") == DECODED:
            assert tid == it["id"], (c.name, tid)
        if "bits" in it:
            assert st in (DECODED, NO_MATCH) and bits == it["bits"], (c.name, st, bits)  # (AGX_QUAD_NO_MATCH carries the bits)
        if st == DECODED:
            q = c.quad.reshape(4, 2)
            rot = [r for r in range(4) if np.array_equal(np.roll(q, -r, axis=0)[::-1].reshape(8), xy)]
            assert len(rot) == 1, c.name
            if "rot" in it:
                assert rot[0] == it["rot"], (c.name, rot)
            if "rot_not" in it:
                assert rot[0] != it["rot_not"], (c.name, rot)
            seen.add((c.kind, "rot%d" % rot[0]))
        seen.add((c.kind, st))
    # what the kinds are there for
    for r in (1, 2, 3):
        assert ("rotation", "rot%d" % r) in seen
    assert {("extremes", LOW_CONTRAST), ("invalid", AMBIGUOUS), ("invalid", DECODED), ("hamming", NO_MATCH), ("hamming", DECODED),
            ("mid", DECODED), ("half", DECODED), ("edge", OUTSIDE), ("edge", DECODED)} <= seen


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_inventory_and_slot_order(fam):
    edge, _, thres, codes = family(fam)
    nb = edge * edge
    cs = T.family_cases(fam)
    assert len(set(c.name for c in cs)) == len(cs)
    by_kind = {k: [s for s, c in enumerate(cs) if c.kind == k] for k in T.KINDS}
    print(fam, {k: len(v) for k, v in by_kind.items()}, len(cs))
    assert N_CASES[fam] == {k: len(v) for k, v in by_kind.items()}
    for k, slots in by_kind.items():  # every kind on all four quad rows of a wave and on both sides of a workgroup's 16-slot boundary
        assert set(s & 3 for s in slots) == {0, 1, 2, 3}, k
        assert {0, 15} <= set(s & 15 for s in slots), k
    names = [c.name for c in cs]
    for k in range(thres + 1):  # every flip kind at every k, for the listed codes
        kinds = ["k0"] if k == 0 else ["low", "top"] + (["high"] if nb > 32 else [])
        for kind in kinds:
            hits = [n for n in names if "/hamming/" in n and n.endswith("_k%d_%s" % (k, kind))]
            assert len(hits) >= len(T.code_indices(fam)) - 2, (k, kind, hits)
    n_codes = len(codes)
    assert {0, 15, 16, 17, n_codes - 1} <= set(T.code_indices(fam)) and (n_codes - 1) // 16 * 16 in T.code_indices(fam)
    signs = set(s for c in cs if c.kind == "invalid" for s in c.intent["signs"])
    assert signs == {0, 1}
    lanes = [c.name for c in cs if c.kind == "invalid" and "_lane" in c.name]
    assert len(lanes) == {16: 0, 25: 2 * 2, 36: 2 * 16}[nb]  # samples s, s + 8, s + 16, s + 24 exist for no s, for s = 0, for every s


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_model_equals_the_yardstick_and_every_mutation_is_caught(fam):
    edge, _, _, _ = family(fam)
    cs = T.family_cases(fam)
    pts = []
    for c in cs:
        if c.kind == "half":
            pts.append(T.positions_f64(c.quad, fam))  # (exact arithmetic; equal to the oracle's by the test above)
        else:
            p = oracle_positions(c.quad, fam)
            pts.append(None if p is None else p.astype(np.float64))
    run = lambda mut: [T.model(c.plane, c.quad, fam, p, mut) if p is not None else (OUTSIDE, 0, np.zeros(8, np.float32), 0) for c, p in zip(cs, pts)]
    base = run(None)
    for c, m, y in zip(cs, base, yard(fam)):
        assert same_result(m, y), (c.name, m, y)
    changed = {}
    for mut in T.MUTATIONS:
        changed[mut] = sum(not same_result(a, b) for a, b in zip(run(mut), base))
    print(fam, changed)
    for mut, n in changed.items():
        assert n >= 1 or (mut == "popcount_low32" and edge * edge <= 32), (mut, n)
    assert changed == CHANGED[fam]


@pytest.mark.parametrize("fam", ("T16H5", "T25H7", "T25H9", "T36H11"))
def test_two_accepted_candidates_never_compete(fam):
    thres = family(fam)[2]
    d = T.min_pair_distance(fam)
    print(fam, "smallest distance between two (code, rotation) pairs:", d)
    assert d >= 2 * thres - 1, (fam, d)


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_host_form_equals_the_yardstick_on_every_case_and_field(fam):
    import aprilgrid_rs_amd as A
    cs = T.family_cases(fam)
    for c, (st, tid, xy, bits) in zip(cs, yard(fam)):
        tags, gst, gbits = A.decode_quads_tail(fam, c.plane, c.quad[None], with_bits=True)
        assert gst[0] == st, (c.name, gst[0], st)
        assert int(gbits[0]) == bits, (c.name, int(gbits[0]), bits)
        ref = np.zeros(1, TAG_DTYPE)
        if st == DECODED:
            ref[0]["id"], ref[0]["xy"] = tid, xy
        assert tags.tobytes() == ref.tobytes(), (c.name, tags, ref)
        check_zero_records(tags, gst, gbits, c.name)


@pytest.mark.parametrize("fam", sorted(T.TAIL_SPEC))
def test_oracle_on_the_boards_with_flipped_bits(fam):
    """Per frame (as rendered, and turned by one, two and three quarter turns): the oracle's detect finds at least half of the tags
    with fewer than thres flipped bits and none with thres."""
    thres = family(fam)[2]
    frames, ks = T.tail_frames(fam)
    under = [p for p, k in enumerate(ks) if k < thres]
    assert len(frames) == 4 * len(T.TAIL_SPEC[fam][2]) and len(under) < len(ks)
    for f, found in enumerate(T.tail_oracle(fam)):
        assert all(0 <= t < len(ks) and ks[t] < thres for t in found), (fam, f, sorted(found))
        assert 2 * len(found) >= len(under), (fam, f, len(found), len(under))
