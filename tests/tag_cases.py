"""Hand-painted tags for the decode stage (decode_positions, bit_code, rotate_bits, best_tag: reference src/detector.rs:42-169,
called from try_decode_quad at :448-476): agx_decode_quads_tail, k_decode_quads and, through rendered boards, k_board_tail's copy.
Numpy only; what every case claims is asserted from the oracle and numpy in tests/test_tag_cases_cpu.py, and
tests/test_gpu_tag_limits.py runs the cases through the kernel.

A painted case is one W x H u8 plane with one axis-aligned tag of 8 x 8 px cells, every pixel set by hand, and one quad.  The
standard quad is TL, TR, BR, BL of the tag's cell grid (side_bits * 8 px: 64 / 72 / 80 / 64 px for T16H5 / T25H7 / T36H11 /
T36H11B1).  tag_affine (src/image_util.rs:39-70) maps the source square (-0.5, -0.5) .. (side_bits - 0.5, side_bits - 0.5) onto
the quad, source y along corner 0 -> corner 1, so sample n (x outer, y inner, :60-63) lies in the middle of the cell of row
border + n / edge and column border + n % edge: 4 px from the cell's first pixel.

`model` restates the four reference functions in plain numpy with switchable mutations; a case's `expect` is the unmutated
model on the exact (rational) sample positions, its `intent` what the construction itself claims, by the reference's lines."""
import collections
import fractions
import functools

import numpy as np

DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS, NO_MATCH = 0, 1, 2, 3, 4  # AGX_QUAD_*
W, H = 100, 91   # (W even, H odd: W - 0.5 and H - 0.5 round alike half away, differently half to even)
CELL = 8
FAMILIES = ("T16H5", "T25H7", "T36H11", "T36H11B1")
F32 = np.float32

Case = collections.namedtuple("Case", "name kind family plane quad intent expect")  # expect: (status, id, xy [8] f32, bits)

MUTATIONS = ("contrast_le_50",   # max - min <= 50 for < 50 (:97)
             "invalid_le_10",    # |mid - b| <= 10 for < 10 (:105)
             "hamming_le",       # best_score <= thres for < thres (:160)
             "invalid_ge_3",     # invalid_count >= 3 for > 3 (:117)
             "bit_ge_mid",       # b >= mid for b > mid (:110)
             "mid_truncated",    # (min + max) / 2 truncated, not rounded half away (:100)
             "round_half_even",  # coordinates rounded half to even, not half away (:51-52, :83)
             "popcount_low32",   # count_ones of the low word only (:147)
             "bit_order_reversed",  # sample n sets bit n, not bit nb - 1 - n (:101 .rev())
             "y_outer",          # the sample loop y outer, x inner (:60-63)
             "rotate_other_way",  # rotate_bits a quarter turn the other way (:124-140)
             "corners_not_reversed")  # rotate_left(rotation) without reverse() (:468-469)


@functools.lru_cache(None)
def family(name):
    """-> (edge, border, thres, codes uint64 [n]) from oracle.FAMILIES and the committed code tables."""
    from oracle import oracle as O
    edge, border, hamming, _ = O.FAMILIES[name]
    return edge, border, hamming, np.ascontiguousarray(O.family_codes(name), np.uint64)


def side_px(fam):
    edge, border, _, _ = family(fam)
    return (edge + 2 * border) * CELL


# ---- the reference's four functions, in plain numpy, with mutations ----------------------------------------------------------
def round_u32(v, mut=None):
    """`f32::round() as u32` (:51-52, :83): half away from zero, negative -> 0, saturating."""
    v = np.asarray(v, np.float64)
    r = np.rint(v) if mut == "round_half_even" else np.sign(v) * np.floor(np.abs(v) + 0.5)
    return np.clip(r, 0.0, 4294967295.0)


def rotate_bits(bits, edge, mut=None):
    """rotate_bits (:124-140): output bit `count` is input bit r + c * edge, r from edge - 1 down, c up."""
    out, count = 0, 0
    if mut == "rotate_other_way":
        for r in range(edge):
            for c in range(edge - 1, -1, -1):
                out |= ((bits >> (r + c * edge)) & 1) << count
                count += 1
        return out
    for r in range(edge - 1, -1, -1):
        for c in range(edge):
            out |= ((bits >> (r + c * edge)) & 1) << count
            count += 1
    return out


def popcounts(x, mut=None):
    x = np.asarray(x, np.uint64)
    if mut == "popcount_low32":
        x = x & np.uint64(0xFFFFFFFF)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def best_tag(bits, fam, mut=None):
    """best_tag (:142-169): per rotation the FIRST code of the smallest distance; the first rotation whose best is under thres."""
    edge, _, thres, codes = family(fam)
    for rotated in range(4):
        d = popcounts(codes ^ np.uint64(bits), mut)
        i = int(d.argmin())  # (the first of equal minima, as reduce with `<` keeps)
        if (d[i] <= thres) if mut == "hamming_le" else (d[i] < thres):
            return i, rotated
        bits = rotate_bits(bits, edge, mut)
    return None


def model(plane, quad, fam, pts, mut=None):
    """try_decode_quad (:448-476) of one quad -> (status, id, xy [8] float32, bits).  pts: [nb, 2] sample positions in the
    reference's order (x outer, y inner), float64 -- decode_positions' values are the caller's: the oracle's, or exact ones."""
    edge, border, thres, codes = family(fam)
    nb = edge * edge
    h, w = plane.shape
    q = np.asarray(quad, F32).reshape(4, 2)
    zero = np.zeros(8, F32)
    cx, cy = round_u32(q[:, 0], mut), round_u32(q[:, 1], mut)
    if ((cx >= w) | (cy >= h)).any():  # :50-56
        return OUTSIDE, 0, zero, 0
    pts = np.asarray(pts, np.float64).reshape(nb, 2)
    if mut == "y_outer":
        pts = pts.reshape(edge, edge, 2).transpose(1, 0, 2).reshape(nb, 2)
    ix, iy = round_u32(pts[:, 0], mut), round_u32(pts[:, 1], mut)
    if ((ix >= w) | (iy >= h)).any():  # :84-93
        return OUTSIDE, 0, zero, 0
    v = plane[iy.astype(np.int64), ix.astype(np.int64)].astype(np.int64)
    lo, hi = int(v.min()), int(v.max())
    if (hi - lo <= 50) if mut == "contrast_le_50" else (hi - lo < 50):  # :97
        return LOW_CONTRAST, 0, zero, 0
    mid = (lo + hi) // 2 if mut == "mid_truncated" else (lo + hi + 1) // 2  # :100 (lo + hi >= 0: half away is half up)
    d = np.abs(mid - v)
    invalid = int(((d <= 10) if mut == "invalid_le_10" else (d < 10)).sum())  # :105
    one = (v >= mid) if mut == "bit_ge_mid" else (v > mid)  # :110
    bits = 0
    for n in range(nb):
        if one[n]:
            bits |= 1 << (n if mut == "bit_order_reversed" else nb - 1 - n)  # :101: the first sample is the top bit
    if (invalid >= 3) if mut == "invalid_ge_3" else (invalid > 3):  # :117
        return AMBIGUOUS, 0, zero, 0
    hit = best_tag(bits, fam, mut)
    if hit is None:
        return NO_MATCH, 0, zero, bits
    idx, rot = hit
    c = np.roll(q, -rot, axis=0)  # rotate_left(rotation) :468
    if mut != "corners_not_reversed":
        c = c[::-1]  # reverse() :469
    return DECODED, idx, np.ascontiguousarray(c, F32).reshape(8), bits


def exact_positions(quad, fam):
    """decode_positions' values in exact arithmetic -> [nb][2] Fractions.  The least-squares affine map of the four source
    corners (-m, -m), (-m, S), (S, S), (S, -m), m = 1/2, S = side_bits - 1/2, onto the quad: the source is a square, so the normal
    equations diagonalise about its centre c = (S - m) / 2 with half side a = (S + m) / 2."""
    edge, border, _, _ = family(fam)
    Fr = fractions.Fraction
    side = edge + 2 * border
    a, c = Fr(side, 2), Fr(side - 1, 2)
    su, sv = (-a, -a, a, a), (-a, a, a, -a)
    q = [Fr(float(v)) for v in np.asarray(quad, F32).reshape(8)]
    h = []
    for axis in range(2):
        t = [q[2 * p + axis] for p in range(4)]
        hu = sum(s * x for s, x in zip(su, t)) / (4 * a * a)
        hv = sum(s * x for s, x in zip(sv, t)) / (4 * a * a)
        h.append((hu, hv, sum(t) / 4 - hu * c - hv * c))
    return [[h[axis][0] * x + h[axis][1] * y + h[axis][2] for axis in range(2)]
            for x in range(border, border + edge) for y in range(border, border + edge)]


def positions_f64(quad, fam):
    return np.array([[float(v) for v in p] for p in exact_positions(quad, fam)], np.float64)


# ---- painting ------------------------------------------------------------------------------------------------------------------
def std_quad(fam, x0, y0):
    s = side_px(fam)
    return np.array([x0, y0, x0 + s, y0, x0 + s, y0 + s, x0, y0 + s], F32)


def paint(fam, vals, x0=10, y0=5, frame=0, ground=128):
    """One tag at the integer pixel (x0, y0): vals[n] fills the 8 x 8 px cell of sample n, the border cells get `frame`."""
    edge, border, _, _ = family(fam)
    plane = np.full((H, W), ground, np.uint8)
    s = side_px(fam)
    assert 0 <= x0 and x0 + s <= W and 0 <= y0 and y0 + s <= H
    plane[y0:y0 + s, x0:x0 + s] = frame
    vals = np.asarray(vals).reshape(edge, edge)
    for r in range(edge):
        for c in range(edge):
            yy, xx = y0 + (border + r) * CELL, x0 + (border + c) * CELL
            plane[yy:yy + CELL, xx:xx + CELL] = vals[r, c]
    return plane


def cell_boxes(fam, x0, y0):
    """[nb, 4]: first and last pixel column, first and last pixel row of the cell of sample n."""
    edge, border, _, _ = family(fam)
    n = np.arange(edge * edge)
    xx, yy = x0 + (border + n % edge) * CELL, y0 + (border + n // edge) * CELL
    return np.stack([xx, xx + CELL - 1, yy, yy + CELL - 1], axis=1)


def code_vals(code, nb, lo=0, hi=255):
    """The cell values that read as `code`: sample n carries bit nb - 1 - n."""
    return np.array([hi if (code >> (nb - 1 - n)) & 1 else lo for n in range(nb)], np.int64)


def code_indices(fam):
    """0, 15, 16, 17, the family's last, the last multiple of 16 and its neighbours: every lane of the 16-lane scan's last
    partial round, and the round before it."""
    n = len(family(fam)[3])
    m = (n - 1) // 16 * 16
    return sorted(set(i for i in (0, 15, 16, 17, n - 1, m - 1, m, m + 1) if 0 <= i < n))


def distances_to_all(bits, fam):
    """[4, n_codes]: the distance of `bits` after 0 .. 3 calls of rotate_bits to every code."""
    edge, _, _, codes = family(fam)
    out = []
    for _ in range(4):
        out.append(popcounts(codes ^ np.uint64(bits)))
        bits = rotate_bits(bits, edge)
    return np.array(out)


def flip_sets(fam, i, k):
    """Up to three sets of k bit positions to flip in code i -- in the low word only, in bits >= 32 only (edge 6), including the
    top bit -- each the first of its kind after which no other (code, rotation) is within thres of the flipped word."""
    edge, _, thres, codes = family(fam)
    nb = edge * edge
    if k == 0:
        return [("k0", ())]
    kinds = [("low", [b for b in range(min(nb, 32))])]
    if nb > 32:
        kinds.append(("high", list(range(32, nb))))
    kinds.append(("top", None))
    out = []
    for kind, pool in kinds:
        found = None
        for start in range(nb):
            if kind == "top":
                pos = (nb - 1,) + tuple((start + 5 * j) % (nb - 1) for j in range(k - 1))
            else:
                pos = tuple(pool[(start + 3 * j + i) % len(pool)] for j in range(k))
            if len(set(pos)) != k:
                continue
            word = int(codes[i])
            for b in pos:
                word ^= 1 << b
            d = distances_to_all(word, fam)
            d[0, i] = 99
            if d.min() > thres:
                found = pos
                break
        if found is not None:  # (tests/test_tag_cases_cpu.py asserts that every family has every kind at every k)
            out.append((kind, found))
    return out


def flipped(code, pos):
    for b in pos:
        code ^= 1 << b
    return code


def _mk(cases, name, kind, fam, plane, quad, intent=None, origin=(10, 5)):
    """intent["origin"]: the pixel of the painted cell grid's first corner."""
    quad = np.asarray(quad, F32).reshape(8)
    intent = dict(intent or {}, origin=origin)
    if np.abs(quad).max() < 1e6:
        expect = model(plane, quad, fam, positions_f64(quad, fam))
    else:
        expect = (OUTSIDE, 0, np.zeros(8, F32), 0)
    cases.append(Case("%s/%s/%s" % (fam, kind, name), kind, fam, plane, quad, intent or {}, expect))


def quad_orderings(q):
    """The quad, its three other cyclic orders, and the four with reversed winding -> [(name, quad [8])]"""
    c = np.asarray(q, F32).reshape(4, 2)
    return [("%s%d" % (wn, r), np.roll(w, -r, axis=0).reshape(8)) for wn, w in (("cyc", c), ("rev", c[::-1])) for r in range(4)]


def build_family(fam):
    edge, border, thres, codes = family(fam)
    nb = edge * edge
    cases = []
    x0, y0 = 10, 5
    q = std_quad(fam, x0, y0)
    # 1. bit order: one cell at 255, the others at 0 -> bit nb - 1 - n (:101, x outer / y inner :60-63)
    for n in range(nb):
        vals = np.zeros(nb, np.int64)
        vals[n] = 255
        _mk(cases, "n%d" % n, "bit_order", fam, paint(fam, vals, x0, y0, frame=77), q, {"bits": 1 << (nb - 1 - n), "carries_bits": True})
    # 2. where the extremes sit: all cells at 100, one at 100 +- d (:94-99: 49 is under the contrast limit, 50 is not)
    for n in range(nb):
        for d in (49, 50):
            for sign in (-1, 1):
                vals = np.full(nb, 100, np.int64)
                vals[n] = 100 + sign * d
                intent = {"status": LOW_CONTRAST} if d == 49 else {"not_status": LOW_CONTRAST}
                _mk(cases, "n%d_%+d" % (n, sign * d), "extremes", fam, paint(fam, vals, x0, y0, frame=100, ground=100), q, intent)
    idxs = code_indices(fam)
    # 3. mid rounding and the strict `>` (:100, :110): lo + hi odd; cells at mid and mid - 1 where the code has 0, mid + 1 where 1
    for lo, hi in ((0, 51), (100, 255)):
        mid = (lo + hi + 1) // 2
        for i in idxs[:4]:
            code = int(codes[i])
            zeros = [n for n in range(nb) if not (code >> (nb - 1 - n)) & 1]
            ones = [n for n in range(nb) if (code >> (nb - 1 - n)) & 1]
            assert len(zeros) >= 4 and len(ones) >= 3
            for name, cells in (("mid", [(zeros[0], mid)]), ("mid_last", [(zeros[-1], mid)]), ("above", [(ones[0], mid + 1)]),
                                ("above_last", [(ones[-1], mid + 1)]), ("below", [(zeros[1], mid - 1)]),
                                ("all3", [(zeros[-2], mid), (ones[1], mid + 1), (zeros[2], mid - 1)])):
                vals = code_vals(code, nb, lo, hi)
                for n, v in cells:
                    vals[n] = v
                _mk(cases, "%d_%d_code%d_%s" % (lo, hi, i, name), "mid", fam, paint(fam, vals, x0, y0, frame=lo), q,
                    {"status": DECODED, "id": i, "bits": code})
    # 4. invalid count (:104-109, :117): lo 0, hi 255, mid 128; |mid - b| = 9 is invalid and 10 is valid; 3 invalid cells decode
    # and 4 do not.  A cell keeps its code bit: mid + 9 / + 10 where the code has 1, mid - 9 / - 10 where it has 0.
    kmax = nb // 8
    for i in idxs[:2]:
        code = int(codes[i])
        bit = lambda n, code=code: (code >> (nb - 1 - n)) & 1
        near = lambda n, d, bit=bit: 128 + d if bit(n) else 128 - d

        def inv_case(name, at9, all10, intent, code=code, i=i, bit=bit, near=near):
            # (one cell stays at 255 and one at 0, away from the cells at +- 9: min, max and mid are 0, 255 and 128 in every case)
            keep = {max(n for n in range(nb) if bit(n) and n not in at9), max(n for n in range(nb) if not bit(n) and n not in at9)}
            vals = code_vals(code, nb)
            if all10:
                for n in range(nb):
                    if n not in keep:
                        vals[n] = near(n, 10)
            for n in at9:
                vals[n] = near(n, 9)
            _mk(cases, "code%d_%s" % (i, name), "invalid", fam, paint(fam, vals, x0, y0), q, dict(intent, signs=sorted(set(bit(n) for n in at9))))

        ok = {"status": DECODED, "id": i, "bits": code}
        inv_case("all10", [], True, ok)
        for o in range(8):
            # four cells in four different sub lanes (n & 7), from lane o on, in as many rounds (n >> 3) as the family has whole ones
            four = [(o + j) % 8 + 8 * (j % kmax) for j in range(4)]
            assert len(set(n % 8 for n in four)) == 4 and max(four) < nb
            inv_case("subs%d_3" % o, four[:3], False, ok)
            inv_case("subs%d_4" % o, four, False, {"status": AMBIGUOUS})
            inv_case("subs%d_3_all10" % o, four[1:], True, ok)
            inv_case("subs%d_4_all10" % o, four, True, {"status": AMBIGUOUS})
        for s in range(8):  # the four in ONE sub lane: samples s, s + 8, s + 16, s + 24
            same = [s, s + 8, s + 16, s + 24]
            if same[-1] < nb:
                inv_case("lane%d_4" % s, same, False, {"status": AMBIGUOUS})
                inv_case("lane%d_3" % s, same[1:], False, ok)
    # 5. Hamming limit (:160: score < thres): code i with k = 0 .. thres flipped bits
    rot_src = []
    for i in idxs:
        for k in range(thres + 1):
            for kind, pos in flip_sets(fam, i, k):
                word = flipped(int(codes[i]), pos)
                intent = {"status": DECODED, "id": i, "rot": 0, "bits": word} if k < thres else {"status": NO_MATCH, "bits": word, "carries_bits": True}
                _mk(cases, "code%d_k%d_%s" % (i, k, kind), "hamming", fam, paint(fam, code_vals(word, nb), x0, y0), q, intent)
                if (k == 0 or k == thres - 1) and kind in ("k0", "low"):
                    rot_src.append((i, k, word))
    # 6. rotations: the cell pattern turned by quarter turns under the same quad; the pattern as it is under the quad's eight orders
    for i, k, word in sorted(set(rot_src)):
        grid = code_vals(word, nb).reshape(edge, edge)
        for t in (1, 2, 3):
            _mk(cases, "code%d_k%d_turn%d" % (i, k, t), "rotation", fam, paint(fam, np.rot90(grid, t), x0, y0), q,
                {"status": DECODED, "id": i, "rot_not": 0})
        plane = paint(fam, grid, x0, y0)
        for name, qq in quad_orderings(q)[1:]:
            intent = {"status": DECODED, "id": i, "rot_not": 0} if name.startswith("cyc") else {}
            _mk(cases, "code%d_k%d_%s" % (i, k, name), "rotation", fam, plane, qq, intent)
    # 8. exact half-integer samples: the quad at (integer + 0.5, integer + 0.5); every sample coordinate is j + 0.5 and reads
    # pixel j + 1 (:83, half away).  The cell is painted as usual one pixel further, and of the four pixels (j, j + 1) x (j, j + 1)
    # around a sample the three that another rounding reads carry the cell's inverse.
    if fam in HALF_FAMILIES:
        for i in idxs:
            code = int(codes[i])
            for ex, ey in ((10, 6), (11, 5), (10, 5), (11, 6)):
                plane = paint(fam, code_vals(code, nb), ex + 1, ey + 1)
                boxes = cell_boxes(fam, ex + 1, ey + 1)
                for n in range(nb):
                    jx, jy = boxes[n, 0] + 3, boxes[n, 2] + 3  # the sample is at (jx + 0.5, jy + 0.5)
                    v = int(plane[jy + 1, jx + 1])
                    plane[jy:jy + 2, jx:jx + 2] = 255 - v
                    plane[jy + 1, jx + 1] = v
                _mk(cases, "code%d_x%d_y%d" % (i, ex, ey), "half", fam, plane, std_quad(fam, ex + 0.5, ey + 0.5),
                    {"status": DECODED, "id": i, "rot": 0, "bits": code}, origin=(ex + 1, ey + 1))
    # 9. corners at the image edge (:50-56).  The tag in the plane's far corner, its outer corner at (W - 1, H - 1): the quad's
    # corner there moved to W - 0.5 (rounds to W: outside) and to the float32 below (inside); the tag in the near corner, the
    # corner at (0, 0) moved to -0.5 and -0.49 (inside: a negative value saturates to 0); 1e10 and 2^32 (outside).  The quad's
    # order is cycled so that each corner index takes its turn at the moved corner.
    i = idxs[1]
    code = int(codes[i])
    s = side_px(fam)
    far = paint(fam, code_vals(code, nb), W - 1 - s, H - 1 - s)
    nearp = paint(fam, code_vals(code, nb), 0, 0)
    for c in range(4):
        qf = np.roll(std_quad(fam, W - 1 - s, H - 1 - s).reshape(4, 2), c - 2, axis=0)   # geometric BR at index c
        qn = np.roll(std_quad(fam, 0, 0).reshape(4, 2), c, axis=0)                        # geometric TL at index c
        assert tuple(qf[c]) == (W - 1, H - 1) and tuple(qn[c]) == (0, 0)
        for axis, size in ((0, W), (1, H)):
            ok = {"status": DECODED, "id": i}  # (in the cycled orders the bits read are the code's turned)
            for name, base, plane, v, intent in (
                    ("at_size", qf, far, F32(size - 0.5), {"status": OUTSIDE}),
                    ("below_size", qf, far, np.nextafter(F32(size - 0.5), F32(0)), ok),
                    ("minus_half", qn, nearp, F32(-0.5), ok),
                    ("minus_049", qn, nearp, F32(-0.49), ok),
                    ("1e10", qf, far, F32(1e10), {"status": OUTSIDE}),
                    ("2p32", qn, nearp, F32(4294967296.0), {"status": OUTSIDE})):
                qq = base.copy()
                qq[c, axis] = v
                _mk(cases, "corner%d_%s_%s" % (c, "xy"[axis], name), "edge", fam, plane, qq.reshape(8), intent,
                    origin=(W - 1 - s, H - 1 - s) if plane is far else (0, 0))
    return cases


HALF_FAMILIES = FAMILIES  # (tests/test_tag_cases_cpu.py asserts, per family, that the oracle's float positions are the exact ones)
KINDS = ("bit_order", "extremes", "mid", "invalid", "hamming", "rotation", "half", "edge")


@functools.lru_cache(None)
def family_cases(fam):
    """The family's cases in the order the GPU test sends them (one frame, one quad, one slot each; slot = position): the first
    seeded shuffle in which every kind's cases fall on all four quad rows of a wave (slot & 3) and on both sides of a workgroup's
    16-slot boundary (slot & 15 = 15 and 0) -- asserted again in tests/test_tag_cases_cpu.py."""
    cases = build_family(fam)
    kinds = np.array([KINDS.index(c.kind) for c in cases])
    for seed in range(1000):
        order = np.random.default_rng(seed).permutation(len(cases))
        slots = np.arange(len(cases))
        if all(set(slots[kinds[order] == k] & 3) == {0, 1, 2, 3} and {0, 15} <= set(slots[kinds[order] == k] & 15) for k in range(len(KINDS))):
            return tuple(cases[j] for j in order)
    raise AssertionError("no shuffle spreads the kinds of " + fam)


def min_pair_distance(fam):
    """The smallest distance between two distinct (code, rotation) pairs of the family, over all four rotations."""
    edge, _, _, codes = family(fam)
    words = []
    for c in codes:
        b = int(c)
        for _ in range(4):
            words.append(b)
            b = rotate_bits(b, edge)
    words = np.array(words, np.uint64)
    best = 64
    for j in range(len(words) - 1):
        best = min(best, int(popcounts(words[j + 1:] ^ words[j]).min()))
    return best


# ---- rendered boards for the device tail's copy of the decode (k_board_tail) ------------------------------------------------------
TAIL_SIZE = (800, 600)
TAIL_SPEC = {"T36H11": (6, 6, (3, 4)), "T25H7": (5, 5, (21, 22))}  # rows, cols, frame seeds


def tail_codes(fam, n_tags):
    """The family's code list with p % (thres + 1) bits flipped in code p -> (list of ints, flipped-bit counts)."""
    edge, _, thres, codes = family(fam)
    nb = edge * edge
    out, ks = [int(c) for c in codes], []
    for p in range(n_tags):
        k = p % (thres + 1)
        for j in range(k):
            out[p] ^= 1 << ((3 * p + j * (nb // 3 + 1)) % nb)
        ks.append(k)
    return out, ks


@functools.lru_cache(None)
def tail_frames(fam):
    """-> (list of u8 frames: every seed's frame as rendered and turned by np.rot90 once, twice and three times; flipped-bit
    count of every tag id)"""
    import aprilgrid_rs_amd  # noqa: F401
    from aprilgrid_rs_amd import synth
    rows, cols, seeds = TAIL_SPEC[fam]
    codes, ks = tail_codes(fam, rows * cols)
    frames = []
    for seed in seeds:
        img = synth.render_frame(seed, TAIL_SIZE[0], TAIL_SIZE[1], spec=synth.BoardSpec(rows=rows, cols=cols), codes=codes, family=fam)[0].numpy()
        frames += [np.ascontiguousarray(np.rot90(img, t)) for t in range(4)]
    return frames, ks


@functools.lru_cache(None)
def tail_oracle(fam):
    from oracle import oracle as O
    return [O.detect(f, family=fam) for f in tail_frames(fam)[0]]
