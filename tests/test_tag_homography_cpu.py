"""The homography sampling model on the host: agx_tag_maps_tail, agx_decode_positions_tail_m (reference src/image_util.rs:5-37,
:39-70, src/detector.rs:42-72) against the numpy yardstick of tests/homography_oracle.py, the exact cases, the refusals, and the
hand-painted perspective tags that the affine model cannot decode.  No device is used."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import homography_oracle as HO
from tests import tag_cases as T

DECODED, OUTSIDE, NO_MATCH, DEGENERATE = 0, 1, 4, 6
AGX_OK, AGX_ERR_ARG = 0, -1
W, H = T.TAIL_SIZE
POISON = np.float32(-12345.5)
BOUND_PX = 1e-3  # the project's stated tolerance for sample points (README, decode-stages row)


def yardstick_quads():
    """Convex quads inside the 800 x 600 frame: tag sides 16 .. 300 px, near / far edge ratios 1.0 .. 0.4, turned and leaning"""
    rng = np.random.default_rng(2024)
    quads = []
    for side in (16, 23, 57, 120, 300):
        for ratio in (1.0, 0.9, 0.75, 0.6, 0.4):
            for _ in range(3):
                reach = 0.75 * side + 1  # (no corner is further from the centre: half the diagonal plus the lean)
                q = HO.trapezoid(rng.uniform(reach, W - 1 - reach), rng.uniform(reach, H - 1 - reach), side, ratio, turn=rng.uniform(0, 2 * np.pi),
                                 lean=rng.uniform(-0.2, 0.2))
                quads.append(q)
    quads = np.array(quads, np.float32)
    assert quads.min() >= 0 and quads[..., 0].max() <= W - 1 and quads[..., 1].max() <= H - 1
    return quads


@functools.lru_cache(None)
def measured():
    """-> the largest distance, in px per coordinate, between the library's sample points (through agx_tag_maps_tail's matrix, and
    as agx_decode_positions_tail_m stores them) and the yardstick's, over every family's side_bits and the margins 0, 0.5, 1"""
    import aprilgrid_rs_amd as A
    quads = yardstick_quads()
    worst_map = worst_pts = 0.0
    for fam in T.FAMILIES:
        edge, border, _, _ = T.family(fam)
        for margin in (0.0, 0.5, 1.0):
            maps, st = A.tag_maps(quads, 2 * border + edge, margin, "homography")
            pts, st2 = A.decode_positions(quads, W, H, border, edge, margin, model="homography")
            assert (st == DECODED).all() and (st2 == DECODED).all(), (fam, margin)
            for q, m, p in zip(quads, maps, pts):
                want = HO.positions(q, border, edge, margin)
                worst_map = max(worst_map, np.abs(HO.apply(m, HO.grid(border, edge)) - want).max())
                worst_pts = max(worst_pts, np.abs(p.astype(np.float64) - want).max())
    return worst_map, worst_pts


def test_maps_and_points_against_the_svd_yardstick():
    """Measured: 1.0e-4 px through the matrix, 1.8e-4 px of the stored points (DESIGN.md section 2 records it); the bound is the project's 1e-3 px, 16 binary32 ulps at
    coordinates below 1024 for an arithmetic of about ten roundings."""
    worst_map, worst_pts = measured()
    print("largest deviation: %.3g px through the matrix in float64, %.3g px of the stored points" % (worst_map, worst_pts))
    assert worst_map <= BOUND_PX and worst_pts <= BOUND_PX


def test_an_integer_parallelogram_has_the_affine_shape():
    import aprilgrid_rs_amd as A
    q = np.array([[100, 100], [180, 120], [200, 220], [120, 200]], np.float32)
    for fam in T.FAMILIES:
        edge, border, _, _ = T.family(fam)
        m, st = A.tag_maps(q[None], 2 * border + edge, 0.5, "homography")
        assert st[0] == DECODED and m[0, 2].tobytes() == np.array([0, 0, 1], np.float32).tobytes()
        a, st = A.tag_maps(q[None], 2 * border + edge, 0.5, "affine")
        assert st[0] == DECODED and a[0, 2].tobytes() == np.array([0, 0, 1], np.float32).tobytes()
        ph, sh = A.decode_positions(q[None], W, H, border, edge, 0.5, model="homography")
        pa, sa = A.decode_positions(q[None], W, H, border, edge, 0.5, model="affine")
        assert sh[0] == DECODED and sa[0] == DECODED and np.abs(ph.astype(np.float64) - pa).max() <= BOUND_PX
        # and the affine matrix gives decode_positions' points: its rows are tag_affine's
        assert np.abs(HO.apply(a[0], HO.grid(border, edge)) - pa[0]).max() <= BOUND_PX


def test_orderings_of_the_quad_permute_the_points():
    """The four cyclic orders and the mirrored quad: the same map of the plane up to the source square's symmetry, so the same
    set of sample points"""
    import aprilgrid_rs_amd as A
    quad = HO.trapezoid(400, 300, 200, 0.6, turn=0.4, lean=0.1)
    edge, border = 6, 2
    side = 2 * border + edge
    base, st = A.decode_positions(quad[None], W, H, border, edge, 0.5, model="homography")
    assert st[0] == DECODED
    g = HO.grid(border, edge)
    for name, qq in T.quad_orderings(quad.reshape(8)):
        p, st = A.decode_positions(qq[None], W, H, border, edge, 0.5, model="homography")
        assert st[0] == DECODED, name
        # where the reordered quad's source grid lies in the first quad's source square
        src = HO.apply(np.linalg.inv(HO.tag_homography(quad, side, 0.5)), HO.positions(qq, border, edge, 0.5))
        perm = [int(np.argmin(np.abs(g - s).sum(axis=1))) for s in src]
        assert sorted(perm) == list(range(edge * edge)), name
        assert np.abs(p[0].astype(np.float64) - base[0][perm]).max() <= 2 * BOUND_PX, name


REFUSED = {"three collinear corners": [[100, 100], [150, 100], [200, 100], [150, 180]],
           "the fourth corner on a diagonal": [[100, 100], [200, 100], [200, 200], [150, 150]],
           "a repeated corner": [[100, 100], [100, 100], [200, 200], [100, 200]],
           "all corners one point": [[100, 100]] * 4,
           "a bow-tie": [[100, 100], [200, 200], [200, 100], [100, 200]],
           "a concave quad": [[100, 100], [200, 100], [130, 130], [100, 200]]}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_quads_without_a_map_are_degenerate_and_write_nothing(name):
    from aprilgrid_rs_amd import _ffi
    q = np.array(REFUSED[name], np.float32)
    for r in range(4):
        qq = np.ascontiguousarray(np.roll(q, -r, axis=0))
        maps, st = np.full(9, POISON, np.float32), np.full(1, 99, np.uint32)
        assert _ffi.lib().agx_tag_maps_tail(qq.ctypes.data, 1, 10, 0.5, 1, maps.ctypes.data, st.ctypes.data) == AGX_OK
        assert st[0] == DEGENERATE and (maps == POISON).all(), (name, r)
        pts, st = np.full(72, POISON, np.float32), np.full(1, 99, np.uint32)
        assert _ffi.lib().agx_decode_positions_tail_m(qq.ctypes.data, 1, W, H, 2, 6, 0.5, pts.ctypes.data, st.ctypes.data, 1) == AGX_OK
        assert st[0] == DEGENERATE and (pts == POISON).all(), (name, r)
        # the affine model never says so
        assert _ffi.lib().agx_tag_maps_tail(qq.ctypes.data, 1, 10, 0.5, 0, maps.ctypes.data, st.ctypes.data) == AGX_OK and st[0] == DECODED
        assert _ffi.lib().agx_decode_positions_tail_m(qq.ctypes.data, 1, W, H, 2, 6, 0.5, pts.ctypes.data, st.ctypes.data, 0) == AGX_OK and st[0] == DECODED


def test_corners_that_are_not_finite_or_outside_the_image():
    import aprilgrid_rs_amd as A
    good = HO.trapezoid(400, 300, 100, 0.7).reshape(8)
    quads = np.stack([good] * 5)
    quads[1, 3], quads[2, 0], quads[3, 6] = np.nan, np.inf, -np.inf
    quads[4] = good + np.float32(600)  # finite, beyond the image: outside for decode_positions, a map all the same
    for model in ("affine", "homography"):
        maps, st = A.tag_maps(quads, 10, 0.5, model)
        assert list(st) == [DECODED, OUTSIDE, OUTSIDE, OUTSIDE, DECODED] and not maps[1:4].any() and maps[4].any(), model
        pts, st = A.decode_positions(quads, W, H, 2, 6, 0.5, model=model)
        assert list(st) == [DECODED, OUTSIDE, OUTSIDE, OUTSIDE, OUTSIDE] and not pts[1:].any(), model


def test_a_sample_behind_the_horizon_is_outside():
    """w is positive on the whole source square of an accepted quad, and at margin >= 0 every sample lies inside the square.  A
    margin below zero makes the square smaller than the sampled grid: under a strong perspective (far edge 0.05 of the near one:
    the horizon lies 0.05 of a side beyond the far edge) samples three cells beyond the square have w <= 0, and the slot is
    AGX_QUAD_OUTSIDE with no point written."""
    import aprilgrid_rs_amd as A
    quad = HO.trapezoid(400, 300, 60, 0.05)  # the horizon lies just beyond the far edge
    edge, border, margin = 8, 0, -3.0        # the square is (3, 3) .. (4, 4): the samples 0 .. 7 reach far beyond it
    maps, st = A.tag_maps(quad[None], 8, margin, "homography")
    assert st[0] == DECODED
    w = HO.grid(border, edge) @ maps[0, 2, :2].astype(np.float64) + maps[0, 2, 2]
    assert (w <= 0).any() and (w > 0).any(), "the case is not what it is meant to be"
    pts = np.full((1, 64, 2), POISON, np.float32)
    st = np.zeros(1, np.uint32)
    from aprilgrid_rs_amd import _ffi
    q = np.ascontiguousarray(quad)
    assert _ffi.lib().agx_decode_positions_tail_m(q.ctypes.data, 1, W, H, border, edge, C.c_float(margin), pts.ctypes.data, st.ctypes.data, 1) == AGX_OK
    assert st[0] == OUTSIDE and (pts == POISON).all()


def test_refused_arguments():
    from aprilgrid_rs_amd import _ffi
    lib = _ffi.lib()
    q = np.ascontiguousarray(HO.trapezoid(400, 300, 100, 0.7))
    maps, pts, st = np.zeros(9, np.float32), np.zeros(128, np.float32), np.zeros(1, np.uint32)
    P = lambda a: a.ctypes.data
    assert lib.agx_tag_maps_tail(P(q), 1, 10, 0.5, 1, P(maps), P(st)) == AGX_OK
    assert lib.agx_decode_positions_tail_m(P(q), 1, W, H, 2, 6, 0.5, P(pts), P(st), 1) == AGX_OK
    for model in (2, -1):
        assert lib.agx_tag_maps_tail(P(q), 1, 10, 0.5, model, P(maps), P(st)) == AGX_ERR_ARG
        assert lib.agx_decode_positions_tail_m(P(q), 1, W, H, 2, 6, 0.5, P(pts), P(st), model) == AGX_ERR_ARG
    for side in (0, 41, -1):
        assert lib.agx_tag_maps_tail(P(q), 1, side, 0.5, 1, P(maps), P(st)) == AGX_ERR_ARG
    assert lib.agx_tag_maps_tail(P(q), 1, 40, 0.5, 1, P(maps), P(st)) == AGX_OK and lib.agx_tag_maps_tail(P(q), 1, 1, 0.5, 0, P(maps), P(st)) == AGX_OK
    for margin in (float("nan"), float("inf")):
        assert lib.agx_tag_maps_tail(P(q), 1, 10, margin, 1, P(maps), P(st)) == AGX_ERR_ARG
        assert lib.agx_decode_positions_tail_m(P(q), 1, W, H, 2, 6, margin, P(pts), P(st), 1) == AGX_ERR_ARG
    # a degenerate source square: (float)side_bits - 1 + margin == -margin
    assert lib.agx_tag_maps_tail(P(q), 1, 1, 0.0, 1, P(maps), P(st)) == AGX_ERR_ARG
    assert lib.agx_tag_maps_tail(P(q), 1, 3, -1.0, 0, P(maps), P(st)) == AGX_ERR_ARG
    assert lib.agx_decode_positions_tail_m(P(q), 1, W, H, 0, 1, 0.0, P(pts), P(st), 1) == AGX_ERR_ARG
    for edge, border in ((0, 2), (9, 2), (6, 17), (6, -1)):
        assert lib.agx_decode_positions_tail_m(P(q), 1, W, H, border, edge, 0.5, P(pts), P(st), 1) == AGX_ERR_ARG
    for null in (0, 5, 6):
        a = [P(q), 1, 10, 0.5, 1, P(maps), P(st)]
        a[null] = None
        assert lib.agx_tag_maps_tail(*a) == AGX_ERR_ARG
    assert lib.agx_tag_maps_tail(None, 0, 10, 0.5, 1, None, None) == AGX_OK
    import aprilgrid_rs_amd as A
    with pytest.raises(A.AgxError):
        A.decode_positions(q[None], W, H, 2, 6, 0.5, model="projective")
    with pytest.raises(A.AgxError):
        A.tag_maps(q[None], 10, 0.5, 2)


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_the_m_entries_at_affine_are_the_existing_entries(fam):
    from aprilgrid_rs_amd import _ffi
    lib = _ffi.lib()
    edge, border, _, _ = T.family(fam)
    quads = np.ascontiguousarray(np.stack([c.quad for c in T.family_cases(fam)]), np.float32)
    n = len(quads)
    out = []
    for call, extra in ((lib.agx_decode_positions_tail, ()), (lib.agx_decode_positions_tail_m, (0,))):
        pts, st = np.full((n, edge * edge, 2), POISON, np.float32), np.full(n, 99, np.uint32)
        assert call(quads.ctypes.data, n, T.W, T.H, border, edge, 0.5, pts.ctypes.data, st.ctypes.data, *extra) == AGX_OK
        out.append((pts, st))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert {DECODED, OUTSIDE} == set(int(s) for s in out[0][1])


# ---- the point of the feature: a tag under perspective ------------------------------------------------------------------------
@functools.lru_cache(None)
def painted(fam):
    return HO.painted_case(fam)


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_painted_perspective_tag_decodes_under_the_homography_only(fam):
    import aprilgrid_rs_amd as A
    plane, cells, quad, code = painted(fam)
    edge, border, thres, codes = T.family(fam)
    nb = edge * edge
    word = int(codes[code])
    near = np.linalg.norm(quad[2] - quad[3])
    assert np.linalg.norm(quad[1] - quad[0]) <= 0.7 * near
    # -- from numpy alone --
    exact = HO.positions(quad, border, edge, 0.5)
    for n, (x, y) in enumerate(exact):  # every exact sample at least 1 px inside its cell's image: the pixels around it are the cell's
        ix, iy = int(np.floor(x + 0.5)), int(np.floor(y + 0.5))
        assert (cells[iy - 2:iy + 3, ix - 2:ix + 3] == n).all(), (fam, n)
    affine = T.positions_f64(quad.reshape(8), fam)
    wrong = 0
    for n, (x, y) in enumerate(affine):  # affine samples in a neighbouring cell of the other colour
        seen = int(plane[int(np.floor(y + 0.5)), int(np.floor(x + 0.5))])
        want = 235 if (word >> (nb - 1 - n)) & 1 else 20
        wrong += seen != want and seen != 128
    assert wrong >= thres + 1, (fam, wrong)
    # -- through the library --
    for r in range(4):
        qq = np.ascontiguousarray(np.roll(quad, -r, axis=0))
        pts, st = A.decode_positions(qq[None], W, H, border, edge, 0.5, model="homography")
        bits, st = A.bit_code(plane, pts, 10, 3, status_in=st)
        ids, rots, st, tags = A.best_tag(bits, thres, tag_family=fam, status_in=st, quads=qq[None])
        assert st[0] == DECODED and ids[0] == code, (fam, r, st, ids)
        corners = np.roll(qq, -int(rots[0]), axis=0)[::-1]  # rotate_left(rotation); reverse() -- agx_decode_quads_tail's
        assert tags[0]["id"] == code and np.array_equal(np.asarray(tags[0]["xy"], np.float32).reshape(4, 2), corners)
        # the existing path on the same quad: pinned, it must not change
        pa, sa = A.decode_positions(qq[None], W, H, border, edge, 0.5, model="affine")
        ba, sa = A.bit_code(plane, pa, 10, 3, status_in=sa)
        ia, _, sa = A.best_tag(ba, thres, tag_family=fam, status_in=sa)
        assert sa[0] != DECODED or ia[0] != code, (fam, r)
        ft, fs = A.decode_quads_tail(fam, plane, qq[None])
        assert fs[0] == sa[0] and (fs[0] != DECODED or ft[0]["id"] == ia[0])


def test_header_library_ctypes_and_rust_declare_the_entries():
    import os
    import re
    from aprilgrid_rs_amd import _ffi
    from tests.util import ROOT
    header = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for fn, n_args in (("agx_decode_positions_enqueue_m", 15), ("agx_decode_positions_tail_m", 10), ("agx_tag_maps_enqueue", 12), ("agx_tag_maps_tail", 7)):
        assert re.search(r"\bint %s\(" % fn, header) and ("pub fn %s(" % fn) in rust and len(_ffi.SYMBOLS[fn][1]) == n_args, fn
        assert getattr(_ffi.lib(), fn).argtypes == _ffi.SYMBOLS[fn][1]
    for name, value in (("AGX_TAG_MAP_AFFINE", 0), ("AGX_TAG_MAP_HOMOGRAPHY", 1), ("AGX_QUAD_DEGENERATE", 6)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header) and getattr(_ffi, name) == value
        assert "pub const %s: c_int = %d;" % (name, value) in rust
    for fn in ("pub fn tag_homography(", "pub fn tag_maps_tail(", "pub fn decode_positions_m("):
        assert fn in lib_rs, fn
    assert re.search(r"#define AGX_ABI_VERSION 1\b", header)
    for cite in ("src/image_util.rs:5-37", "src/image_util.rs:39-70"):
        assert cite in header
