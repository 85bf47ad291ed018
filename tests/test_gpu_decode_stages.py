"""The decode in three stages on the device: agx_decode_positions_enqueue (k_decode_positions), agx_bit_code_enqueue (k_bit_code)
and agx_best_tag_enqueue (k_best_tag) -- reference src/detector.rs:42-72, :74-122, :142-169.

Each kernel against its host form, byte for byte, on the inputs of tests/test_decode_stages_cpu.py (which holds the host forms to
the oracle); the three chained on device arrays with no sync in between against agx_decode_quads_enqueue and, through
agx_collect_tags_enqueue, against the fused path's tag table; counts, sentinels around every output, strides, formats, long code
lists, argument errors and the caller's stream.  Frames are 64 x 48 unless a test's inputs bring their own."""
import ctypes as C

import numpy as np
import pytest

from tests import tag_cases as T
from tests import test_decode_stages_cpu as S
from tests.test_decode_quads_cpu import TAG_DTYPE, family

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_STATE = 0, -1, -2, -7
AGX_L8, AGX_LF32 = 0, 3
DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS, NO_MATCH, SKIPPED = range(6)
SENT = 0x7E7E7E7E
MARGIN = 64  # sentinel words in front of and behind every output
W, H = S.PW, S.PH
S_BT_LDS_CODES = 640  # csrc/decode_stages.h BT_LDS_CODES: the longest code list k_best_tag stages in LDS


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """An output array of `words` 32-bit words filled with the sentinel, MARGIN sentinel words in front and behind."""

    def __init__(self, shape, dtype):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.words = int(np.prod(shape)) * self.dtype.itemsize // 4
        self.raw = torch.full((2 * MARGIN + self.words,), SENT, dtype=torch.int32, device="cuda")
        tdt = {"float32": torch.float32, "int32": torch.int32, "uint32": torch.int32, "int64": torch.int64, "uint64": torch.int64}[self.dtype.name]
        self.t = self.raw[MARGIN:MARGIN + self.words].view(tdt).view(*[int(s) for s in shape])

    def host(self):
        """-> the payload as a numpy array of the dtype; asserts that the margins survived"""
        raw = self.raw.cpu().numpy().view(np.uint32)
        assert (raw[:MARGIN] == SENT).all() and (raw[MARGIN + self.words:] == SENT).all(), "a sentinel word outside the array was overwritten"
        return raw[MARGIN:MARGIN + self.words].view(self.dtype).reshape(self.shape).copy()


def sentinel(dtype):
    return np.full(1, SENT, np.uint32).view(np.uint32).repeat(np.dtype(dtype).itemsize // 4).view(dtype)[0]


def written(counts, qpf, n):
    """[n, qpf] bool: the slots below a frame's count (a count above qpf means qpf)"""
    c = np.minimum(np.asarray(counts if counts is not None else [qpf] * n, np.int64), qpf)
    return np.arange(qpf)[None, :] < c[:, None]


# ---- k_decode_positions -------------------------------------------------------------------------------------------------------
def positions_quads():
    """[3, 16, 8]: the decision quads of a 64 x 48 image (corners at the edges, negative, huge, +inf), random ones, NaN and -inf"""
    q = S.decision_quads(W, H)
    rng = np.random.default_rng(3)
    q = np.concatenate([q[-14:], S.random_quads(rng, 34, W, H, lo=6.0, hi=40.0)])
    q[20, 3], q[31, 6] = np.nan, -np.inf
    return q.reshape(3, 16, 8)


@pytest.mark.parametrize("counts", [None, [0, 20, 5]])
def test_decode_positions_kernel_equals_the_host_form(det, counts):
    import aprilgrid_rs_amd as A
    quads = positions_quads()
    d_quads = dev(quads)
    d_counts = dev(np.array(counts, np.int32)) if counts else None
    live = written(counts, 16, 3)
    for border, edge in S.SETTINGS:
        for margin in S.MARGINS:
            if S.degenerate(border, edge, margin):
                continue
            pts, st = Guarded((3, 16, edge * edge, 2), np.float32), Guarded((3, 16), np.uint32)
            det.decode_positions_enqueue(d_quads, pts.t, st.t, img_size=(W, H), border_bits=border, edge_bits=edge, margin=margin, counts=d_counts)
            det.sync()
            hp, hs = A.decode_positions(quads.reshape(48, 8), W, H, border, edge, margin)
            gp, gs = pts.host(), st.host()
            hp, hs = hp.reshape(3, 16, edge * edge, 2), hs.reshape(3, 16)
            assert np.array_equal(gs[live], hs[live]) and (gs[~live] == SENT).all(), (border, edge, margin)
            ok = live & (hs == DECODED)
            assert gp[ok].tobytes() == hp[ok].tobytes(), (border, edge, margin)
            assert (gp[~ok].view(np.uint32) == SENT).all(), "a slot that is not DECODED, or beyond its frame's count, wrote a point"
    assert set(np.unique(hs)) == {DECODED, OUTSIDE}


def test_decode_positions_reads_refine_records_and_skips_unrefined_corners(det):
    """point stride 20 (agx_saddle records) with the refine statuses: a corner whose word is non-zero makes the quad SKIPPED"""
    import aprilgrid_rs_amd as A
    quads = positions_quads()
    records = np.full((3, 64, 5), np.nan, np.float32)  # (k, theta, phi are never read)
    records[:, :, 0:2] = quads.reshape(3, 64, 2)
    pstatus = np.zeros((3, 64), np.int32)
    pstatus[0, 5], pstatus[1, 0], pstatus[2, 63], pstatus[2, 62] = 2, 1, 3, 1  # quads (0, 1), (1, 0), (2, 15)
    pts, st = Guarded((3, 16, 36, 2), np.float32), Guarded((3, 16), np.uint32)
    det.decode_positions_enqueue(None, pts.t, st.t, img_size=(W, H), refined=(dev(records), dev(pstatus)))
    det.sync()
    hp, hs = A.decode_positions(quads.reshape(48, 8), W, H, 2, 6, 0.5)
    hp, hs = hp.reshape(3, 16, 36, 2), hs.reshape(3, 16).copy()
    for f, q in ((0, 1), (1, 0), (2, 15)):
        hs[f, q] = SKIPPED
    gp, gs = pts.host(), st.host()
    assert np.array_equal(gs, hs)
    ok = hs == DECODED
    assert gp[ok].tobytes() == hp[ok].tobytes() and (gp[~ok].view(np.uint32) == SENT).all()


# ---- k_bit_code ---------------------------------------------------------------------------------------------------------------
def bit_code_groups():
    """The CPU file's cases by (P, threshold, max_invalid_bit): one launch each, a frame per case and two slots per frame -- the
    case's points, and the next case's points on this case's plane"""
    groups = {}
    for c in S.bit_code_cases():
        groups.setdefault((len(c[2]), c[3], c[4]), []).append(c)
    return groups


def test_bit_code_kernel_equals_the_host_form(det):
    import aprilgrid_rs_amd as A
    seen = set()
    for (p, thr, max_inv), cases in sorted(bit_code_groups().items()):
        n = len(cases)
        planes = np.stack([c[1] for c in cases])
        pts = np.stack([np.stack([cases[f][2], cases[(f + 1) % n][2]]) for f in range(n)])  # [n, 2, P, 2]
        bits, st = Guarded((n, 2), np.uint64), Guarded((n, 2), np.uint32)
        det.bit_code_enqueue(dev(planes), dev(pts), bits.t, st.t, valid_brightness_threshold=thr, max_invalid_bit=max_inv)
        det.sync()
        gb, gs = bits.host(), st.host()
        for f in range(n):
            hb, hs = A.bit_code(planes[f], pts[f], thr, max_inv)
            assert np.array_equal(gs[f], hs) and np.array_equal(gb[f], hb), (cases[f][0], gs[f], hs, gb[f], hb)
            assert cases[f][5] is None or gs[f, 0] == cases[f][5], cases[f][0]
        seen |= set(int(s) for s in gs.reshape(-1))
    assert seen == {DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS}


def bit_code_batch():
    """3 frames x 16 slots x 36 points on noise planes with a bright / dark pattern under most slots -> (planes, points)"""
    rng = np.random.default_rng(12)
    planes = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    pts = np.zeros((3, 16, 36, 2), np.float32)
    for f in range(3):
        for q in range(16):
            g = S.grid_points(36, x0=2.0 + 3 * (q % 8), y0=3.0 + 20 * (q // 8), cols=6) + rng.uniform(-0.45, 0.45, (36, 2)).astype(np.float32)
            pts[f, q] = g
            if q % 4:
                ix, iy = np.rint(g[:, 0]).astype(int), np.rint(g[:, 1]).astype(int)
                planes[f, iy, ix] = np.where(rng.integers(0, 2, 36) == 1, 220, 15)
    pts[1, 3, 7, 0] = W + 0.6  # outside
    pts[2, 9, 0, 1] = np.nan
    return planes, pts


def host_bit_code_batch(planes, pts, thr=10, max_inv=3, status_in=None):
    import aprilgrid_rs_amd as A
    out = [A.bit_code(planes[f], pts[f], thr, max_inv, status_in=None if status_in is None else status_in[f]) for f in range(len(planes))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("counts", [None, [16, 0, 40]])
def test_bit_code_counts_status_pass_through_and_aliasing(det, counts):
    planes, pts = bit_code_batch()
    s_in = np.zeros((3, 16), np.uint32)
    s_in[0, 2], s_in[1, 3], s_in[2, 0], s_in[2, 15] = SKIPPED, OUTSIDE, 0xDEAD, NO_MATCH
    hb, hs = host_bit_code_batch(planes, pts, status_in=s_in)
    assert (hs == DECODED).sum() >= 20 and {OUTSIDE, SKIPPED, 0xDEAD} <= set(int(s) for s in hs.reshape(-1))
    live = written(counts, 16, 3)
    d_counts = dev(np.array(counts, np.int32)) if counts else None
    d_planes, d_pts = dev(planes), dev(pts)
    # a status array of its own
    bits, st = Guarded((3, 16), np.uint64), Guarded((3, 16), np.uint32)
    det.bit_code_enqueue(d_planes, d_pts, bits.t, st.t, counts=d_counts, status_in=dev(s_in.view(np.int32)))
    det.sync()
    gb, gs = bits.host(), st.host()
    assert np.array_equal(gs[live], hs[live]) and np.array_equal(gb[live], hb[live])
    assert (gs[~live] == SENT).all() and (gb[~live] == sentinel(np.uint64)).all()
    # d_status_in is d_status
    bits, st = Guarded((3, 16), np.uint64), Guarded((3, 16), np.uint32)
    st.t.copy_(dev(s_in.view(np.int32)))
    det.bit_code_enqueue(d_planes, d_pts, bits.t, st.t, counts=d_counts, status_in=st.t)
    det.sync()
    gb, gs = bits.host(), st.host()
    assert np.array_equal(gs[live], hs[live]) and np.array_equal(gb[live], hb[live])
    assert np.array_equal(gs[~live], s_in[~live]) and (gb[~live] == sentinel(np.uint64)).all()


def test_bit_code_rgb8_frames_and_a_padded_row_stride(det):
    import aprilgrid_rs_amd as A
    planes, pts = bit_code_batch()
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    luma = np.stack([A.TagDetector.luma8(rgb[f]) for f in range(3)])
    hb, hs = host_bit_code_batch(luma, pts, thr=4, max_inv=30)
    bits, st = Guarded((3, 16), np.uint64), Guarded((3, 16), np.uint32)
    det.bit_code_enqueue(dev(rgb), dev(pts), bits.t, st.t, valid_brightness_threshold=4, max_invalid_bit=30)
    det.sync()
    assert np.array_equal(st.host(), hs) and np.array_equal(bits.host(), hb) and (hs == DECODED).sum() >= 8
    # rows 80 bytes apart, frames with a gap behind them: the padding holds 255 and is never read
    hb, hs = host_bit_code_batch(planes, pts)
    wide = np.full((3, H + 2, 80), 255, np.uint8)
    wide[:, :H, :W] = planes
    d_wide, d_pts = dev(wide), dev(pts)
    bits, st = Guarded((3, 16), np.uint64), Guarded((3, 16), np.uint32)
    det._follow_torch_stream(d_wide)
    assert det._lib.agx_bit_code_enqueue(det._h, d_wide.data_ptr(), 3, W, H, 80, 80 * (H + 2), AGX_L8, d_pts.data_ptr(), 36, 16, None, None, 10, 3,
                                         bits.t.data_ptr(), st.t.data_ptr()) == AGX_OK
    det.sync()
    assert np.array_equal(st.host(), hs) and np.array_equal(bits.host(), hb)


# ---- k_best_tag ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(S.best_tag_sets())), ids=[s[0] for s in S.best_tag_sets()])
def test_best_tag_kernel_equals_the_host_form(det, i):
    """The CPU file's sets: the five families, lists of 1 .. 4096 codes (640 is the last the kernel stages in LDS, 641 the first it
    reads in place), edge_bits 1, 7 and 8, ties, bits above edge_bits^2, thres 0 -- with the tags made of quads."""
    import aprilgrid_rs_amd as A
    name, codes, edge, thres, bits = S.best_tag_sets()[i]
    m = len(bits)
    quads = np.random.default_rng(i).uniform(0, 60, (1, m, 8)).astype(np.float32)
    hi, hr, hs, ht = A.best_tag(bits, thres, codes=codes, edge_bits=edge, quads=quads)
    ids, rots, st, tags = Guarded((1, m), np.uint32), Guarded((1, m), np.uint32), Guarded((1, m), np.uint32), Guarded((1, m, 9), np.uint32)
    det.best_tag_enqueue(dev(bits.view(np.int64).reshape(1, m)), ids.t, rots.t, st.t, thres=thres, codes=dev(codes.view(np.int64)), edge_bits=edge,
                         quads=dev(quads), tags=tags.t)
    det.sync()
    assert np.array_equal(st.host()[0], hs) and np.array_equal(ids.host()[0], hi) and np.array_equal(rots.host()[0], hr), name
    assert tags.host().tobytes() == ht.tobytes(), name
    if name == "T36H11":  # NULL codes = the handle's family list, thres and edge_bits the family's by default; no tags
        ids, rots, st = (Guarded((1, m), np.uint32) for _ in range(3))
        det.best_tag_enqueue(dev(bits.view(np.int64).reshape(1, m)), ids.t, rots.t, st.t)
        det.sync()
        assert np.array_equal(st.host()[0], hs) and np.array_equal(ids.host()[0], hi) and np.array_equal(rots.host()[0], hr)


def test_best_tag_counts_status_pass_through_aliasing_and_stride_20(det):
    import aprilgrid_rs_amd as A
    _, codes, edge, thres, probe = [s for s in S.best_tag_sets() if s[0] == "random 641"][0]
    bits = np.resize(probe, 48).reshape(3, 16)
    s_in = np.zeros((3, 16), np.uint32)
    s_in[0, 1], s_in[1, 15], s_in[2, 0] = AMBIGUOUS, SKIPPED, 0xDEAD
    counts = [3, 0, 99]
    live = written(counts, 16, 3)
    records = np.random.default_rng(8).uniform(0, 60, (3, 64, 5)).astype(np.float32)
    quads = np.ascontiguousarray(records[:, :, 0:2]).reshape(48, 8)
    hi, hr, hs, ht = A.best_tag(bits.reshape(-1), thres, codes=codes, edge_bits=edge, status_in=s_in.reshape(-1), quads=quads)
    hi, hr, hs, ht = hi.reshape(3, 16), hr.reshape(3, 16), hs.reshape(3, 16), ht.view(np.uint32).reshape(3, 16, 9)
    ids, rots, st, tags = Guarded((3, 16), np.uint32), Guarded((3, 16), np.uint32), Guarded((3, 16), np.uint32), Guarded((3, 16, 9), np.uint32)
    st.t.copy_(dev(s_in.view(np.int32)))
    det.best_tag_enqueue(dev(bits.view(np.int64)), ids.t, rots.t, st.t, thres=thres, codes=dev(codes.view(np.int64)), edge_bits=edge,
                         counts=dev(np.array(counts, np.int32)), status_in=st.t, refined=(dev(records), dev(np.zeros((3, 64), np.int32))), tags=tags.t)
    det.sync()
    gi, gr, gs, gt = ids.host(), rots.host(), st.host(), tags.host()
    assert np.array_equal(gs[live], hs[live]) and np.array_equal(gi[live], hi[live]) and np.array_equal(gr[live], hr[live])
    assert gt[live].tobytes() == ht[live].tobytes() and (hs[live] == DECODED).sum() >= 8
    assert np.array_equal(gs[~live], s_in[~live]) and (gi[~live] == SENT).all() and (gr[~live] == SENT).all() and (gt[~live] == SENT).all()


# ---- where a sampler and a scan written for any lane count and pass count can go wrong ----------------------------------------
@pytest.mark.parametrize("p", [1, 16, 17, 48, 49, 64])
def test_bit_code_at_the_pass_boundaries_of_the_row(det, p):
    """points_per_slot at the ends of the 16-lane form's four passes: the last sample is lane 15's of a pass or lane 0's of the next.
    Frame 0: noise under random points; frame 1: bright samples exactly at the indices 0, 15, 16, 31, 32, 47, 48, p - 1 (their bits
    are the ones a wrong pass count drops or misplaces), and the same points with the LAST one outside the image."""
    import aprilgrid_rs_amd as A
    rng = np.random.default_rng(100 + p)
    pts = np.zeros((2, 8, p, 2), np.float32)
    pts[0] = np.stack([rng.uniform(-0.4, W - 0.6, (8, p)), rng.uniform(-0.4, H - 0.6, (8, p))], axis=-1)
    grid = S.grid_points(p)
    pts[1, :] = grid
    pts[1, 1, p - 1] = (W - 0.5, 3.0)
    marks = [i for i in (0, 15, 16, 31, 32, 47, 48, p - 1) if i < p]
    planes = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), S.painted(grid, np.where(np.isin(np.arange(p), marks), 210, 20))])
    bits, st = Guarded((2, 8), np.uint64), Guarded((2, 8), np.uint32)
    det.bit_code_enqueue(dev(planes), dev(pts), bits.t, st.t, valid_brightness_threshold=10, max_invalid_bit=3)
    det.sync()
    hb, hs = host_bit_code_batch(planes, pts)
    gb, gs = bits.host(), st.host()
    assert np.array_equal(gs, hs) and np.array_equal(gb, hb), (p, gs, hs, gb, hb)
    assert hs[1, 1] == OUTSIDE and hs[1, 0] == (LOW_CONTRAST if len(set(marks)) == p else DECODED)
    if hs[1, 0] == DECODED:
        assert int(hb[1, 0]) == sum(1 << (p - 1 - i) for i in set(marks))


@pytest.mark.parametrize("n", [1, 15, 16, 17, S_BT_LDS_CODES + 1])
def test_best_tag_best_code_last_and_ties_at_the_list_lengths_of_the_scan(det, n):
    """Lists that end in lane 0, 14, 15 and 0 of the next pass, and the first length that is read where it lies: the best code is
    the LAST of the list (exact and one bit away), and two codes at the same distance -- in neighbouring lanes (n - 3, n - 2) and
    in the same lane a pass apart (n - 17, n - 1: the last code again) -- where the lower index wins."""
    import aprilgrid_rs_amd as A
    rng = np.random.default_rng(500 + n)
    codes = rng.integers(0, 1 << 36, n, dtype=np.uint64)
    a, b = 0x5A5A5A5A5, 0x3C3C3C3C3
    probes, want = [], []
    if n >= 15:
        codes[n - 3], codes[n - 2] = a, a ^ 0b11
        probes, want = [a ^ 0b01], [n - 3]
    if n >= 17:
        codes[n - 17], codes[n - 1] = b, b ^ 0b11
        probes, want = probes + [b ^ 0b10], want + [n - 17]
    last = int(codes[n - 1])
    bits = np.array(probes + [last, last ^ (1 << 20)], np.uint64)
    want += [n - 1, n - 1]
    m = len(bits)
    quads = rng.uniform(0, 60, (1, m, 8)).astype(np.float32)
    hi, hr, hs, ht = A.best_tag(bits, 4, codes=codes, edge_bits=6, quads=quads)
    assert (hs == DECODED).all() and list(hi) == want and (hr == 0).all(), "the inputs are not what the test is about"
    ids, rots, st, tags = Guarded((1, m), np.uint32), Guarded((1, m), np.uint32), Guarded((1, m), np.uint32), Guarded((1, m, 9), np.uint32)
    det.best_tag_enqueue(dev(bits.view(np.int64).reshape(1, m)), ids.t, rots.t, st.t, thres=4, codes=dev(codes.view(np.int64)), edge_bits=6,
                         quads=dev(quads), tags=tags.t)
    det.sync()
    assert np.array_equal(st.host()[0], hs) and np.array_equal(ids.host()[0], hi) and np.array_equal(rots.host()[0], hr), n
    assert tags.host().tobytes() == ht.tobytes(), n


# ---- the three chained against the fused kernel -------------------------------------------------------------------------------
def chain(d, frames, quads, counts=None, refined=None, fmt=None):
    """decode_positions -> bit_code -> best_tag on device arrays, one status array handed on, no sync or fetch in between
    -> Guarded (tags, status, bits, points)"""
    n, qpf = (int(quads.shape[0]), int(quads.shape[1])) if quads is not None else (int(refined[0].shape[0]), int(refined[0].shape[1]) // 4)
    edge = d._family_info()[0]
    h, w = (int(frames.shape[1]), int(frames.shape[2]))
    pts, st, bits = Guarded((n, qpf, edge * edge, 2), np.float32), Guarded((n, qpf), np.uint32), Guarded((n, qpf), np.uint64)
    ids, rots, tags = Guarded((n, qpf), np.uint32), Guarded((n, qpf), np.uint32), Guarded((n, qpf, 9), np.uint32)
    d.decode_positions_enqueue(quads, pts.t, st.t, img_size=(w, h), counts=counts, refined=refined)
    d.bit_code_enqueue(frames, pts.t, bits.t, st.t, counts=counts, status_in=st.t, format=fmt)
    d.best_tag_enqueue(bits.t, ids.t, rots.t, st.t, counts=counts, status_in=st.t, quads=quads, refined=refined, tags=tags.t)
    return tags, st, bits, pts


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_chained_stages_equal_k_decode_quads_on_the_painted_cases(fam):
    import aprilgrid_rs_amd as A
    cs = T.family_cases(fam)
    n = len(cs)
    d_planes = dev(np.stack([c.plane for c in cs]))
    d_quads = dev(np.stack([c.quad for c in cs]).reshape(n, 1, 8))
    d = A.TagDetector(fam, None, device=0)
    try:
        ftags, fst, fbits = Guarded((n, 1, 9), np.uint32), Guarded((n, 1), np.uint32), Guarded((n, 1), np.uint64)
        d.decode_quads_enqueue(d_planes, d_quads, out=ftags.t, status=fst.t, bits=fbits.t)
        tags, st, bits, _ = chain(d, d_planes, d_quads)
        d.sync()
    finally:
        d.close()
    gs, hs = st.host(), fst.host()
    assert np.array_equal(gs, hs) and bits.host().tobytes() == fbits.host().tobytes() and tags.host().tobytes() == ftags.host().tobytes()
    assert len(np.unique(gs)) == 5, np.bincount(gs.reshape(-1).astype(np.int64))
    for i, c in enumerate(cs):  # and what each case expects
        assert gs[i, 0] == c.expect[0], c.name


def test_chained_stages_on_a_board_frame_feed_collect_tags_like_the_fused_path(det):
    """Three 320 x 240 frames with a synthetic board each through the staged chain up to agx_find_boards_enqueue; its quad points
    and counts (slots beyond a count hold the sentinel) through the fused kernel and through the three stages; both results
    through agx_collect_tags_enqueue."""
    import torch
    from aprilgrid_rs_amd import synth
    n, sw, sh, cpf, qpf, tpf = 3, 320, 240, 1024, 64, 64
    frames, _ = synth.render_batch(40, n, sw, sh, device="cuda:0")
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    blur, resp = torch.empty((n, sh, sw), **f32), torch.empty((n, sh, sw), **f32)
    rows, cpts = torch.zeros((n, cpf, 4), **i32), torch.zeros((n, cpf, 2), **f32)
    counts, cst = torch.zeros(n, **i32), torch.zeros(n, **i32)
    records, pstatus = torch.zeros((n, cpf, 5), **f32), torch.zeros((n, cpf), **i32)
    det.planes_enqueue(frames, det.blur_sigma, blur=blur, response=resp)
    det.clusters_enqueue(resp, clusters=rows, points=cpts, counts=counts, status=cst)
    det.refine_points_enqueue(blur, cpts, counts=counts, out=records, status=pstatus, image="plane")
    det.filter_saddles_enqueue(records, pstatus, counts=counts)
    quads, nq, bst = torch.zeros((n, qpf, 4), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
    qpts = torch.full((n, qpf, 4, 2), float("nan"), **f32)
    det.find_boards_enqueue(records, counts=counts, point_status=pstatus, quads=quads, quad_points=qpts, n_quads=nq, status=bst)
    det.find_boards_fetch()
    assert (bst.cpu().numpy() == 0).all() and (nq.cpu().numpy() >= 6).all(), (bst, nq)
    ftags, fst, fbits = Guarded((n, qpf, 9), np.uint32), Guarded((n, qpf), np.uint32), Guarded((n, qpf), np.uint64)
    det.decode_quads_enqueue(frames, qpts, counts=nq, out=ftags.t, status=fst.t, bits=fbits.t)
    tags, st, bits, _ = chain(det, frames, qpts, counts=nq)
    tables = []
    for qt, qs in ((ftags, fst), (tags, st)):
        tt, nt, ts = torch.zeros((n, tpf, 9), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        det.collect_tags_enqueue(quads, nq, bst, qt.t, qs.t, None, tt, nt, ts, reset=True, saddles_per_frame=cpf)
        tables.append((tt, nt, ts))
    det.sync()
    assert st.host().tobytes() == fst.host().tobytes() and bits.host().tobytes() == fbits.host().tobytes()
    assert tags.host().tobytes() == ftags.host().tobytes()
    live = written(nq.cpu().numpy(), qpf, n)
    assert (st.host()[live] == DECODED).sum() >= 12 and (st.host()[~live] == SENT).all()
    (ta, na, sa), (tb, nb_, sb) = tables
    assert torch.equal(ta, tb) and torch.equal(na, nb_) and torch.equal(sa, sb) and (na.cpu().numpy() >= 4).all() and not sa.cpu().numpy().any()


def test_decode_quads_staged_returns_the_fused_result_and_the_points(det):
    import aprilgrid_rs_amd as A
    from tests.test_decode_quads_cpu import jittered_quads
    frames, quads = jittered_quads(3, 16, 5)
    d_frames, d_quads = dev(frames), dev(quads.reshape(3, 16, 4, 2))
    det.decode_quads_enqueue(d_frames, d_quads)
    ftags, fst, fbits = det.decode_quads_fetch()
    tags, st, bits, pts = det.decode_quads_staged(d_frames, d_quads)
    assert tags.tobytes() == ftags.tobytes() and np.array_equal(st, fst) and np.array_equal(bits, fbits) and (st == DECODED).sum() >= 8
    h, w = frames.shape[1:]
    hp, hs = A.decode_positions(quads.reshape(48, 8), w, h, 2, 6, 0.5)
    assert pts.reshape(48, 36, 2)[hs == DECODED].tobytes() == hp[hs == DECODED].tobytes()
    # a sub-family as the code list and looser brightness rules: the host forms' answer
    _, _, hamming, codes = family("T36H11")
    sub = np.ascontiguousarray(codes[::2])
    tags2, st2, bits2, _ = det.decode_quads_staged(d_frames, d_quads, margin=0.25, valid_brightness_threshold=5, max_invalid_bit=6, thres=5, codes=sub)
    for f in range(3):
        hp, hs = A.decode_positions(quads[f], w, h, 2, 6, 0.25)
        hb, hs = A.bit_code(frames[f], hp, 5, 6, status_in=hs)
        _, _, hs, ht = A.best_tag(hb, 5, codes=sub, edge_bits=6, status_in=hs, quads=quads[f])
        assert np.array_equal(st2[f], hs) and np.array_equal(bits2[f], hb) and tags2[f].tobytes() == ht.tobytes()


# ---- arguments, state, the caller's stream ----------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_batch_in_flight(det):
    import torch
    lib, h = det._lib, det._h
    i32 = dict(dtype=torch.int32, device="cuda")
    frames = torch.zeros((3, H, W), dtype=torch.uint8, device="cuda")
    quads = torch.zeros((3, 16, 8), dtype=torch.float32, device="cuda")
    pts = torch.zeros((3, 16, 64, 2), dtype=torch.float32, device="cuda")
    st, ids, rots = torch.zeros((3, 16), **i32), torch.zeros((3, 16), **i32), torch.zeros((3, 16), **i32)
    bits = torch.zeros((3, 16), dtype=torch.int64, device="cuda")
    codes = torch.zeros(700, dtype=torch.int64, device="cuda")
    tags = torch.zeros((3, 16, 9), **i32)
    counts = torch.zeros(3, **i32)
    P = lambda t: t.data_ptr()
    good_pos = [P(quads), 8, 3, 16, P(counts), None, W, H, 2, 6, C.c_float(0.5), P(pts), P(st)]
    bad_pos = {"null quads": {0: None}, "stride 6": {1: 6}, "stride 4": {1: 4}, "no frames": {2: 0}, "no quads per frame": {3: 0},
               "misaligned counts": {4: P(counts) + 2}, "edge 0": {9: 0}, "edge 9": {9: 9}, "border 17": {8: 17}, "border -1": {8: -1},
               "margin nan": {10: C.c_float(float("nan"))}, "margin inf": {10: C.c_float(float("inf"))},
               "degenerate square": {8: 0, 9: 1, 10: C.c_float(0.0)}, "null points": {11: None}, "null status": {12: None},
               "misaligned points": {11: P(pts) + 2}, "2^29 slots": {2: 1 << 15, 3: 1 << 14}}
    good_bit = [P(frames), 3, W, H, W, W * H, AGX_L8, P(pts), 36, 16, P(counts), None, 10, 3, P(bits), P(st)]
    bad_bit = {"null frames": {0: None}, "null points": {7: None}, "no points": {8: 0}, "65 points": {8: 65}, "no quads per frame": {9: 0},
               "threshold -1": {12: -1}, "threshold 256": {12: 256}, "null bits": {14: None}, "null status": {15: None},
               "bits not 8-byte aligned": {14: P(bits) + 4}, "misaligned status_in": {11: P(st) + 1}, "row stride below the width": {4: W - 1},
               "no frames": {1: 0}}
    good_tag = [P(bits), 48, 16, P(counts), None, 11, P(codes), 700, 6, P(quads), 8, P(ids), P(rots), P(st), P(tags)]
    bad_tag = {"null bits": {0: None}, "no slots": {1: 0}, "2^31 slots": {1: 1 << 31, 3: None}, "counts and 47 slots": {1: 47},
               "counts and no quads per frame": {2: 0}, "thres -1": {5: -1}, "thres 256": {5: 256}, "codes without a count": {7: 0},
               "65536 codes": {7: 65536}, "a count without codes": {6: None}, "edge 0": {8: 0}, "edge 9": {8: 9}, "quads without tags": {14: None},
               "tags without quads": {9: None}, "stride 6": {10: 6}, "null ids": {11: None}, "null rotations": {12: None}, "null status": {13: None},
               "codes not 8-byte aligned": {6: P(codes) + 4}, "misaligned tags": {14: P(tags) + 2}}
    det.saddles_batch_enqueue(frames)
    for fn, good, bad in ((lib.agx_decode_positions_enqueue, good_pos, bad_pos), (lib.agx_bit_code_enqueue, good_bit, bad_bit),
                          (lib.agx_best_tag_enqueue, good_tag, bad_tag)):
        for what, change in bad.items():
            a = list(good)
            for i, v in change.items():
                a[i] = v
            assert fn(h, *a) == AGX_ERR_ARG, what
        assert fn(None, *good) == AGX_ERR_ARG
    a = list(good_bit)
    a[6] = AGX_LF32
    a[4], a[5] = 4 * W, 4 * W * H
    assert lib.agx_bit_code_enqueue(h, *a) == AGX_ERR_FORMAT
    a = list(good_bit)
    a[6] = 99
    assert lib.agx_bit_code_enqueue(h, *a) == AGX_ERR_FORMAT
    res, fst = det.saddles_batch_fetch()  # the saddle batch is still in flight
    assert len(res) == 3 and (fst == 0).all()
    # a good call of each replaces the batch, has no fetch of its own, and every kind's fetch is AGX_ERR_STATE
    cnt, sti = np.zeros(3, np.uint32), np.zeros(3, np.int32)
    sad = np.zeros((3, 8, 5), np.float32)
    for fn, good in ((lib.agx_decode_positions_enqueue, good_pos), (lib.agx_bit_code_enqueue, good_bit), (lib.agx_best_tag_enqueue, good_tag)):
        det.saddles_batch_enqueue(frames)
        assert fn(h, *good) == AGX_OK
        assert lib.agx_saddles_batch_fetch(h, sad.ctypes.data, 8, cnt.ctypes.data, sti.ctypes.data) == AGX_ERR_STATE
        assert lib.agx_decode_quads_fetch(h, None, None, None) == AGX_ERR_STATE
        assert lib.agx_find_boards_fetch(h, None, None, None, None, 0) == AGX_ERR_STATE
    det.sync()


def test_the_stages_run_on_the_callers_stream(det):
    """Under torch.cuda.stream(s) the binding hands s to agx_detector_set_stream: the inputs are produced on s right before the
    stages, the results are read after s alone has been waited for."""
    import torch
    from tests.test_decode_quads_cpu import jittered_quads
    frames, quads = jittered_quads(3, 16, 6)
    det.decode_quads_enqueue(dev(frames), dev(quads.reshape(3, 16, 8)))
    ftags, fst, fbits = det.decode_quads_fetch()
    s = torch.cuda.Stream()
    h_frames, h_quads = torch.from_numpy(frames).pin_memory(), torch.from_numpy(np.ascontiguousarray(quads.reshape(3, 16, 8))).pin_memory()
    with torch.cuda.stream(s):
        d_frames, d_quads = h_frames.to("cuda", non_blocking=True), h_quads.to("cuda", non_blocking=True)
        tags, st, bits, _ = chain(det, d_frames, d_quads)
        assert det._stream_ptr == s.cuda_stream
    s.synchronize()
    assert np.array_equal(st.host(), fst) and np.array_equal(bits.host(), fbits) and tags.host().tobytes() == ftags.tobytes()
