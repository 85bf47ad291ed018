"""rochade_refine of caller-given points on device batches (agx_refine_points_enqueue / _fetch, agx_rochade_refine; reference
src/detector.rs:194-361) against the oracle's orc_rochade_refine, called one point at a time so that every point has its own
answer.  Per refined point x, y and k are the oracle's bit for bit and theta, phi within tests/util.ANGLE_TOL_DEG -- the bar
the chain's own refinement is held to --; the refined set is exactly the oracle's accepted set; AGX_POINT_OUTSIDE is exactly
the rule of the header, computed here in Python (the oracle is never asked about such a point: its `as i32` + indexing is
undefined there); a rejected point's record is zero."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import ANGLE_TOL_DEG, bits_equal, check_saddles, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_STATE = 0, -1, -2, -7
REFINED, OUTSIDE, NOT_SADDLE, MOVED = 0, 1, 2, 3
BLURRED, PLANE = 0, 1
L8, L16, RGB8, LF32, BGRA8 = 0, 1, 2, 3, 7
W, H = 320, 200
UNWRITTEN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


# ---- the yardstick --------------------------------------------------------------------------------------------------------
def roundf(v):
    """C's roundf (half away from zero) of float32 values, in binary64 (|v| + 0.5 is exact there)."""
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.sign(v) * np.floor(np.abs(v) + 0.5)


def outside_rule(pts, w, h):
    """AGX_POINT_OUTSIDE unless both coordinates are finite, roundf(x) in [4, w-5] and roundf(y) in [4, h-5]."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    rx, ry = roundf(pts[:, 0]), roundf(pts[:, 1])
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(pts).all(axis=1) & (rx >= 4) & (rx <= w - 5) & (ry >= 4) & (ry <= h - 5)
    return ~inside


def oracle_points(O, plane, pts):
    """-> (accepted [n] bool, records [n] SADDLE_DTYPE) of orc_rochade_refine(plane, ..., half = 2), one point per call; points
    the rule above puts outside are not handed to it."""
    plane = np.ascontiguousarray(plane, np.float32)
    h, w = plane.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    acc = np.zeros(len(pts), bool)
    rec = np.zeros(len(pts), O.SADDLE_DTYPE)
    out = np.zeros(1, O.SADDLE_DTYPE)
    lib = O.lib()
    for i in np.flatnonzero(~outside_rule(pts, w, h)):
        one = np.ascontiguousarray(pts[i])
        r = lib.orc_rochade_refine(plane.ctypes.data, w, h, one.ctypes.data, 1, 2, out.ctypes.data)
        assert r in (0, 1)
        if r:
            acc[i] = True
            rec[i] = out[0]
    return acc, rec


def check_points(O, plane, pts, rec, st, what, n=None):
    """One frame's records and statuses (the first n slots) against the oracle on `plane`.  -> the accepted mask."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts) if n is None else n
    pts, rec, st = pts[:n], rec[:n], st[:n]
    h, w = plane.shape
    acc, ref = oracle_points(O, plane, pts)
    out = outside_rule(pts, w, h)
    assert np.array_equal(st == OUTSIDE, out), "%s: OUTSIDE differs from the rule at %s" % (what, np.flatnonzero((st == OUTSIDE) != out)[:8])
    assert np.array_equal(st == REFINED, acc), "%s: refined set differs from the oracle's at %s" % (what, np.flatnonzero((st == REFINED) != acc)[:8])
    assert np.isin(st, (REFINED, OUTSIDE, NOT_SADDLE, MOVED)).all(), what
    for f in ("x", "y", "k"):
        assert bits_equal(rec[f][acc], ref[f][acc]), "%s: field %s differs" % (what, f)
    for f in ("theta", "phi"):
        if acc.any():
            assert np.max(np.abs(rec[f][acc] - ref[f][acc])) <= ANGLE_TOL_DEG, (what, f)
    assert not np.frombuffer(rec[~acc].tobytes(), np.uint8).any(), what + ": a rejected point's record is not zero"
    return acc


def gt_corners(gt, w, h, margin=6.0):
    g = np.unique(np.concatenate([gt[t] for t in gt]).round(6), axis=0)
    return g[(g[:, 0] > margin) & (g[:, 0] < w - margin) & (g[:, 1] > margin) & (g[:, 1] < h - margin)]


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def run(det, frames, pts, image="blurred", format=None, counts=None):
    """Internal result buffers + fetch -> (records [N, P], status [N, P])."""
    det.refine_points_enqueue(frames, dev(np.asarray(pts, np.float32)), counts=counts, image=image, format=format)
    return det.refine_points_fetch()


def run_raw(det, dptr, n, w, h, row_stride, frame_stride, fmt, image, pts):
    """The same on a raw device address with any strides (what the tensor form cannot say)."""
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    p = dev(np.asarray(pts, np.float32))
    assert p.dim() == 3 and p.shape[0] == n
    det._follow_torch_stream()
    det._check(det._lib.agx_refine_points_enqueue(det._h, dptr, n, w, h, row_stride, frame_stride, fmt, image, p.data_ptr(), p.shape[1],
                                                  None, None, None))
    rec = np.zeros((n, p.shape[1]), SADDLE_DTYPE)
    st = np.full((n, p.shape[1]), UNWRITTEN, np.uint32)
    det._check(det._lib.agx_refine_points_fetch(det._h, rec.ctypes.data, st.ctypes.data))
    return rec, st


@pytest.fixture(scope="module")
def case1(oracle):
    """3 L8 frames of 320 x 200; per frame the ground-truth corners inside a 6 px margin jittered by up to a pixel, then
    uniform points over [-3, W+3] x [-3, H+3]: 544 points per frame.  The oracle's blur planes, computed once."""
    synth = synth_module()
    rng = np.random.default_rng(1)
    frames, pts, blur = [], [], []
    P = 544
    for f in range(3):
        fr, gt = synth.render_frame(f, W, H)
        g = gt_corners(gt, W, H)
        assert (len(g) == 144) if f == 0 else (100 <= len(g) <= 144)
        jit = g + rng.uniform(-1, 1, g.shape)
        n_rnd = P - len(g)
        rnd = np.stack([rng.uniform(-3, W + 3, n_rnd), rng.uniform(-3, H + 3, n_rnd)], 1)
        frames.append(fr.numpy())
        pts.append(np.concatenate([jit, rnd]).astype(np.float32))
        blur.append(oracle.gaussian_blur_f32(oracle.luma_f32(frames[-1])))
    return {"frames": np.stack(frames), "pts": np.stack(pts), "blur": blur, "n_gt": 144}


@pytest.fixture(scope="module")
def case1_gpu(det, case1):
    """Case 1's batch through the internal buffers, run once: what the other modes and planes must reproduce byte for byte."""
    rec, st = run(det, dev(case1["frames"]), case1["pts"])
    return rec.copy(), st.copy()


# ---- 1. L8 batch ----------------------------------------------------------------------------------------------------------
def test_l8_batch_equals_the_oracle_point_by_point(oracle, case1, case1_gpu):
    rec, st = case1_gpu
    seen = set()
    for f in range(3):
        acc = check_points(oracle, case1["blur"][f], case1["pts"][f], rec[f], st[f], "frame %d" % f)
        seen |= set(int(s) for s in st[f])
        if f == 0:  # jittered corners and random points are both accepted and refused
            n = case1["n_gt"]
            assert 0 < acc[:n].sum() < n and 0 < acc[n:].sum() < len(acc) - n, (acc[:n].sum(), acc[n:].sum())
    assert seen == {REFINED, OUTSIDE, NOT_SADDLE, MOVED}, seen


def test_caller_owned_buffers_ragged_counts_and_padding(det, case1, case1_gpu):
    """Both result modes give the same bytes; with per-frame counts (P, 17, 0) the slots at or beyond a frame's count keep the
    0xFF fill, in the caller's device buffers and in the fetch's host arrays; the test's padding around its device buffers
    stays intact."""
    import torch
    rec0, st0 = case1_gpu
    frames, pts = dev(case1["frames"]), dev(case1["pts"])
    N, P, PAD = 3, rec0.shape[1], 256
    for counts in (None, (P, 17, 0)):
        big_out = torch.full((PAD + N * P * 5 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
        big_out.view(torch.int32).fill_(-1)
        big_st = torch.full((PAD + N * P + PAD,), -1, dtype=torch.int32, device="cuda")
        out = big_out[PAD:PAD + N * P * 5].view(N, P, 5)
        status = big_st[PAD:PAD + N * P].view(N, P)
        cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
        det.refine_points_enqueue(frames, pts, counts=cnt, out=out, status=status)
        got_out, got_st = det.refine_points_fetch()
        assert got_out is out and got_st is status
        raw_out = big_out.cpu().numpy().view(np.uint32)
        raw_st = big_st.cpu().numpy().view(np.uint32)
        assert (raw_out[:PAD] == UNWRITTEN).all() and (raw_out[-PAD:] == UNWRITTEN).all(), "padding around the records"
        assert (raw_st[:PAD] == UNWRITTEN).all() and (raw_st[-PAD:] == UNWRITTEN).all(), "padding around the statuses"
        o = raw_out[PAD:-PAD].reshape(N, P, 5)
        s = raw_st[PAD:-PAD].reshape(N, P)
        # the internal buffers with the same counts
        rec_i, st_i = run(det, frames, case1["pts"], counts=cnt)
        for f in range(N):
            n = P if counts is None else counts[f]
            assert o[f, :n].tobytes() == rec0[f, :n].tobytes() and s[f, :n].tobytes() == st0[f, :n].tobytes(), (counts, f)
            assert (o[f, n:] == UNWRITTEN).all() and (s[f, n:] == UNWRITTEN).all(), (counts, f, "slots beyond the count were written")
            assert rec_i[f, :n].tobytes() == rec0[f, :n].tobytes() and st_i[f, :n].tobytes() == st0[f, :n].tobytes(), (counts, f)
            assert (st_i[f, n:] == UNWRITTEN).all() and not np.frombuffer(rec_i[f, n:].tobytes(), np.uint8).any(), (counts, f)
    # a count beyond points_per_frame means points_per_frame
    cnt = torch.tensor([P + 5, P, 1 << 30], dtype=torch.int32, device="cuda")
    rec_i, st_i = run(det, frames, case1["pts"], counts=cnt)
    assert rec_i.tobytes() == rec0.tobytes() and st_i.tobytes() == st0.tobytes()


# ---- 2. unaligned width and pitch -----------------------------------------------------------------------------------------
def test_unaligned_width_and_row_stride(det, oracle):
    """203 x 131 with a row stride of 207 bytes: the blur kernel's unaligned form in front, a blur plane whose rows are not on
    the 16-byte grid behind it (the kernel's single-float loads)."""
    import torch
    synth = synth_module()
    w, h, stride = 203, 131, 207
    fr, gt = synth.render_frame(5, w, h)
    img = fr.numpy()
    g = gt_corners(gt, w, h).astype(np.float32)
    assert len(g) == 144
    buf = np.full(h * stride + 64, 0xC3, np.uint8)
    buf[:h * stride].reshape(h, stride)[:, :w] = img
    d_buf = torch.from_numpy(buf).cuda()
    rec, st = run_raw(det, d_buf.data_ptr(), 1, w, h, stride, h * stride, L8, BLURRED, g[None])
    blur = oracle.gaussian_blur_f32(oracle.luma_f32(img))
    acc = check_points(oracle, blur, g, rec[0], st[0], "203 x 131, stride 207")
    assert acc.sum() == 77, acc.sum()
    # the tight form of the same frame (width still off the grid)
    rec2, st2 = run(det, dev(img[None]), g[None])
    assert rec2.tobytes() == rec.tobytes() and st2.tobytes() == st.tobytes()


# ---- 3. other formats -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L16", "RGB8", "BGRA8", "LF32"])
def test_other_formats_in_blurred_mode(det, oracle, case1, name):
    """One 320 x 200 frame per format; the oracle's luma is that of the native base image (tests/test_gpu_formats.py: RGB8 for
    BGRA8), the caller's own plane for LF32."""
    from tests.test_gpu_formats import make
    rng = np.random.default_rng(31)
    grey = case1["frames"][0]
    pts = case1["pts"][0]
    if name == "LF32":
        px = oracle.luma_f32(grey)
        base, fmt = px, None
    elif name == "L16":
        px, base, _ = make("LA16", grey, rng)  # (its base: an L16 image with the low byte filled)
        px, fmt = base, None
    elif name == "RGB8":
        _, base, _ = make("BGR8", grey, rng)
        px, fmt = base, None
    else:
        px, base, _ = make("BGRA8", grey, rng)
        fmt = BGRA8
    blur = oracle.gaussian_blur_f32(oracle.luma_f32(base))
    rec, st = run(det, dev(px[None]), pts[None], format=fmt)
    acc = check_points(oracle, blur, pts, rec[0], st[0], name)
    assert acc.sum() > 50


# ---- 4. AGX_REFINE_PLANE --------------------------------------------------------------------------------------------------
def test_plane_mode_on_a_padded_plane_off_the_16_byte_grid(det, oracle, case1, case1_gpu):
    """The plane is the oracle's blur of frame 0, rows 3 floats longer than the image and the base 4 bytes off the 16-byte
    grid: the oracle's results, and the BLURRED results of case 1 for the same points in all five fields, bit for bit."""
    import torch
    blur, pts = case1["blur"][0], case1["pts"][0]
    pitch, off = W + 3, 1
    host = np.full(off + H * pitch + 8, np.float32(777.0), np.float32)
    host[off:off + H * pitch].reshape(H, pitch)[:, :W] = blur
    d_plane = torch.from_numpy(host).cuda()
    ptr = d_plane.data_ptr() + 4 * off
    assert d_plane.data_ptr() % 16 == 0 and ptr % 16 == 4
    rec, st = run_raw(det, ptr, 1, W, H, 4 * pitch, 4 * pitch * H, LF32, PLANE, pts[None])
    check_points(oracle, blur, pts, rec[0], st[0], "plane mode")
    assert rec[0].tobytes() == case1_gpu[0][0].tobytes() and st[0].tobytes() == case1_gpu[1][0].tobytes()
    # the tensor form: a tight plane
    rec2, st2 = run(det, dev(blur[None]), pts[None], image="plane")
    assert rec2.tobytes() == rec.tobytes() and st2.tobytes() == st.tobytes()


def test_plane_mode_on_constructed_planes(det, oracle):
    """64 x 64 planes with a known answer: a bilinear saddle at (31.25, 30.75) -- refined from (31, 31), moved too far from
    (33, 31) --, a paraboloid and an all-zero plane (not saddles)."""
    y, x = np.mgrid[0:64, 0:64].astype(np.float64)
    saddle = ((x - 31.25) * (y - 30.75) / 64).astype(np.float32)
    bowl = (((x - 31) ** 2 + (y - 31) ** 2) / 64).astype(np.float32)
    flat = np.zeros((64, 64), np.float32)
    planes = np.stack([saddle, saddle, bowl, flat])
    pts = np.array([[[31, 31]], [[33, 31]], [[31, 31]], [[31, 31]]], np.float32)
    rec, st = run(det, dev(planes), pts, image="plane")
    assert list(st[:, 0]) == [REFINED, MOVED, NOT_SADDLE, NOT_SADDLE], st
    assert abs(rec[0, 0]["x"] - 31.25) < 1e-3 and abs(rec[0, 0]["y"] - 30.75) < 1e-3, rec[0, 0]
    for f in range(4):
        check_points(oracle, planes[f], pts[f], rec[f], st[f], "constructed plane %d" % f)


# ---- 5. edges -------------------------------------------------------------------------------------------------------------
EDGE = [3.5, 3.49, None, None, float("nan"), float("inf"), float("-inf"), 1e20, -1e20, -0.0, 2147483648.0, -2147483904.0, 4294967296.0]


def edge_points():
    xs = [W - 5.0 if v is None and i == 2 else (W - 4.5 if v is None else v) for i, v in enumerate(EDGE)]
    ys = [H - 5.0 if v is None and i == 2 else (H - 4.5 if v is None else v) for i, v in enumerate(EDGE)]
    pts = [(x, 100.0) for x in xs] + [(160.0, y) for y in ys] + [(4.0, 4.0), (W - 5.0, H - 5.0), (float("nan"), float("nan"))]
    return np.array(pts, np.float32)


def test_edge_coordinates(det, oracle, case1):
    pts = edge_points()
    n = len(EDGE)
    want_out = [False, True, False, True] + [True] * (n - 4)
    assert list(outside_rule(pts, W, H)) == want_out + want_out + [False, False, True]
    for image, frames, plane in (("blurred", case1["frames"][:1], case1["blur"][0]), ("plane", case1["blur"][0][None], case1["blur"][0])):
        rec, st = run(det, dev(frames), pts[None], image=image)
        check_points(oracle, plane, pts, rec[0], st[0], "edges, " + image)


def test_a_frame_smaller_than_the_window_has_only_outside_points(det):
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-2, 10, (60, 2)), [[4, 4], [3.5, 3.5], [0, 0], [np.nan, 1]]]).astype(np.float32)
    for w, h in ((8, 8), (8, 40), (40, 8), (1, 1)):
        img = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
        for image, frames in (("blurred", img), ("plane", img.astype(np.float32) / 255)):
            rec, st = run(det, dev(frames), pts[None], image=image)
            assert (st == OUTSIDE).all(), (w, h, image)
            assert not np.frombuffer(rec.tobytes(), np.uint8).any()


def test_windows_at_the_first_and_last_pixel_stay_inside_the_buffers(oracle, case1, case1_gpu):
    """A handle with guard bytes around every buffer (tests/test_gpu_memory_safety.py): points (4, 4) and (W-5, H-5), whose
    windows touch the blur plane's first and last pixel, with case 1's points; a plane that ends with the allocation."""
    import aprilgrid_rs_amd as A
    os.environ["AGX_REDZONE_BYTES"] = str(1 << 16)
    try:
        d = A.TagDetector("t36h11", None, device=0)
    finally:
        del os.environ["AGX_REDZONE_BYTES"]
    try:
        corners = np.array([[4, 4], [W - 5, H - 5], [4, H - 5], [W - 5, 4]], np.float32)
        pts = np.concatenate([corners, case1["pts"][0]])
        for frames, image, plane in ((case1["frames"][:1], "blurred", case1["blur"][0]), (case1["blur"][0][None], "plane", case1["blur"][0])):
            rec, st = run(d, dev(frames), pts[None], image=image)
            check_points(oracle, plane, pts, rec[0], st[0], "guarded handle, " + image)
            assert (st[0, :4] != OUTSIDE).all()
            assert rec[0, 4:].tobytes() == case1_gpu[0][0].tobytes()
            r = d.debug_fetch(0, "redzones")
            assert r["damaged_bytes"] == 0, (image, r)
            assert r["buffers"] >= (20 if image == "blurred" else 2), (image, r)  # (the internal result buffers are guarded too)
        # width off the 16-byte grid
        img = np.ascontiguousarray(case1["frames"][:1, :131, :203])
        blur = oracle.gaussian_blur_f32(oracle.luma_f32(img[0]))
        c2 = np.array([[4, 4], [203 - 5, 131 - 5]], np.float32)
        rec, st = run(d, dev(img), c2[None])
        check_points(oracle, blur, c2, rec[0], st[0], "guarded handle, 203 x 131")
        assert d.debug_fetch(0, "redzones")["damaged_bytes"] == 0
    finally:
        d.close()


# ---- 6. agreement with the chain ------------------------------------------------------------------------------------------
def test_the_chains_centroids_refine_to_the_chains_records(det, case1):
    """A saddle batch on frame 0, then its cluster centroids as points: the refined records, in order, are the chain's own
    unfiltered refinement."""
    frames = dev(case1["frames"][:1])
    det.saddles_batch_enqueue(frames)
    det.saddles_batch_fetch()
    centers = det.debug_fetch(0, "centers")
    refined = det.debug_fetch(0, "refined")
    assert len(centers) > 100 and 0 < len(refined) <= len(centers)
    pts = np.stack([centers["cx"], centers["cy"]], 1).astype(np.float32)
    rec, st = run(det, frames, pts[None])
    got = rec[0][st[0] == REFINED]
    check_saddles(got, refined, "centroids as points")


# ---- 7. state and arguments -----------------------------------------------------------------------------------------------
def test_batches_of_both_kinds_alternate_on_one_handle(oracle, case1, case1_gpu):
    """The counter hand-over: the blur kernel of a refine batch leaves a counter set nothing clears; a saddle batch after it,
    and a refine batch after that, still give the oracle's results -- several times over, so that both counter sets take
    part."""
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    try:
        frames = dev(case1["frames"])
        refs = [oracle.refined_saddle_points(case1["frames"][f]) for f in range(3)]
        for rounds in range(3):
            rec, st = run(d, frames, case1["pts"])
            assert rec.tobytes() == case1_gpu[0].tobytes() and st.tobytes() == case1_gpu[1].tobytes(), rounds
            if rounds == 1:  # two refine batches in a row
                rec, st = run(d, frames, case1["pts"])
                assert rec.tobytes() == case1_gpu[0].tobytes(), rounds
            d.saddles_batch_enqueue(frames)
            res, status = d.saddles_batch_fetch()
            assert (status == 0).all()
            for f in range(3):
                check_saddles(res[f], refs[f], "saddle batch after a refine batch, round %d frame %d" % (rounds, f))
    finally:
        d.close()


def test_state_rules(det, case1):
    import torch
    lib, h = det._lib, det._h
    frames, pts = dev(case1["frames"]), dev(case1["pts"])
    n, P = 3, pts.shape[1]
    counts = np.zeros(n, np.uint32)
    status = np.zeros(n, np.int32)
    rec = np.zeros((n, P, 5), np.float32)
    st = np.zeros((n, P), np.uint32)
    det.refine_points_enqueue(frames, pts)
    assert lib.agx_saddles_batch_fetch(h, None, 0, counts.ctypes.data, status.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_detect_batch_fetch(h, None, counts.ctypes.data, status.ctypes.data, 1) == AGX_ERR_STATE
    assert lib.agx_refine_points_fetch(h, None, st.ctypes.data) == AGX_ERR_ARG  # (internal buffers need host arrays; still in flight)
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_OK
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE  # a second fetch
    det._refine = None
    # a saddle batch, then a detect batch, in flight: not this fetch's
    det.saddles_batch_enqueue(frames)
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    res, status2 = det.saddles_batch_fetch()
    assert (status2 == 0).all() and len(res[0]) > 50  # (and the saddle batch is still there)
    det.detect_batch_enqueue(frames, cap=128)
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    tags = det.detect_batch_fetch()
    assert isinstance(tags, list) and len(tags) == 3
    # a later enqueue of another kind replaces a refine batch
    det.refine_points_enqueue(frames, pts)
    det.saddles_batch_enqueue(frames)
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    det.saddles_batch_fetch()
    # caller-owned buffers: the fetch takes NULL host arrays and only waits
    out = torch.zeros((n, P, 5), dtype=torch.float32, device="cuda")
    dst = torch.full((n, P), -1, dtype=torch.int32, device="cuda")
    det.refine_points_enqueue(frames, pts, out=out, status=dst)
    det._refine = None
    assert lib.agx_refine_points_fetch(h, None, None) == AGX_OK
    assert lib.agx_refine_points_fetch(h, None, None) == AGX_ERR_STATE
    assert int((dst == -1).sum()) == 0


def test_argument_rules(det, case1):
    import torch
    lib, h = det._lib, det._h
    frames, pts = dev(case1["frames"]), dev(case1["pts"])
    plane = dev(case1["blur"][0][None])
    n, P = 3, pts.shape[1]
    out = torch.zeros((n, P, 5), dtype=torch.float32, device="cuda")
    dst = torch.zeros((n, P), dtype=torch.int32, device="cuda")
    f, p, o, s = frames.data_ptr(), pts.data_ptr(), out.data_ptr(), dst.data_ptr()
    enq = lambda *a: lib.agx_refine_points_enqueue(h, *a)
    assert enq(None, n, W, H, W, W * H, L8, BLURRED, p, P, None, None, None) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, BLURRED, None, P, None, None, None) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, BLURRED, p, 0, None, None, None) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, BLURRED, p, P, None, o, None) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, BLURRED, p, P, None, None, s) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, 2, p, P, None, None, None) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, -1, p, P, None, None, None) == AGX_ERR_ARG
    assert enq(f, n, W, H, W, W * H, L8, PLANE, p, P, None, None, None) == AGX_ERR_FORMAT
    assert enq(f, n, W, H, W, W * H, 12, BLURRED, p, P, None, None, None) == AGX_ERR_FORMAT
    assert enq(plane.data_ptr(), 1, W, H, 4 * W + 2, 0, LF32, PLANE, p, P, None, None, None) == AGX_ERR_ARG  # stride not a multiple of 4
    rec = np.zeros((n, P, 5), np.float32)
    st = np.zeros((n, P), np.uint32)
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE  # none of them left a batch
    import aprilgrid_rs_amd as A
    with pytest.raises(A.AgxError) as e:
        det.refine_points_enqueue(frames, pts, image="sharpened")
    assert e.value.status == AGX_ERR_ARG
    with pytest.raises(A.AgxError) as e:
        det.refine_points_fetch()
    assert e.value.status == AGX_ERR_STATE


def test_single_frame_host_form_equals_the_batch_form(det, oracle, case1, case1_gpu):
    """agx_rochade_refine on a host image: the batch form's records and statuses, and *n_refined = the oracle's return value
    for the whole list of points inside the image."""
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    img, pts, blur = case1["frames"][0], case1["pts"][0], case1["blur"][0]
    rec, st = det.rochade_refine(img, pts)
    assert rec.tobytes() == case1_gpu[0][0].tobytes() and st.tobytes() == case1_gpu[1][0].tobytes()
    inside = np.ascontiguousarray(pts[~outside_rule(pts, W, H)])
    whole = np.zeros(len(inside), oracle.SADDLE_DTYPE)
    n_ref = oracle.lib().orc_rochade_refine(blur.ctypes.data, W, H, inside.ctypes.data, len(inside), 2, whole.ctypes.data)
    n = C.c_uint32(12345)
    out = np.zeros(len(pts), SADDLE_DTYPE)
    status = np.zeros(len(pts), np.uint32)
    assert det._lib.agx_rochade_refine(det._h, img.ctypes.data, W, H, W, L8, BLURRED, pts.ctypes.data, len(pts), out.ctypes.data,
                                       status.ctypes.data, C.byref(n)) == AGX_OK
    assert n.value == n_ref == int((status == REFINED).sum())
    # the reference's Vec<Saddle>: the refined records in input order
    check_saddles(out[status == REFINED], whole[:n_ref], "Vec<Saddle>")
    # the plane form on the host, a padded row stride; no points: an empty Vec
    wide = np.zeros((H, W + 5), np.float32)
    wide[:, :W] = blur
    assert det._lib.agx_rochade_refine(det._h, wide.ctypes.data, W, H, 4 * (W + 5), LF32, PLANE, pts.ctypes.data, len(pts), out.ctypes.data,
                                       status.ctypes.data, C.byref(n)) == AGX_OK
    assert out.tobytes() == case1_gpu[0][0].tobytes() and status.tobytes() == case1_gpu[1][0].tobytes()
    rec_p, st_p = det.rochade_refine(blur, pts, image="plane")
    assert rec_p.tobytes() == out.tobytes() and st_p.tobytes() == status.tobytes()
    assert det._lib.agx_rochade_refine(det._h, img.ctypes.data, W, H, W, L8, BLURRED, None, 0, None, None, C.byref(n)) == AGX_OK and n.value == 0
    assert det._lib.agx_rochade_refine(det._h, img.ctypes.data, W, H, W, L8, PLANE, pts.ctypes.data, len(pts), out.ctypes.data,
                                       status.ctypes.data, C.byref(n)) == AGX_ERR_FORMAT
