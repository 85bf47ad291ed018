"""rochade_refine of caller-given points at half_size_patch 1 .. 4 (agx_refine_points_enqueue_h, agx_rochade_refine_h; reference
src/detector.rs:194-361) against the oracle's orc_rochade_refine(.., half, ..), one point per call.  The recipe and the helpers
are tests/test_gpu_refine_points.py's, restated with a `half` argument: per refined point x, y and k are the oracle's bit for
bit and theta, phi within tests/util.ANGLE_TOL_DEG; the refined set is exactly the oracle's accepted set; AGX_POINT_OUTSIDE is
exactly the header's rule at that half, computed here in Python (the oracle is never asked about such a point); a rejected
point's record is zero.

The inputs (seed 1, 3 frames of 320 x 200, the corners inside a 10 px margin jittered by up to a pixel + uniform random points,
544 per frame): on frame 0 at sigma 1.5 the oracle accepts 92 / 103 / 111 / 76 of the 144 jittered corners and 26 / 21 / 17 /
19 of the 400 random points at half 1 / 2 / 3 / 4 -- both kinds are accepted and refused at every half."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import ANGLE_TOL_DEG, bits_equal, check_saddles, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
REFINED, OUTSIDE, NOT_SADDLE, MOVED = 0, 1, 2, 3
BLURRED, PLANE = 0, 1
L8, LF32 = 0, 3
W, H = 320, 200
UNWRITTEN = 0xFFFFFFFF
HALVES = (1, 2, 3, 4)


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


def outside_rule(pts, w, h, half):
    """AGX_POINT_OUTSIDE unless both coordinates are finite, roundf(x) in [2 half, w-1-2 half] and roundf(y) in
    [2 half, h-1-2 half]."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    rx, ry = roundf(pts[:, 0]), roundf(pts[:, 1])
    m = 2 * half
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(pts).all(axis=1) & (rx >= m) & (rx <= w - 1 - m) & (ry >= m) & (ry <= h - 1 - m)
    return ~inside


def oracle_points(O, plane, pts, half):
    """-> (accepted [n] bool, records [n] SADDLE_DTYPE) of orc_rochade_refine(plane, ..., half), one point per call; points the
    rule above puts outside are not handed to it."""
    plane = np.ascontiguousarray(plane, np.float32)
    h, w = plane.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    acc = np.zeros(len(pts), bool)
    rec = np.zeros(len(pts), O.SADDLE_DTYPE)
    out = np.zeros(1, O.SADDLE_DTYPE)
    lib = O.lib()
    for i in np.flatnonzero(~outside_rule(pts, w, h, half)):
        one = np.ascontiguousarray(pts[i])
        r = lib.orc_rochade_refine(plane.ctypes.data, w, h, one.ctypes.data, 1, half, out.ctypes.data)
        assert r in (0, 1)
        if r:
            acc[i] = True
            rec[i] = out[0]
    return acc, rec


def check_points(O, plane, pts, rec, st, half, what, n=None):
    """One frame's records and statuses (the first n slots) against the oracle on `plane`.  -> the accepted mask."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts) if n is None else n
    pts, rec, st = pts[:n], rec[:n], st[:n]
    h, w = plane.shape
    what = "%s, half %d" % (what, half)
    acc, ref = oracle_points(O, plane, pts, half)
    out = outside_rule(pts, w, h, half)
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


def gt_corners(gt, w, h, margin=10.0):
    g = np.unique(np.concatenate([gt[t] for t in gt]).round(6), axis=0)
    return g[(g[:, 0] > margin) & (g[:, 0] < w - margin) & (g[:, 1] > margin) & (g[:, 1] < h - margin)]


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(det, frames, pts, half, image="blurred", counts=None):
    """Internal result buffers + fetch -> (records [N, P], status [N, P])."""
    det.refine_points_enqueue(frames, dev(np.asarray(pts, np.float32)), counts=counts, image=image, half_size_patch=half)
    return det.refine_points_fetch()


def run_raw(det, dptr, n, w, h, row_stride, frame_stride, fmt, image, pts, half):
    """The same on a raw device address with any strides (what the tensor form cannot say)."""
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    p = dev(np.asarray(pts, np.float32))
    assert p.dim() == 3 and p.shape[0] == n
    det._follow_torch_stream()
    det._check(det._lib.agx_refine_points_enqueue_h(det._h, dptr, n, w, h, row_stride, frame_stride, fmt, image, p.data_ptr(), p.shape[1],
                                                    None, None, None, half))
    rec = np.zeros((n, p.shape[1]), SADDLE_DTYPE)
    st = np.full((n, p.shape[1]), UNWRITTEN, np.uint32)
    det._check(det._lib.agx_refine_points_fetch(det._h, rec.ctypes.data, st.ctypes.data))
    return rec, st


@pytest.fixture(scope="module")
def case1(oracle):
    """3 L8 frames of 320 x 200; per frame the ground-truth corners inside a 10 px margin jittered by up to a pixel, then
    uniform points over [-3, W+3] x [-3, H+3]: 544 points per frame.  The oracle's blur planes, computed once."""
    synth = synth_module()
    rng = np.random.default_rng(1)
    frames, pts, blur = [], [], []
    P = 544
    for f in range(3):
        fr, gt = synth.render_frame(f, W, H)
        g = gt_corners(gt, W, H)
        assert (len(g) == 144) if f == 0 else (60 <= len(g) <= 144)
        jit = g + rng.uniform(-1, 1, g.shape)
        n_rnd = P - len(g)
        rnd = np.stack([rng.uniform(-3, W + 3, n_rnd), rng.uniform(-3, H + 3, n_rnd)], 1)
        frames.append(fr.numpy())
        pts.append(np.concatenate([jit, rnd]).astype(np.float32))
        blur.append(oracle.gaussian_blur_f32(oracle.luma_f32(frames[-1])))
    return {"frames": np.stack(frames), "pts": np.stack(pts), "blur": blur, "n_gt": 144}


@pytest.fixture(scope="module")
def case1_gpu(det, case1):
    """Case 1's batch through the internal buffers at each half, run once: what the other modes must reproduce byte for byte."""
    frames = dev(case1["frames"])
    res = {}
    for half in HALVES:
        rec, st = run(det, frames, case1["pts"], half)
        res[half] = (rec.copy(), st.copy())
    return res


# ---- 1. L8 batch, BLURRED -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", HALVES)
def test_the_inputs_exercise_both_answers_by_the_oracle_alone(oracle, case1, half):
    """No device result is looked at: on frame 0 the oracle accepts and refuses jittered corners and random points alike."""
    acc, _ = oracle_points(oracle, case1["blur"][0], case1["pts"][0], half)
    n = case1["n_gt"]
    assert (int(acc[:n].sum()), int(acc[n:].sum())) == {1: (92, 26), 2: (103, 21), 3: (111, 17), 4: (76, 19)}[half]


@pytest.mark.parametrize("half", HALVES)
def test_l8_batch_equals_the_oracle_point_by_point(det, oracle, case1, case1_gpu, half):
    rec, st = case1_gpu[half]
    seen = set()
    for f in range(3):
        acc = check_points(oracle, case1["blur"][f], case1["pts"][f], rec[f], st[f], half, "frame %d" % f)
        seen |= set(int(s) for s in st[f])
        if f == 0:  # jittered corners and random points are both accepted and refused
            n = case1["n_gt"]
            assert 0 < acc[:n].sum() < n and 0 < acc[n:].sum() < len(acc) - n, (acc[:n].sum(), acc[n:].sum())
    assert seen == {REFINED, OUTSIDE, NOT_SADDLE, MOVED}, seen


def test_half_2_is_agx_refine_points_enqueue_on_either_kernel(det, case1, case1_gpu):
    """The _h entry at 2 gives agx_refine_points_enqueue's bytes and ran its kernel; under "refine_general_kernel" the same
    bytes come from the kernel of the other sizes."""
    frames = dev(case1["frames"])
    rec_h, st_h = case1_gpu[2]
    det.refine_points_enqueue(frames, dev(case1["pts"]))  # (the binding's default: 2)
    rec0, st0 = det.refine_points_fetch()
    assert det.get_option("last_refine_kernel") == 0
    from tests.test_gpu_refine_points import run_raw as run_raw_parent  # agx_refine_points_enqueue itself, without the parameter
    rec_p, st_p = run_raw_parent(det, frames.data_ptr(), 3, W, H, W, W * H, L8, BLURRED, case1["pts"])
    assert det.get_option("last_refine_kernel") == 0
    assert rec_p.tobytes() == rec_h.tobytes() == rec0.tobytes() and st_p.tobytes() == st_h.tobytes() == st0.tobytes()
    assert det.get_option("refine_general_kernel") == 0
    det.set_option("refine_general_kernel", 1)
    try:
        rec_g, st_g = run(det, frames, case1["pts"], 2)
        assert det.get_option("last_refine_kernel") == 1
        rec_pg, st_pg = run_raw_parent(det, frames.data_ptr(), 3, W, H, W, W * H, L8, BLURRED, case1["pts"])
        assert det.get_option("last_refine_kernel") == 1
    finally:
        det.set_option("refine_general_kernel", 0)
    assert rec_g.tobytes() == rec_h.tobytes() and st_g.tobytes() == st_h.tobytes()
    assert rec_pg.tobytes() == rec_h.tobytes() and st_pg.tobytes() == st_h.tobytes()
    run(det, frames, case1["pts"], 3)
    assert det.get_option("last_refine_kernel") == 1
    run(det, frames, case1["pts"], 2)
    assert det.get_option("last_refine_kernel") == 0


# ---- 2. AGX_REFINE_PLANE --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (1, 3, 4))
def test_plane_mode_on_a_padded_plane_off_the_16_byte_grid(det, oracle, case1, half):
    """A plane 317 wide (the left part of the oracle's blur of frame 0), rows 3 floats longer than that and the base 4 bytes
    off the 16-byte grid; the plane ends with its last row: nothing behind it belongs to the caller."""
    import torch
    w = 317
    plane = np.ascontiguousarray(case1["blur"][0][:, :w])
    pts = case1["pts"][0]
    pitch, off = w + 3, 1
    host = np.full(off + (H - 1) * pitch + w, np.float32(777.0), np.float32)
    for y in range(H):
        host[off + y * pitch:off + y * pitch + w] = plane[y]
    d_plane = torch.from_numpy(host).cuda()
    ptr = d_plane.data_ptr() + 4 * off
    assert d_plane.data_ptr() % 16 == 0 and ptr % 16 == 4
    rec, st = run_raw(det, ptr, 1, w, H, 4 * pitch, 4 * pitch * H, LF32, PLANE, pts[None], half)
    acc = check_points(oracle, plane, pts, rec[0], st[0], half, "plane mode, 317 wide")
    assert acc.sum() > 50
    # the tensor form: a tight plane
    rec2, st2 = run(det, dev(plane[None]), pts[None], half, image="plane")
    assert rec2.tobytes() == rec.tobytes() and st2.tobytes() == st.tobytes()


# ---- 3. result modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (1, 3, 4))
def test_caller_owned_buffers_ragged_counts_and_padding(det, case1, case1_gpu, half):
    """Both result modes give the same bytes; with per-frame counts (P, 17, 0) the slots at or beyond a frame's count keep the
    0xFF fill, in the caller's device buffers and in the fetch's host arrays; the padding around the buffers stays intact."""
    import torch
    rec0, st0 = case1_gpu[half]
    frames, pts = dev(case1["frames"]), dev(case1["pts"])
    N, P, PAD = 3, rec0.shape[1], 256
    for counts in (None, (P, 17, 0)):
        big_out = torch.full((PAD + N * P * 5 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
        big_out.view(torch.int32).fill_(-1)
        big_st = torch.full((PAD + N * P + PAD,), -1, dtype=torch.int32, device="cuda")
        out = big_out[PAD:PAD + N * P * 5].view(N, P, 5)
        status = big_st[PAD:PAD + N * P].view(N, P)
        cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
        det.refine_points_enqueue(frames, pts, counts=cnt, out=out, status=status, half_size_patch=half)
        got_out, got_st = det.refine_points_fetch()
        assert got_out is out and got_st is status
        raw_out = big_out.cpu().numpy().view(np.uint32)
        raw_st = big_st.cpu().numpy().view(np.uint32)
        assert (raw_out[:PAD] == UNWRITTEN).all() and (raw_out[-PAD:] == UNWRITTEN).all(), "padding around the records"
        assert (raw_st[:PAD] == UNWRITTEN).all() and (raw_st[-PAD:] == UNWRITTEN).all(), "padding around the statuses"
        o = raw_out[PAD:-PAD].reshape(N, P, 5)
        s = raw_st[PAD:-PAD].reshape(N, P)
        rec_i, st_i = run(det, frames, case1["pts"], half, counts=cnt)  # the internal buffers with the same counts
        for f in range(N):
            n = P if counts is None else counts[f]
            assert o[f, :n].tobytes() == rec0[f, :n].tobytes() and s[f, :n].tobytes() == st0[f, :n].tobytes(), (counts, f)
            assert (o[f, n:] == UNWRITTEN).all() and (s[f, n:] == UNWRITTEN).all(), (counts, f, "slots beyond the count were written")
            assert rec_i[f, :n].tobytes() == rec0[f, :n].tobytes() and st_i[f, :n].tobytes() == st0[f, :n].tobytes(), (counts, f)
            assert (st_i[f, n:] == UNWRITTEN).all() and not np.frombuffer(rec_i[f, n:].tobytes(), np.uint8).any(), (counts, f)


# ---- 4. edges -------------------------------------------------------------------------------------------------------------
def saddle_plane(w, h, half):
    """A plane with a bilinear saddle a quarter pixel off each of the four innermost-allowed points (2 half, 2 half) ..
    (w-1-2 half, h-1-2 half): f = (x - cx) (y - cy) / 16 with cx, cy the nearer of the two allowed extremes + 0.25 / - 0.25 --
    linear in x and in y over each point's whole window."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    m = 2 * half
    cx = np.where(x < w / 2, m, w - 1 - m) + 0.25
    cy = np.where(y < h / 2, m, h - 1 - m) - 0.25
    return ((x - cx) * (y - cy) / 16).astype(np.float32)


def edge_points(w, h, half):
    """-> (points, which of them must be REFINED on saddle_plane, which must be OUTSIDE)"""
    m = 2 * half
    x0, x1, y0, y1 = float(m), float(w - 1 - m), float(m), float(h - 1 - m)
    on = [(x0, y0), (x1, y0), (x0, y1), (x1, y1), (x0 - 0.5, y0 - 0.5), (x1 + 0.49, y1 + 0.49)]  # (roundf: half away from zero)
    off = [(x0 - 1, y0), (x0, y0 - 1), (x1 + 1, y1), (x1, y1 + 1), (x0 - 0.51, y0), (x1 + 0.5, y1)]
    bad = [(v, y0) for v in (float("nan"), float("inf"), float("-inf"), 3e9, -3e9)] + [(x0, v) for v in (float("nan"), float("inf"), float("-inf"), 3e9)]
    bad += [(float("nan"), float("nan"))]
    pts = np.array(on + off + bad, np.float32)
    return pts, np.arange(len(on)), np.arange(len(on), len(pts))


@pytest.mark.parametrize("half", HALVES)
def test_edge_coordinates(det, oracle, case1, half):
    w, h = 64, 48
    plane = saddle_plane(w, h, half)
    pts, on, off = edge_points(w, h, half)
    rule = outside_rule(pts, w, h, half)
    assert not rule[on].any() and rule[off].all()
    rec, st = run(det, dev(plane[None]), pts[None], half, image="plane")
    check_points(oracle, plane, pts, rec[0], st[0], half, "edges of a constructed plane")
    assert (st[0][on] == REFINED).all(), st[0][on]
    m = 2 * half
    assert abs(rec[0][0]["x"] - (m + 0.25)) < 1e-3 and abs(rec[0][0]["y"] - (m - 0.25)) < 1e-3, rec[0][0]
    assert abs(rec[0][3]["x"] - (w - 1 - m + 0.25)) < 1e-3 and abs(rec[0][3]["y"] - (h - 1 - m - 0.25)) < 1e-3, rec[0][3]
    assert (st[0][off] == OUTSIDE).all()
    # the same coordinates' rule on a frame's blur
    pts2, _, off2 = edge_points(W, H, half)
    rec, st = run(det, dev(case1["frames"][:1]), pts2[None], half)
    check_points(oracle, case1["blur"][0], pts2, rec[0], st[0], half, "edges of frame 0")
    assert (st[0][off2] == OUTSIDE).all()


def placement_points(w, h, half):
    """Rounded coordinates exactly at the first and last allowed value (inside), one beyond each (outside), the x.5 values that
    roundf takes away from zero onto either, and what no int can hold."""
    m = 2 * half
    xs = [m, w - 1 - m, m - 1, w - m, m - 0.5, m - 1.5, w - 1 - m + 0.5, w - 1 - m - 0.5, -0.5]
    ys = [m, h - 1 - m, m - 1, h - m, m - 0.5, m - 1.5, h - 1 - m + 0.5, h - 1 - m - 0.5, -0.5]
    bad = [float("nan"), float("inf"), float("-inf"), 2147483648.0, -2147483648.0]
    pts = [(vx, float(m)) for vx in xs + bad] + [(float(m), vy) for vy in ys + bad] + [(w - 1 - m, h - 1 - m), (w - m, h - m)]
    return np.array(pts, np.float32)


@pytest.mark.parametrize("half", HALVES)
def test_window_placement_on_the_smallest_plane_with_an_interior_at_half_4(det, oracle, half):
    """24 x 20: a 17 x 17 window still has 8 x 4 places.  Statuses and records are the oracle's at every half; at 2 the one-lane
    kernel and the sixteen-lane kernel decide every point alike, byte for byte."""
    w, h = 24, 20
    plane = saddle_plane(w, h, half)
    pts = placement_points(w, h, half)
    rule = outside_rule(pts, w, h, half)
    m = 2 * half
    assert list(rule[:9]) == [False, False, True, True, False, True, True, False, True] and rule[9:14].all(), "premise: the x sweep"
    assert list(rule[14:23]) == [False, False, True, True, False, True, True, False, True] and rule[23:28].all(), "premise: the y sweep"
    assert not rule[28] and rule[29]
    d_plane = dev(plane)  # (kept alive across the calls that are given its address)
    rec, st = run_raw(det, d_plane.data_ptr(), 1, w, h, 4 * w, 4 * w * h, LF32, PLANE, pts[None], half)
    assert det.get_option("last_refine_kernel") == (0 if half == 2 else 1)
    check_points(oracle, plane, pts, rec[0], st[0], half, "placement on 24 x 20")
    assert (st[0][rule] == OUTSIDE).all() and (st[0][~rule] != OUTSIDE).all()
    if half == 2:
        det.set_option("refine_general_kernel", 1)
        try:
            rec_g, st_g = run_raw(det, d_plane.data_ptr(), 1, w, h, 4 * w, 4 * w * h, LF32, PLANE, pts[None], half)
            assert det.get_option("last_refine_kernel") == 1
        finally:
            det.set_option("refine_general_kernel", 0)
        assert rec_g.tobytes() == rec.tobytes() and st_g.tobytes() == st.tobytes()


@pytest.mark.parametrize("half", HALVES)
def test_a_frame_smaller_than_the_window_has_only_outside_points(det, oracle, half):
    rng = np.random.default_rng(4)
    s = 4 * half
    pts = np.concatenate([rng.uniform(-2, s + 2, (60, 2)), [[2 * half, 2 * half], [s / 2 - 0.5, s / 2 - 0.5], [0, 0], [np.nan, 1]]]).astype(np.float32)
    for w, h in ((s, s), (s, 40), (40, s), (1, 1)):
        img = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
        for image, frames in (("blurred", img), ("plane", img.astype(np.float32) / 255)):
            rec, st = run(det, dev(frames), pts[None], half, image=image)
            assert (st == OUTSIDE).all(), (w, h, image)
            assert not np.frombuffer(rec.tobytes(), np.uint8).any()
    # one pixel more each way: exactly one window fits, the centre's
    plane = saddle_plane(s + 1, s + 1, half)
    rec, st = run(det, dev(plane[None]), pts[None], half, image="plane")
    check_points(oracle, plane, pts, rec[0], st[0], half, "a frame of one window")
    assert st[0][60] != OUTSIDE and (st[0] != OUTSIDE).sum() >= 1


def test_windows_at_the_first_and_last_pixel_stay_inside_the_buffers(oracle, case1, case1_gpu):
    """A handle with guard bytes around every buffer (tests/test_gpu_memory_safety.py): at half 4 the points (8, 8) and
    (W-9, H-9), whose 17 x 17 windows touch the plane's first and last pixel, with case 1's points -- on the handle's blur
    plane, and on a caller's plane that ends with its allocation."""
    import aprilgrid_rs_amd as A
    half = 4
    os.environ["AGX_REDZONE_BYTES"] = str(1 << 16)
    try:
        d = A.TagDetector("t36h11", None, device=0)
    finally:
        del os.environ["AGX_REDZONE_BYTES"]
    try:
        corners = np.array([[8, 8], [W - 9, H - 9], [8, H - 9], [W - 9, 8]], np.float32)
        pts = np.concatenate([corners, case1["pts"][0]])
        for frames, image, plane in ((case1["frames"][:1], "blurred", case1["blur"][0]), (case1["blur"][0][None], "plane", case1["blur"][0])):
            rec, st = run(d, dev(frames), pts[None], half, image=image)
            check_points(oracle, plane, pts, rec[0], st[0], half, "guarded handle, " + image)
            assert (st[0, :4] != OUTSIDE).all()
            assert rec[0, 4:].tobytes() == case1_gpu[half][0][0].tobytes()
            r = d.debug_fetch(0, "redzones")
            assert r["damaged_bytes"] == 0, (image, r)
            assert r["buffers"] >= (20 if image == "blurred" else 3), (image, r)  # (results and constants are guarded too)
        # width off the 16-byte grid
        img = np.ascontiguousarray(case1["frames"][:1, :131, :203])
        blur = oracle.gaussian_blur_f32(oracle.luma_f32(img[0]))
        c2 = np.array([[8, 8], [203 - 9, 131 - 9]], np.float32)
        rec, st = run(d, dev(img), c2[None], half)
        check_points(oracle, blur, c2, rec[0], st[0], half, "guarded handle, 203 x 131")
        assert d.debug_fetch(0, "redzones")["damaged_bytes"] == 0
    finally:
        d.close()


# ---- 5. the patch that goes with a wider blur -----------------------------------------------------------------------------
def test_sigma_3_with_half_4_on_a_640_x_400_frame(oracle):
    """set_blur_sigma(3.0) and half 4 in BLURRED mode against the oracle's sigma-3 blur; the oracle accepts 123 of the 144
    jittered corners."""
    import aprilgrid_rs_amd as A
    synth = synth_module()
    w, h = 640, 400
    fr, gt = synth.render_frame(0, w, h)
    img = fr.numpy()
    g = gt_corners(gt, w, h)
    assert len(g) == 144
    rng = np.random.default_rng(1)
    pts = np.concatenate([g + rng.uniform(-1, 1, g.shape),
                          np.stack([rng.uniform(-3, w + 3, 400), rng.uniform(-3, h + 3, 400)], 1)]).astype(np.float32)
    blur = oracle.gaussian_blur_f32(oracle.luma_f32(img), 3.0)
    d = A.TagDetector("t36h11", None, device=0)
    try:
        d.set_blur_sigma(3.0)
        rec, st = run(d, dev(img[None]), pts[None], 4)
        assert d.get_option("last_refine_kernel") == 1
        acc = check_points(oracle, blur, pts, rec[0], st[0], 4, "sigma 3")
        assert acc[:144].sum() == 123, acc[:144].sum()
    finally:
        d.close()


# ---- 6. host form, state and arguments ------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (1, 3, 4))
def test_single_frame_host_form_equals_the_batch_form(det, oracle, case1, case1_gpu, half):
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    img, pts, blur = case1["frames"][0], case1["pts"][0], case1["blur"][0]
    rec, st = det.rochade_refine(img, pts, half_size_patch=half)
    assert rec.tobytes() == case1_gpu[half][0][0].tobytes() and st.tobytes() == case1_gpu[half][1][0].tobytes()
    inside = np.ascontiguousarray(pts[~outside_rule(pts, W, H, half)])
    whole = np.zeros(len(inside), oracle.SADDLE_DTYPE)
    n_ref = oracle.lib().orc_rochade_refine(blur.ctypes.data, W, H, inside.ctypes.data, len(inside), half, whole.ctypes.data)
    n = C.c_uint32(12345)
    out = np.zeros(len(pts), SADDLE_DTYPE)
    status = np.zeros(len(pts), np.uint32)
    assert det._lib.agx_rochade_refine_h(det._h, img.ctypes.data, W, H, W, L8, BLURRED, pts.ctypes.data, len(pts), out.ctypes.data,
                                         status.ctypes.data, C.byref(n), half) == AGX_OK
    assert n.value == n_ref == int((status == REFINED).sum())
    check_saddles(out[status == REFINED], whole[:n_ref], "Vec<Saddle>, half %d" % half)  # the refined records in input order
    rec_p, st_p = det.rochade_refine(blur, pts, image="plane", half_size_patch=half)
    assert rec_p.tobytes() == out.tobytes() and st_p.tobytes() == status.tobytes()
    for bad in (0, 5):
        assert det._lib.agx_rochade_refine_h(det._h, img.ctypes.data, W, H, W, L8, BLURRED, pts.ctypes.data, len(pts), out.ctypes.data,
                                             status.ctypes.data, C.byref(n), bad) == AGX_ERR_ARG


def test_a_bad_half_leaves_the_batch_in_flight_and_halves_alternate(det, case1, case1_gpu):
    from aprilgrid_rs_amd.detector import SADDLE_DTYPE
    lib, h = det._lib, det._h
    frames, pts = dev(case1["frames"]), dev(case1["pts"])
    n, P = 3, pts.shape[1]
    f, p = frames.data_ptr(), pts.data_ptr()
    det._follow_torch_stream(frames)
    assert lib.agx_refine_points_enqueue_h(h, f, n, W, H, W, W * H, L8, BLURRED, p, P, None, None, None, 3) == AGX_OK
    for bad in (0, 5, -1, 1 << 20):
        assert lib.agx_refine_points_enqueue_h(h, f, n, W, H, W, W * H, L8, BLURRED, p, P, None, None, None, bad) == AGX_ERR_ARG
    rec = np.zeros((n, P), SADDLE_DTYPE)
    st = np.full((n, P), UNWRITTEN, np.uint32)
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_OK  # the batch at 3 is still there
    assert rec.tobytes() == case1_gpu[3][0].tobytes() and st.tobytes() == case1_gpu[3][1].tobytes()
    assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    for bad in (0, 5):  # and with nothing in flight nothing is left behind
        assert lib.agx_refine_points_enqueue_h(h, f, n, W, H, W, W * H, L8, BLURRED, p, P, None, None, None, bad) == AGX_ERR_ARG
        assert lib.agx_refine_points_fetch(h, rec.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    det._refine = None
    # every batch its own half, on one handle; a batch enqueued over another replaces it
    for half in (4, 1, 2, 3, 1, 4, 2):
        r, s = run(det, frames, case1["pts"], half)
        assert r.tobytes() == case1_gpu[half][0].tobytes() and s.tobytes() == case1_gpu[half][1].tobytes(), half
    det.refine_points_enqueue(frames, pts, half_size_patch=4)
    det.refine_points_enqueue(frames, pts, half_size_patch=1)
    r, s = det.refine_points_fetch()
    assert r.tobytes() == case1_gpu[1][0].tobytes() and s.tobytes() == case1_gpu[1][1].tobytes()
