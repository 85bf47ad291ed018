"""k_refine_windows (agx_refine_windows_enqueue) against the entry it restates: every record and status word must equal, byte for
byte, what refine_points_enqueue(.., image="blurred", half_size_patch=h) -- the front end, the blur plane and k_refine_points /
k_refine_patch -- writes for the same full-resolution points on the same frames.  The reference is that existing entry, never
the new kernel.

Frames 5x5, 9x9, 17x23 and 67x45 (on the small ones every clamp region of the blur overlaps), L8, L16 and LF32, tight and
padded, 1 and 3 frames; half_size_patch 1 .. 4 at sigma 0.8, 1.5, 3.0 and 8.0 (radius 2, 3, 6, 16).  The points: every pixel
of the frame (all border cases), every pixel centre moved by a half (rounding), NaN, +-inf and +-1e10, points beyond the frame;
as [N,P,2] points and as [N,P,5] records (strides 8 and 20); counts shorter than the row; status_in with non-zero words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = ((5, 5), (9, 9), (17, 23), (67, 45))  # (W, H)
SIGMAS = (0.8, 1.5, 3.0, 8.0)
HALVES = (1, 2, 3, 4)
FORMATS = ("L8", "L16", "LF32")
UNWRITTEN = -1  # 0xFFFFFFFF


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def make_frames(n, w, h, fmt, seed):
    """A noisy chessboard of 6 px squares, shifted per frame: saddles, edges and flat areas -> numpy [n, h, w] of the format."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for f in range(n):
        board = (((x + 2 * f) // 6 + (y + f) // 6) & 1) * 170.0 + 40.0 + rng.normal(0.0, 6.0, (h, w))
        out.append(np.clip(board, 0, 255))
    a = np.stack(out)
    if fmt == "L8":
        return a.astype(np.uint8)
    if fmt == "L16":
        return (a * 257.0).astype(np.uint16)
    return (a / 255.0).astype(np.float32)


def make_points(n, w, h, seed):
    """-> float32 [n, P, 2]: every pixel (at most 400 of them), the same moved by (0.5, 0.5) and (-0.5, 0.5), random points in and
    around the frame, and the values that must be refused before anything is read."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([x.ravel(), y.ravel()], axis=1).astype(np.float32)
    if len(px) > 400:
        px = px[rng.choice(len(px), 400, replace=False)]
    special = np.array([[np.nan, 3.0], [3.0, np.nan], [np.inf, 2.0], [2.0, -np.inf], [1e10, 4.0], [4.0, -1e10], [-0.5, -0.5],
                        [w - 0.5, h - 0.5], [w + 3.0, 1.0], [2.0 ** 31, 2.0 ** 31]], np.float32)
    frames = []
    for f in range(n):
        rnd = rng.uniform(-3.0, max(w, h) + 3.0, (64, 2)).astype(np.float32)
        frames.append(np.concatenate([px, px + np.float32(0.5), px + np.array([-0.5, 0.5], np.float32), rnd, special]))
    return np.stack(frames)


def to_device(a):
    import torch
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def padded(t, row_pad, frame_pad):
    """the same frames as a view with row_pad pixels behind every row and frame_pad rows behind every frame"""
    import torch
    n, h, w = t.shape
    big = torch.full((n, h + frame_pad, w + row_pad), 77, dtype=t.dtype, device=t.device)
    big[:, :h, :w] = t
    return big[:, :h, :w]


def reference(det, frames, pts, counts, half):
    """the existing entry on contiguous frames and [N,P,2] points -> (records float32 [N,P,5], status int32 [N,P]) on the host;
    slots it did not write keep NaN / UNWRITTEN"""
    import torch
    n, p = pts.shape[0], pts.shape[1]
    out = torch.full((n, p, 5), float("nan"), dtype=torch.float32, device="cuda:0")
    st = torch.full((n, p), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    det.refine_points_enqueue(frames.contiguous(), pts.contiguous(), counts=counts, out=out, status=st, image="blurred", half_size_patch=half)
    det.refine_points_fetch()
    return out.cpu().numpy(), st.cpu().numpy()


def windows(det, frames, points, counts, status_in, half, factor=1):
    import torch
    n, p = points.shape[0], points.shape[1]
    out = torch.full((n, p, 5), float("nan"), dtype=torch.float32, device="cuda:0")
    st = torch.full((n, p), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    det.refine_windows_enqueue(frames, points, out, st, counts=counts, status_in=status_in, factor=factor, half_size_patch=half)
    det.sync()
    return out.cpu().numpy(), st.cpu().numpy()


def same_bytes(got, ref, what):
    (g_rec, g_st), (r_rec, r_st) = got, ref
    bad = np.flatnonzero((g_st != r_st).ravel() | (g_rec.view(np.uint32) != r_rec.view(np.uint32)).any(axis=2).ravel())
    assert bad.size == 0, "%s: %d slots differ, first %d: status %d / %d, record %s / %s" % (
        what, bad.size, bad[0], g_st.ravel()[bad[0]], r_st.ravel()[bad[0]], g_rec.reshape(-1, 5)[bad[0]], r_rec.reshape(-1, 5)[bad[0]])


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_bytes_equal_the_blurred_entry(det, sigma, half):
    import torch
    det.set_blur_sigma(sigma)
    refined = 0
    for k, (w, h) in enumerate(FRAMES):
        for fmt in FORMATS:
            what = "%dx%d %s sigma %g half %d" % (w, h, fmt, sigma, half)
            # one tight frame, [N,P,2] points, no counts
            frames, pts = to_device(make_frames(1, w, h, fmt, 10 + k)), to_device(make_points(1, w, h, 20 + k))
            ref = reference(det, frames, pts, None, half)
            same_bytes(windows(det, frames, pts, None, None, half), ref, what + ", 1 frame")
            refined += int((ref[1] == 0).sum())
            # three padded frames, the points as the head of [N,P,5] records, counts shorter than the row, status_in
            frames, pts_h = to_device(make_frames(3, w, h, fmt, 30 + k)), make_points(3, w, h, 40 + k)
            p = pts_h.shape[1]
            counts = torch.tensor([p, p - 7, 3], dtype=torch.int32, device="cuda:0")
            pts = to_device(pts_h)
            ref_rec, ref_st = reference(det, frames, pts, counts, half)
            records = torch.full((3, p, 5), 123.0, dtype=torch.float32, device="cuda:0")
            records[:, :, :2] = pts
            same_bytes(windows(det, padded(frames, 5, 2), records, counts, None, half), (ref_rec, ref_st), what + ", 3 padded frames, stride 20")
            rng = np.random.default_rng(50 + k)
            words = rng.choice(np.array([0, 0, 0, 1, 2, 5, 0x7EADBEEF], np.int32), size=(3, p)).astype(np.int32)
            handed = (words != 0) & (ref_st != UNWRITTEN)
            exp_rec, exp_st = ref_rec.copy(), ref_st.copy()
            exp_rec[handed] = 0.0
            exp_st[handed] = words[handed]
            same_bytes(windows(det, padded(frames, 3, 0), records[:, :, :2], counts, to_device(words), half), (exp_rec, exp_st), what + ", status_in")
    # (squares of 6 px survive the detector's own blur and a sharper one; a wider blur may leave no saddle to accept)
    assert refined > 0 or sigma > 1.5, "no point of any frame refined: the inputs check nothing"


@pytest.mark.parametrize("factor", (2, 3))
def test_factor_maps_the_points_as_numpy_float32_does(det, factor):
    """At factor 2 and 3 the bytes equal the existing entry's on the points mapped by numpy in float32: one rounded multiply, one
    rounded add."""
    refined = 0
    for sigma, half in ((1.5, 2), (3.0, 4), (0.8, 1)):
        det.set_blur_sigma(sigma)
        for k, (w, h) in enumerate(((17, 23), (67, 45))):
            for fmt in FORMATS:
                frames = to_device(make_frames(3, w, h, fmt, 60 + k))
                coarse = make_points(3, -(-w // factor), -(-h // factor), 70 + k)
                coarse[:, ::3] += np.float32(0.37)  # (not only multiples of a half)
                mapped = coarse * np.float32(factor) + np.float32(0.5) * np.float32(factor - 1)
                assert mapped.dtype == np.float32
                ref = reference(det, frames, to_device(mapped), None, half)
                got = windows(det, frames, to_device(coarse), None, None, half, factor=factor)
                same_bytes(got, ref, "%dx%d %s factor %d sigma %g half %d" % (w, h, fmt, factor, sigma, half))
                refined += int((ref[1] == 0).sum())
    assert refined > 0, "no point of any frame refined: the inputs check nothing"


def test_refusals(det):
    import torch
    import aprilgrid_rs_amd as A
    ARG = A._ffi.AGX_ERR_ARG
    frames, pts = to_device(make_frames(1, 17, 23, "L8", 1)), to_device(make_points(1, 17, 23, 2))
    p = pts.shape[1]
    out, st = torch.zeros((1, p, 5), dtype=torch.float32, device="cuda:0"), torch.zeros((1, p), dtype=torch.int32, device="cuda:0")
    for kw in (dict(factor=0), dict(factor=5), dict(half_size_patch=0), dict(half_size_patch=5)):
        with pytest.raises(A.AgxError) as e:
            det.refine_windows_enqueue(frames, pts, out, st, **kw)
        assert e.value.status == ARG, kw
    lib, h = A._ffi.lib(), det._h
    args = lambda fmt, stride, o, s: (h, frames.data_ptr(), 1, 17, 23, 17, 17 * 23, fmt, pts.data_ptr(), stride, p, None, None, o, s, 1, 2)
    assert lib.agx_refine_windows_enqueue(*args(A._ffi.AGX_L8, 8, out.data_ptr(), st.data_ptr())) == A._ffi.AGX_OK
    assert lib.agx_refine_windows_enqueue(*args(A._ffi.AGX_RGB8, 8, out.data_ptr(), st.data_ptr())) == A._ffi.AGX_ERR_FORMAT
    for stride, o, s in ((4, out.data_ptr(), st.data_ptr()), (10, out.data_ptr(), st.data_ptr()), (8, None, st.data_ptr()), (8, out.data_ptr(), None)):
        assert lib.agx_refine_windows_enqueue(*args(A._ffi.AGX_L8, stride, o, s)) == ARG, (stride, o, s)
    det.sync()
