"""The host forms of the rectified batches (agx_rectify_map_tail, agx_remap_tail, agx_rectified_points_tail) without a device:
the map against a numpy float64 statement of both lens models, the remap against a numpy integer statement byte for byte and
against scipy's map_coordinates, the points against the map and the model, the refusals, and the oracle's detect on rectified
fisheye frames."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

from tests import board_pose_cases as PC
from tests import rectify_cases as RC
from tests.rectify_cases import CAMERAS, DST, NEW_CAMERA, NONE, PINHOLE, ROTATION, SRC


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("lens", ["radtan", "equi"])
def test_map_is_the_numpy_model_rounded_to_a_32nd_of_a_pixel(lens, rotated):
    """Every entry valid on both sides is within 1/64 px (+ 1e-9) of numpy's float64 projection; validity agrees everywhere but
    within 1e-9 px of a boundary, and numpy alone shows that such entries are at most 0.5 % of the map (none, for these cameras)."""
    cam, R = CAMERAS[lens], ROTATION if rotated else None
    m = A.rectify_map(cam, SRC, DST, NEW_CAMERA, R)
    assert m.shape == (DST[1], DST[0], 2) and m.dtype == np.int32
    uv, valid, near = RC.numpy_map(cam, SRC, DST, NEW_CAMERA, R)
    assert near.mean() <= 0.005
    ours = m[..., 0] != NONE
    assert np.array_equal(ours, m[..., 1] != NONE)
    assert np.array_equal(ours[~near], valid[~near])
    assert 0.5 < valid.mean() < 0.99  # (the case has entries of both kinds)
    both = ours & valid
    err = np.abs(m[both] / 32.0 - uv[both]).max()
    print("%s rotated=%s: %d valid of %d, max |m / 32 - numpy| = %.6f px" % (lens, rotated, both.sum(), both.size, err))
    assert err <= 1.0 / 64.0 + 1e-9
    assert m[both][:, 0].max() <= 32 * (SRC[0] - 1) and m[both][:, 1].max() <= 32 * (SRC[1] - 1) and m[both].min() >= 0


def test_map_row_stride_leaves_the_padding_alone():
    m = A.rectify_map(CAMERAS["equi"], SRC, DST, NEW_CAMERA, ROTATION, row_stride=8 * DST[0] + 24)
    assert np.array_equal(m, A.rectify_map(CAMERAS["equi"], SRC, DST, NEW_CAMERA, ROTATION))
    assert (m.base[:, 2 * DST[0]:] == 0x5a5a5a5a).all() and m.base.shape[1] == 2 * DST[0] + 6


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_identity(dtype):
    """A zero-distortion camera rectified to itself: the map is exactly (32 i, 32 j) and remap returns the source's bytes."""
    m = A.rectify_map(PINHOLE, SRC)  # (defaults: the source's size, the camera's own fx fy cx cy, no rotation)
    i, j = np.meshgrid(np.arange(SRC[0]), np.arange(SRC[1]))
    assert np.array_equal(m[..., 0], 32 * i) and np.array_equal(m[..., 1], 32 * j)
    assert np.array_equal(m, A.rectify_map(PINHOLE, SRC, SRC, PINHOLE[:4], np.eye(3)))
    img = RC.image(2, SRC, dtype)
    assert np.array_equal(A.remap(img, m), img)
    assert np.array_equal(A.remap(img[0], m), img[0])


def _maps():
    m = A.rectify_map(CAMERAS["equi"], SRC, DST, NEW_CAMERA, ROTATION)
    return {"camera": m, "callers": RC.callers_map(SRC, DST), "none": np.full_like(m, NONE), "one": RC.callers_map(SRC, (1, 1)),
            "narrow": RC.callers_map(SRC, (5, 3))}


@pytest.mark.parametrize("dtype,border", [(np.uint8, 0), (np.uint8, 201), (np.uint16, 51234)])
@pytest.mark.parametrize("which", ["camera", "callers", "none", "one", "narrow"])
def test_remap_is_the_numpy_integer_statement_byte_for_byte(which, dtype, border):
    """L8 and L16, padded strides on both sides with their padding intact, a non-zero border, entries exactly at 32 (src - 1) in x,
    in y and in both, out-of-range entries of a caller's map, an all-AGX_MAP_NONE map."""
    m = _maps()[which]
    px = np.dtype(dtype).itemsize
    img = RC.image(3, SRC, dtype)
    want = RC.numpy_remap(img, m, border)
    assert np.array_equal(A.remap(img, m, border), want)
    src, _ = RC.padded(img, 6 * px, 10 * px)
    out, buf = RC.padded(np.zeros_like(want), 3 * px, 8 * px)
    keep = buf.copy()
    A.remap(src, m, border, out=out)
    assert np.array_equal(out, want)
    out[...] = 0
    mask = buf.copy()
    out[...] = np.iinfo(dtype).max
    pad = mask == buf  # the bytes that are no pixel of out
    assert np.array_equal(keep[pad], buf[pad]) and (buf[pad] == 0xA5).all()
    if which == "none":
        assert (want == border).all()
    if which == "callers":
        flat, w = m.reshape(-1, 2), want[0].reshape(-1)
        ex, ey = 32 * (SRC[0] - 1), 32 * (SRC[1] - 1)
        assert tuple(flat[1]) == (ex, 40) and tuple(flat[4]) == (40, ey) and tuple(flat[7]) == (ex, ey)
        assert w[7] == img[0, SRC[1] - 1, SRC[0] - 1]  # (the last pixel itself: both neighbours are clamped onto it)
        for k in range(3, 11):  # callers_map's entries one past the limits, negative, half or wholly AGX_MAP_NONE, INT32_MAX
            assert w[3 * k + 1] == border


def test_remap_against_scipy_map_coordinates():
    """At the quantised positions scipy's order-1 interpolation in float64 and the 5-bit fixed-point blend differ by at most one
    grey level (round half up against round half even, at ties only)."""
    from scipy.ndimage import map_coordinates
    m = A.rectify_map(CAMERAS["radtan"], SRC, DST, NEW_CAMERA, ROTATION)
    valid = m[..., 0] != NONE
    for dtype in (np.uint8, np.uint16):
        img = RC.image(1, SRC, dtype)[0]
        got = A.remap(img, m).astype(np.int64)
        ref = map_coordinates(img.astype(np.float64), [m[..., 1] / 32.0, m[..., 0] / 32.0], order=1, mode="nearest")
        d = np.abs(got - np.rint(ref))[valid]
        print("%s: %.4f %% of %d pixels differ from rint(scipy), max %d" % (np.dtype(dtype).name, 100.0 * (d > 0).mean(), d.size, d.max()))
        assert d.max() <= 1
        assert np.abs(got - ref)[valid].max() <= 0.5 + 1e-6  # (the blend is the exact bilinear value rounded half up)


@pytest.mark.parametrize("lens", ["radtan", "equi"])
def test_rectified_points_are_the_maps_projection(lens):
    """At integer positions the points are the map's entries before quantisation (|p - m / 32| <= 1/64 + a float32 rounding), within
    1e-4 px of the numpy model everywhere, and (NaN, NaN) where Z <= 0 or the point is not finite."""
    cam = CAMERAS[lens]
    i, j = np.meshgrid(np.arange(DST[0]), np.arange(DST[1]))
    pts = np.stack([i, j], axis=-1).astype(np.float32)
    got = A.rectified_points(pts, cam, NEW_CAMERA, ROTATION)
    assert got.dtype == np.float32 and got.shape == pts.shape
    m = A.rectify_map(cam, SRC, DST, NEW_CAMERA, ROTATION)
    valid = m[..., 0] != NONE
    assert np.abs(got[valid].astype(np.float64) - m[valid] / 32.0).max() <= 1.0 / 64.0 + 2.0 ** -17  # (half an ulp of a float32 below 128)
    q = np.floor(got[valid].astype(np.float64) * 32.0 + 0.5)
    assert (np.abs(q - m[valid]) <= 1).all() and (q == m[valid]).mean() > 0.999
    uv, _ = RC.numpy_points(cam, NEW_CAMERA, ROTATION, i, j)
    err = np.abs(got - uv).max()
    print("%s: max |rectified_points - numpy| = %.3g px" % (lens, err))
    assert err <= 1e-4
    # fractional positions, and a rotation that puts part of the target behind the camera
    rng = np.random.RandomState(5)
    pts = (rng.rand(500, 2) * [DST[0] * 3, DST[1]]).astype(np.float32)
    R = PC.rotation(0.0, 75.0, 0.0)
    got = A.rectified_points(pts, cam, NEW_CAMERA, R)
    uv, z = RC.numpy_points(cam, NEW_CAMERA, R, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    behind = z <= 0.0
    assert 20 < behind.sum() < 480
    assert np.isnan(got[behind]).all() and np.isfinite(got[~behind]).all()
    assert np.abs(got[~behind] - uv[~behind]).max() <= 1e-4 * max(1.0, np.abs(uv[~behind]).max() / 100.0)
    odd = A.rectified_points(np.array([[np.nan, 1.0], [1.0, np.inf], [3.0, 4.0]], np.float32), cam, NEW_CAMERA)
    assert np.isnan(odd[:2]).all() and np.isfinite(odd[2]).all()
    assert A.rectified_points(np.zeros((0, 2), np.float32), cam, NEW_CAMERA).shape == (0, 2)


# the counts the oracle's detect gives on the host form's rectified frame; numpy's rectification (scipy's interpolation at the
# same quantised positions) gives the same two
PINNED = {0.62: 36, 0.35: 21}


@pytest.mark.parametrize("ratio", [0.62, 0.35])
def test_detect_on_rectified_fisheye_frames(ratio):
    """board_pose_equi_cases' rendered 6 x 6 frame behind an equidistant lens of `ratio` times the pinhole's focal length, rectified
    by the host forms at the lens's own focal length and size: the oracle's detect finds what it finds on the numpy-rectified frame
    (36 tags at 0.62, 21 at 0.35 where the fisheye frame itself gives 16), and its corners, taken back to the sensor with
    rectified_points, are compared with the ground truth pushed through the fisheye model beside the direct detect's corners, over
    the tags both paths find.  Measured, px (median / max):
        ratio 0.62, 36 common tags: rectified path 0.028 / 0.062, direct 0.029 / 0.057
        ratio 0.35, 13 common tags: rectified path 0.057 / 0.115, direct 0.083 / 0.462
    The rectified path's maximum must be at most twice the direct path's: its image is interpolated twice."""
    from oracle import oracle as O
    luma, cam, truth, (w, h) = RC.fisheye_frame(ratio)
    rect = A.remap(luma, A.rectify_map(cam, (w, h)))
    found = O.detect(rect)
    by_numpy = O.detect(RC.numpy_rectified(luma, cam))
    direct = O.detect(luma)
    print("ratio %.2f: detect finds %d tags on the fisheye frame, %d on the host form's rectified frame, %d on numpy's" %
          (ratio, len(direct), len(found), len(by_numpy)))
    assert sorted(found) == sorted(by_numpy)
    assert len(found) == PINNED[ratio]
    back = {t: A.rectified_points(np.asarray(xy, np.float32).reshape(4, 2), cam, None) for t, xy in found.items()}
    common = sorted(set(back) & set(direct))
    assert len(common) >= 10
    e_rect = RC.corner_errors({t: back[t] for t in common}, truth)
    e_direct = RC.corner_errors({t: direct[t] for t in common}, truth)
    print("ratio %.2f, %d common tags: rectified path median %.3f max %.3f px, direct median %.3f max %.3f px" %
          (ratio, len(common), np.median(e_rect), e_rect.max(), np.median(e_direct), e_direct.max()))
    assert e_rect.max() <= 2.0 * e_direct.max()


def _refused(call, *a, **kw):
    with pytest.raises(A.AgxError) as e:
        call(*a, **kw)
    assert e.value.status == _ffi.AGX_ERR_ARG, e.value


def test_refusals():
    """Every AGX_ERR_ARG rule of the three host forms, through Python."""
    cam, eq = CAMERAS["radtan"], CAMERAS["equi"]
    nan, inf = float("nan"), float("inf")
    for mk in (lambda c, n, r=None: A.rectify_map(c, SRC, DST, n, r), lambda c, n, r=None: A.rectified_points(np.zeros((2, 2), np.float32), c, n, r)):
        # agx_board_pose_enqueue_m's rules on the lens model and the camera
        _refused(mk, cam._replace(fx=0.0), NEW_CAMERA)
        _refused(mk, cam._replace(fy=-1.0), NEW_CAMERA)
        _refused(mk, cam._replace(k1=nan), NEW_CAMERA)
        _refused(mk, cam._replace(cx=inf), NEW_CAMERA)
        _refused(mk, type(eq)(*eq[:8], 1e-3), NEW_CAMERA)  # the equidistant model's ninth double
        # new_camera
        _refused(mk, cam, (0.0, 50.0, 1.0, 1.0))
        _refused(mk, cam, (50.0, -2.0, 1.0, 1.0))
        _refused(mk, cam, (50.0, 50.0, nan, 1.0))
        _refused(mk, cam, (inf, 50.0, 1.0, 1.0))
        _refused(mk, cam, (50.0, 50.0, 1.0))
        # rotation
        bad = np.eye(3)
        bad[1, 2] = nan
        _refused(mk, cam, NEW_CAMERA, bad)
        _refused(mk, cam, NEW_CAMERA, np.eye(2))
    lib = _ffi.lib()
    buf = np.zeros((4, 4, 2), np.int32)
    nc, c9 = (A.detector.C.c_double * 4)(*NEW_CAMERA), cam.as_doubles()
    assert lib.agx_rectify_map_tail(7, c9, nc, None, 8, 8, 4, 4, buf.ctypes.data, 32) == _ffi.AGX_ERR_ARG  # an unknown lens model
    assert lib.agx_rectify_map_tail(0, None, nc, None, 8, 8, 4, 4, buf.ctypes.data, 32) == _ffi.AGX_ERR_ARG
    assert lib.agx_rectify_map_tail(0, c9, None, None, 8, 8, 4, 4, buf.ctypes.data, 32) == _ffi.AGX_ERR_ARG  # a NULL new_camera
    assert lib.agx_rectify_map_tail(0, c9, nc, None, 8, 8, 4, 4, buf.ctypes.data, 32) == _ffi.AGX_OK
    # sizes
    for src, dst in (((0, 59), DST), ((83, 0), DST), ((16385, 59), DST), ((83, 16385), DST), (SRC, (0, 61)), (SRC, (97, 0)), (SRC, (16385, 61)),
                     (SRC, (97, 16385))):
        _refused(A.rectify_map, cam, src, dst, NEW_CAMERA)
    assert A.rectify_map(cam, (16384, 16384), (3, 2), NEW_CAMERA).shape == (2, 3, 2)
    # the map's stride and pointer
    _refused(A.rectify_map, cam, SRC, DST, NEW_CAMERA, row_stride=8 * DST[0] - 8)
    _refused(A.rectify_map, cam, SRC, DST, NEW_CAMERA, row_stride=8 * DST[0] + 4)
    assert lib.agx_rectify_map_tail(0, c9, nc, None, 8, 8, 4, 4, None, 32) == _ffi.AGX_ERR_ARG
    assert lib.agx_rectify_map_tail(0, c9, nc, None, 8, 8, 3, 4, buf.ctypes.data + 4, 32) == _ffi.AGX_ERR_ARG
    # the remap
    m = A.rectify_map(cam, SRC, DST, NEW_CAMERA)
    img8, img16 = RC.image(2, SRC, np.uint8), RC.image(2, SRC, np.uint16)
    _refused(A.remap, img8, m, 256)
    _refused(A.remap, img16, m, 65536)
    _refused(A.remap, img8.astype(np.float32), m)
    _refused(A.remap, img8, m.astype(np.int64))
    _refused(A.remap, img8, m, out=np.zeros((2, DST[1], DST[0]), np.uint16))
    out = np.zeros((2, DST[1], DST[0]), np.uint8)

    def raw(**kw):
        a = dict(src=img8.ctypes.data, n=2, sw=SRC[0], sh=SRC[1], srs=SRC[0], sfs=SRC[0] * SRC[1], fmt=_ffi.AGX_L8, map=m.ctypes.data, ms=8 * DST[0],
                 dw=DST[0], dh=DST[1], dst=out.ctypes.data, drs=DST[0], dfs=DST[0] * DST[1], border=0)
        a.update(kw)
        return lib.agx_remap_tail(a["src"], a["n"], a["sw"], a["sh"], a["srs"], a["sfs"], a["fmt"], a["map"], a["ms"], a["dw"], a["dh"], a["dst"], a["drs"],
                                  a["dfs"], a["border"])

    assert raw() == _ffi.AGX_OK
    for kw in (dict(src=None), dict(dst=None), dict(map=None), dict(n=0), dict(n=65536), dict(fmt=_ffi.AGX_RGB8), dict(fmt=_ffi.AGX_LF32), dict(fmt=99),
               dict(sw=0), dict(sh=0), dict(sw=65001, srs=65001), dict(dw=0), dict(dh=0), dict(dw=16385, drs=16385, ms=8 * 16385), dict(srs=SRC[0] - 1),
               dict(sfs=SRC[0] * SRC[1] - 1), dict(drs=DST[0] - 1), dict(dfs=DST[0] * DST[1] - 1), dict(srs=2 ** 31, sfs=2 ** 40), dict(srs=2 ** 26, sfs=2 ** 40),
               dict(ms=8 * DST[0] - 8), dict(ms=8 * DST[0] + 4), dict(map=m.ctypes.data + 4), dict(border=256)):
        assert raw(**kw) == _ffi.AGX_ERR_ARG, kw
    for kw in (dict(src=img16.ctypes.data + 1), dict(srs=2 * SRC[0] + 1), dict(sfs=2 * SRC[0] * SRC[1] + 1), dict(border=65536)):
        a = dict(src=img16.ctypes.data, srs=2 * SRC[0], sfs=2 * SRC[0] * SRC[1], fmt=_ffi.AGX_L16, dst=np.zeros((2, DST[1], DST[0]), np.uint16).ctypes.data,
                 drs=2 * DST[0], dfs=2 * DST[0] * DST[1])
        a.update(kw)
        assert raw(**a) == _ffi.AGX_ERR_ARG, kw
    # the points' list
    pts = np.zeros((4, 2), np.float32)
    ok = lambda p, s, n, o, os: lib.agx_rectified_points_tail(0, c9, nc, None, p, s, n, o, os)
    assert ok(pts.ctypes.data, 8, 4, pts.ctypes.data, 8) == _ffi.AGX_OK
    assert ok(None, 8, 0, None, 8) == _ffi.AGX_OK
    for args in ((None, 8, 4, pts.ctypes.data, 8), (pts.ctypes.data, 8, 4, None, 8), (pts.ctypes.data, 4, 4, pts.ctypes.data, 8),
                 (pts.ctypes.data, 8, 4, pts.ctypes.data, 6), (pts.ctypes.data + 2, 8, 3, pts.ctypes.data, 8), (pts.ctypes.data, 8, 2 ** 30, pts.ctypes.data, 8)):
        assert ok(*args) == _ffi.AGX_ERR_ARG, args
