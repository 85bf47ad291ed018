"""Blur and Hessian-response planes at any sigma on device batches (agx_planes_enqueue, agx_gaussian_blur_f32,
agx_hessian_response; reference src/image_util.rs:110-206 and :72-109) against the oracle's gaussian_blur_f32 /
hessian_response.  Every comparison of planes is bit equality: the operations and their order are the reference's and
contraction is off -- the bar the chain's own blur plane meets."""
import os

import numpy as np
import pytest

from tests.util import bits_equal, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
L8, L16, RGB8, LF32, BGRA8, RGB8P, RGBA16 = 0, 1, 2, 3, 7, 8, 11
SENTINEL = 0x7FC5A5A5  # a NaN with a payload: no arithmetic produces it
TILE_X, TILE_Y = 64, 64  # k_gauss_blur's output tile (csrc/chain_kernels.h: GB_TX, GB_TY)

SIGMAS = [0.3, 0.5, 1.5, 2.0, 2.25, 3.3, 8.0]  # radii 1, 1, 3, 4, 5, 7, 16
SHAPES = [(1, 1), (2, 3), (3, 2), (5, 40), (40, 5), (7, 7), (16, 17), (17, 33), (33, 34), (64, 32), (65, 33), (131, 70), (320, 200),
          # one pixel either side of the tile in both directions
          (TILE_X - 1, TILE_Y + 1), (TILE_X + 1, TILE_Y - 1), (TILE_X, TILE_Y), (2 * TILE_X + 1, 2 * TILE_Y - 1)]


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


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def sentinel(shape):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def f32_frames(rng, n, w, h):
    """Finite float32 planes: [0,1) values, exact zeros, and values up to +-1e6."""
    a = rng.random((n, h, w)).astype(np.float32)
    a[rng.random(a.shape) < 0.1] = 0.0
    wide = rng.random(a.shape) < 0.1
    a[wide] = rng.uniform(-1e6, 1e6, int(wide.sum())).astype(np.float32)
    return a


def planes(det, frames, sigma, want_blur=True, want_response=False, format=None):
    """-> (blur or None, response or None) as numpy, outputs pre-filled with the sentinel."""
    n = frames.shape[0]
    h, w = (frames.shape[2], frames.shape[3]) if format == RGB8P else (frames.shape[1], frames.shape[2])
    blur = sentinel((n, h, w)) if want_blur else None
    resp = sentinel((n, h, w)) if want_response else None
    det.planes_enqueue(frames, sigma, blur=blur, response=resp, format=format)
    return (host(blur) if want_blur else None), (host(resp) if want_response else None)


# ---- 1. radius x shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SIGMAS)
def test_every_radius_at_every_shape(det, oracle, sigma):
    rng = np.random.default_rng(int(sigma * 1000))
    for w, h in SHAPES:
        a = f32_frames(rng, 2, w, h)
        blur, _ = planes(det, dev(a), sigma)
        for f in range(2):
            assert bits_equal(blur[f], oracle.gaussian_blur_f32(a[f], sigma)), "sigma %g, %dx%d, frame %d" % (sigma, w, h, f)


# ---- 2. formats -------------------------------------------------------------------------------------------------------------
FW, FH, FSIGMA = 131, 70, 2.25


def weighted(r, g, b):
    return (2126 * r.astype(np.uint32) + 7152 * g.astype(np.uint32) + 722 * b.astype(np.uint32)) // 10000


def format_cases(rng):
    """name -> (device tensor, format or None, expected to_luma32f plane [n, FH, FW])."""
    from oracle import oracle as O
    n = 2
    l8 = rng.integers(0, 256, (n, FH, FW), dtype=np.uint8)
    l16 = rng.integers(0, 65536, (n, FH, FW), dtype=np.uint16)
    rgb = rng.integers(0, 256, (n, FH, FW, 3), dtype=np.uint8)
    f32 = f32_frames(rng, n, FW, FH)
    bgra = rng.integers(0, 256, (n, FH, FW, 4), dtype=np.uint8)
    planar = rng.integers(0, 256, (n, 3, FH, FW), dtype=np.uint8)
    rgba16 = rng.integers(0, 65536, (n, FH, FW, 4), dtype=np.uint16)
    via_oracle = lambda a: np.stack([O.luma_f32(x) for x in a])
    return {
        "L8": (dev(l8), None, via_oracle(l8)),
        "L16": (dev(l16), None, via_oracle(l16)),
        "RGB8": (dev(rgb), None, via_oracle(rgb)),
        "LF32": (dev(f32), None, via_oracle(f32)),
        # the front-end layouts: the header's integer formula, then / 255 or / 65535 in float32
        "BGRA8": (dev(bgra), BGRA8, weighted(bgra[..., 2], bgra[..., 1], bgra[..., 0]).astype(np.float32) / np.float32(255)),
        "RGB8P": (dev(planar), RGB8P, weighted(planar[:, 0], planar[:, 1], planar[:, 2]).astype(np.float32) / np.float32(255)),
        "RGBA16": (dev(rgba16), RGBA16, weighted(rgba16[..., 0], rgba16[..., 1], rgba16[..., 2]).astype(np.float32) / np.float32(65535)),
    }


def run_formats(det, oracle):
    for name, (t, fmt, luma) in format_cases(np.random.default_rng(2)).items():
        assert luma.dtype == np.float32
        blur, resp = planes(det, t, FSIGMA, True, True, format=fmt)
        for f in range(luma.shape[0]):
            ref = oracle.gaussian_blur_f32(luma[f], FSIGMA)
            assert bits_equal(blur[f], ref), "%s frame %d: blur" % (name, f)
            assert bits_equal(resp[f], oracle.hessian_response(ref)), "%s frame %d: response" % (name, f)


def test_every_kind_of_format(det, oracle):
    run_formats(det, oracle)


# ---- 3. strides -------------------------------------------------------------------------------------------------------------
def test_padded_rows_and_frames_in_and_out(det, oracle):
    import torch
    rng = np.random.default_rng(3)
    n, w, h = 3, 61, 37
    big = rng.integers(0, 256, (n, h + 2, w + 3), dtype=np.uint8)  # byte pitch w + 3, two rows of padding per frame
    frames = dev(big)[:, :h, :w]
    guard = 257
    store = sentinel((n * (h + 3) * (w + 5) + guard,))
    out = store[: n * (h + 3) * (w + 5)].view(n, h + 3, w + 5)[:, :h, :w]  # row stride 4 * (w + 5), padded frame stride
    assert not frames.is_contiguous() and out.stride() == ((h + 3) * (w + 5), w + 5, 1)
    for sigma, key in ((2.25, "blur"), (0.0, "response")):
        store.view(torch.int32).fill_(SENTINEL)
        det.planes_enqueue(frames, sigma, **{key: out})
        got = host(store).view(np.uint32)
        body = got[: n * (h + 3) * (w + 5)].reshape(n, h + 3, w + 5)
        assert (got[n * (h + 3) * (w + 5):] == SENTINEL).all(), "guard behind the last frame"
        assert (body[:, h:, :] == SENTINEL).all() and (body[:, :, w:] == SENTINEL).all(), "padding was written"
        for f in range(n):
            luma = oracle.luma_f32(np.ascontiguousarray(big[f, :h, :w]))
            ref = oracle.gaussian_blur_f32(luma, sigma) if sigma else oracle.hessian_response(luma)
            assert bits_equal(body[f, :h, :w].view(np.float32), ref), "%s frame %d" % (key, f)


# ---- 4. batches -------------------------------------------------------------------------------------------------------------
def test_five_frames_each_its_own_plane_and_the_same_bits_twice(det, oracle):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (5, 50, 75), dtype=np.uint8)
    t = dev(a)
    first, _ = planes(det, t, 3.3)
    for f in range(5):
        assert bits_equal(first[f], oracle.gaussian_blur_f32(oracle.luma_f32(a[f]), 3.3)), f
    second, _ = planes(det, t, 3.3)
    assert bits_equal(first, second)


# ---- 5. response ------------------------------------------------------------------------------------------------------------
RESPONSE_SHAPES = [(2, 9), (9, 2), (3, 3), (65, 33)]


def run_responses(det, oracle):
    rng = np.random.default_rng(5)
    for w, h in RESPONSE_SHAPES:
        a = f32_frames(rng, 2, w, h)
        t = dev(a)
        for sigma in (1.5, 3.3):
            blur, resp = planes(det, t, sigma, True, True)
            only, = planes(det, t, sigma, False, True)[1:]
            for f in range(2):
                ref_blur = oracle.gaussian_blur_f32(a[f], sigma)
                ref = oracle.hessian_response(ref_blur)
                what = "sigma %g, %dx%d, frame %d" % (sigma, w, h, f)
                assert bits_equal(blur[f], ref_blur), what
                assert bits_equal(resp[f], ref), what + ": response"
                assert bits_equal(only[f], ref), what + ": response alone"
        plain = planes(det, t, 0.0, False, True)[1]
        for f in range(2):
            ref = oracle.hessian_response(a[f])
            assert bits_equal(plain[f], ref), "no blur, %dx%d, frame %d" % (w, h, f)
            # the outputs were NaN bits: the border ring -- the whole plane of a frame below 3 x 3 -- was written as +0.0
            ring = np.ones((h, w), bool)
            ring[1:-1, 1:-1] = False
            assert (plain[f].view(np.uint32)[ring] == 0).all()


def test_response_of_the_blur_and_of_the_luma_plane(det, oracle):
    run_responses(det, oracle)


# ---- 6. agreement with the chain ----------------------------------------------------------------------------------------------
def test_sigma_one_and_a_half_is_the_chains_blur_plane(det, oracle):
    synth = synth_module()
    fr, _ = synth.render_frame(0, 320, 200)
    a = fr.numpy()
    t = dev(a[None])
    blur, _ = planes(det, t, 1.5)
    det.saddles_batch_enqueue(t)
    det.saddles_batch_fetch()
    chain = det.debug_fetch(0, "blur", (200, 320))
    assert bits_equal(blur[0], chain)
    assert bits_equal(blur[0], oracle.gaussian_blur_f32(oracle.luma_f32(a), 1.5))


# ---- 7. into the refiner, no sync ---------------------------------------------------------------------------------------------
def test_a_plane_goes_straight_into_the_refiner(det, oracle):
    import torch
    from tests.test_gpu_refine_points import check_points, gt_corners
    synth = synth_module()
    w, h, sigma = 320, 200, 2.25
    fr, gt = synth.render_frame(0, w, h)
    a = fr.numpy()
    g = gt_corners(gt, w, h)
    assert len(g) >= 100
    rng = np.random.default_rng(7)
    pts = (g + rng.uniform(-1, 1, g.shape)).astype(np.float32)
    plane = torch.empty((1, h, w), dtype=torch.float32, device="cuda")
    det.planes_enqueue(dev(a[None]), sigma, blur=plane)
    det.refine_points_enqueue(plane, dev(pts[None]), image="plane", format=LF32)  # no sync, no fetch in between
    rec, st = det.refine_points_fetch()
    ref_plane = oracle.gaussian_blur_f32(oracle.luma_f32(a), sigma)
    acc = check_points(oracle, ref_plane, pts, rec[0], st[0], "sigma 2.25 plane")
    assert acc.sum() >= 50  # (the corners of a rendered board refine on a wider blur too)


# ---- 8. stream order ----------------------------------------------------------------------------------------------------------
def test_stream_order_behind_and_in_front_of_torch_ops(det, oracle):
    import torch
    rng = np.random.default_rng(8)
    a = rng.integers(0, 128, (2, 90, 140), dtype=np.uint8)
    src = dev(a)
    blur = sentinel((2, 90, 140))
    frames = src * 2  # produced on the current stream ...
    det.planes_enqueue(frames, 2.0, blur=blur)
    doubled = blur * 2.0  # ... and consumed on it, no host sync in between
    got = host(doubled)
    for f in range(2):
        ref = oracle.gaussian_blur_f32(oracle.luma_f32((a[f] * 2).astype(np.uint8)), 2.0)
        assert bits_equal(got[f], ref * np.float32(2.0)), f


# ---- 9. host calls ------------------------------------------------------------------------------------------------------------
def test_host_calls_give_the_batch_paths_bits(det, oracle):
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (70, 131), dtype=np.uint8)
    blur, _ = planes(det, dev(img[None]), 2.25)
    got = det.gaussian_blur_f32(img, 2.25)
    assert got.shape == (70, 131) and bits_equal(got, blur[0])
    assert bits_equal(got, oracle.gaussian_blur_f32(oracle.luma_f32(img), 2.25))
    assert bits_equal(det.gaussian_blur_f32(img), oracle.gaussian_blur_f32(oracle.luma_f32(img), 1.5))  # the default sigma
    resp = planes(det, dev(img[None]), 0.0, False, True)[1]
    got = det.hessian_response(img)
    assert bits_equal(got, resp[0]) and bits_equal(got, oracle.hessian_response(oracle.luma_f32(img)))
    rgb = rng.integers(0, 256, (33, 65, 3), dtype=np.uint8)
    assert bits_equal(det.gaussian_blur_f32(rgb, 0.5), oracle.gaussian_blur_f32(oracle.luma_f32(rgb), 0.5))
    f32 = f32_frames(rng, 1, 17, 9)[0]
    assert bits_equal(det.hessian_response(f32), oracle.hessian_response(f32))
    import aprilgrid_rs_amd as A
    for bad in (0.0, -1.0, float("nan"), 8.01):
        with pytest.raises(A.AgxError) as e:
            det.gaussian_blur_f32(img, bad)
        assert e.value.status == AGX_ERR_ARG


# ---- 10. errors and state -----------------------------------------------------------------------------------------------------
def test_argument_errors_and_the_sixth_kind_of_batch(det, oracle):
    import ctypes as C
    import torch
    from tests.test_golden_lists import check_saddle_fields, golden
    from tests.util import load_image
    lib, hnd = det._lib, det._h
    n, w, h = 2, 40, 30
    l8 = dev(np.zeros((n, h, w), np.uint8))
    f32 = dev(np.zeros((n, h, w + 1), np.float32))
    blur, resp = sentinel((n, h, w)), sentinel((n, h, w))
    det._follow_torch_stream(l8)

    def call(frames=l8.data_ptr(), rs=w, fs=w * h, fmt=L8, sigma=1.5, b=blur.data_ptr(), r=resp.data_ptr(), ors=4 * w, ofs=4 * w * h):
        return lib.agx_planes_enqueue(hnd, frames, n, w, h, rs, fs, fmt, sigma, b, r, ors, ofs)

    assert call() == AGX_OK
    assert call(frames=None) == AGX_ERR_ARG
    assert call(b=None, r=None) == AGX_ERR_ARG
    for sigma in (-1.0, float("nan"), float("inf"), float("-inf"), 8.01):
        assert call(sigma=sigma) == AGX_ERR_ARG, sigma
    assert call(sigma=8.0) == AGX_OK
    assert call(sigma=0.0) == AGX_ERR_ARG  # no blur, but a blur plane given
    assert call(sigma=0.0, b=None) == AGX_OK
    assert call(ors=4 * w - 4) == AGX_ERR_ARG and call(ors=4 * w + 2) == AGX_ERR_ARG
    assert call(ofs=4 * w * h - 4) == AGX_ERR_ARG
    assert call(frames=f32.data_ptr(), rs=4 * w + 2, fs=4 * (w + 1) * h, fmt=LF32) == AGX_ERR_ARG
    assert call(frames=f32.data_ptr(), rs=4 * w + 4, fs=4 * (w + 1) * h, fmt=LF32) == AGX_OK
    torch.cuda.synchronize()
    assert (blur.view(torch.int32) == 0).all() and not (resp.view(torch.int32) == SENTINEL).any()  # (the last good call ran)

    # a sixth kind of batch: nothing of it can be fetched, by any fetch
    assert call() == AGX_OK
    counts = np.zeros(n, np.uint32)
    st = np.zeros(n, np.int32)
    u32 = np.zeros(16, np.uint32)
    assert lib.agx_saddles_batch_fetch(hnd, None, 0, counts.ctypes.data, st.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_detect_batch_fetch(hnd, None, counts.ctypes.data, st.ctypes.data, 1) == AGX_ERR_STATE
    assert lib.agx_refine_points_fetch(hnd, u32.ctypes.data, u32.ctypes.data) == AGX_ERR_STATE
    assert lib.agx_decode_quads_fetch(hnd, u32.ctypes.data, u32.ctypes.data, None) == AGX_ERR_STATE
    assert lib.agx_find_boards_fetch(hnd, u32.ctypes.data, None, u32.ctypes.data, u32.ctypes.data, 1) == AGX_ERR_STATE
    import aprilgrid_rs_amd as A
    for fetch in (det.saddles_batch_fetch, det.detect_batch_fetch, det.refine_points_fetch, det.decode_quads_fetch, det.find_boards_fetch):
        with pytest.raises(A.AgxError) as e:
            fetch()
        assert e.value.status == AGX_ERR_STATE

    # and the handle goes on: the next saddle batch is a fixture's golden list
    name = "EuRoC.png"
    img = load_image(name)
    det.saddles_batch_enqueue(dev(img[None]))
    res, status = det.saddles_batch_fetch()
    assert status[0] == 0
    s = res[0]
    check_saddle_fields(s["x"], s["y"], s["k"], s["theta"], s["phi"], golden(name), name + " after a planes batch")


# ---- 11. guard bytes ----------------------------------------------------------------------------------------------------------
def test_guard_bytes_stay_intact(oracle):
    import aprilgrid_rs_amd as A
    os.environ["AGX_REDZONE_BYTES"] = "4096"
    try:
        gdet = A.TagDetector("t36h11", None, device=0)
    finally:
        del os.environ["AGX_REDZONE_BYTES"]
    try:
        run_formats(gdet, oracle)
        run_responses(gdet, oracle)
        gdet.gaussian_blur_f32(np.zeros((9, 11), np.uint8), 8.0)
        r = gdet.debug_fetch(0, "redzones")
        assert r["buffers"] >= 4, r  # the front-end plane, the workspace blur planes, staging and the host calls' plane
        assert r["damaged_bytes"] == 0, r
    finally:
        gdet.close()
