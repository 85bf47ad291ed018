"""The saddle chain and detect at a blur sigma other than the reference's 1.5 (agx_detector_set_blur_sigma): k_gauss_blur +
k_response_front in front of the unchanged sparse stages, against tests/sigma_oracle.py -- the reference's
refined_saddle_points composed from the oracle's pieces with the sigma in place of the 1.5 of src/detector.rs:410, which
tests/test_sigma_cpu.py holds to the oracle's own chain at 1.5.  The bar is the chain's (tests/test_gpu_parity.py): planes,
minima, cluster tables, centroids and x / y / k bit for bit, theta / phi within tests.util.ANGLE_TOL_DEG."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sigma_oracle
from tests.util import bits_equal, check_frame, check_saddles, check_tags, load_image, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
L8, L16, RGB8, LF32, BGRA8 = 0, 1, 2, 3, 7
SWEEP = (0.5, 1.0, 2.0, 2.5, 4.0, 6.0, 8.0)


class SigmaOracle:
    """What tests.util.check_frame asks of the oracle module, answered by the helper at one sigma (results kept per image)."""

    def __init__(self, sigma):
        self.sigma = sigma
        self.seen = {}

    def refined_saddle_points(self, img, params=None, debug=False):
        key = (img.shape, img.dtype.str, img.tobytes())
        if key not in self.seen:
            self.seen[key] = sigma_oracle.refined_saddle_points(img, self.sigma, params)
        ref, d = self.seen[key]
        return (ref, d) if debug else ref


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


def new_detector(sigma=None, **options):
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0, blur_sigma=sigma)
    for k, v in options.items():
        d.set_option(k, v)
    return d


@pytest.fixture(scope="module")
def det():
    """One handle for the whole sweep, with store_response: it alternates between sigmas, sizes and fronts."""
    d = new_detector(store_response=1)
    yield d
    d.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


@pytest.fixture(scope="module")
def boards():
    """Three distinct synthetic 320 x 240 L8 frames."""
    return synth_module().render_batch(0, 3, 320, 240)[0].numpy()


def run(d, frames, fmt=None):
    d.saddles_batch_enqueue(dev(frames), format=fmt)
    res, status = d.saddles_batch_fetch()
    assert (status == 0).all(), status
    return res


def same_lists(a, b, what):
    assert len(a) == len(b), what
    for i in range(len(a)):
        assert a[i].tobytes() == b[i].tobytes(), "%s: frame %d" % (what, i)


# ---- 1. sigma sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SWEEP)
def test_sigma_sweep(det, boards, sigma):
    """Every product of the chain -- blur plane, the response recomputed from it and the one k_response_front stores, min,
    cluster first pixels and sizes, centroids, unfiltered refine output, final list -- no overflow flag, the any-sigma front."""
    orc = SigmaOracle(sigma)
    det.set_blur_sigma(sigma)
    assert det.blur_sigma == np.float32(sigma)
    res = run(det, boards)
    assert det.get_option("last_chain_front") == 1
    for i in range(3):
        ref = check_frame(det, orc, boards[i], i, "sigma %g frame %d" % (sigma, i))
        check_saddles(res[i], ref, "sigma %g frame %d" % (sigma, i))
        assert len(ref) >= 1
    if sigma == 6.0:  # frame 0 has a component of 7756 pixels: it leaves both flood windows and takes the generic path
        assert int(orc.refined_saddle_points(boards[0], debug=True)[1]["sizes"].max()) == 7756
        assert det.debug_fetch(0, "counters")["flags"] & 16
    img = load_image("EuRoC.png")
    got = det.refined_saddle_points(img, as_array=True)
    assert det.get_option("last_chain_front") == 1
    ref = check_frame(det, orc, img, 0, "EuRoC.png at sigma %g" % sigma)
    check_saddles(got, ref, "EuRoC.png at sigma %g" % sigma)
    assert len(ref) >= 2
    if sigma == 0.5:
        assert len(ref) == 259


# ---- 2. default and explicit 1.5 ------------------------------------------------------------------------------------------
def test_default_explicit_and_next_to_1_5(boards):
    untouched, explicit = new_detector(), new_detector()
    try:
        assert untouched.blur_sigma == 1.5
        want = run(untouched, boards)
        assert untouched.get_option("last_chain_front") == 0
        explicit.set_blur_sigma(1.5)
        got = run(explicit, boards)
        assert explicit.get_option("last_chain_front") == 0
        same_lists(got, want, "explicit 1.5")
        near = np.nextafter(np.float32(1.5), np.float32(2))
        explicit.set_blur_sigma(near)
        assert np.float32(explicit.blur_sigma) == near and near != np.float32(1.5)
        got = run(explicit, boards)
        assert explicit.get_option("last_chain_front") == 1
        orc = SigmaOracle(near)
        for i in range(3):
            check_saddles(got[i], check_frame(explicit, orc, boards[i], i, "nextafter(1.5) frame %d" % i), "nextafter(1.5) frame %d" % i)
        explicit.blur_sigma = 1.5  # and back, on the same handle
        same_lists(run(explicit, boards), want, "back at 1.5")
        assert explicit.get_option("last_chain_front") == 0
    finally:
        untouched.close()
        explicit.close()


# ---- 3. state left behind -------------------------------------------------------------------------------------------------
def test_nothing_is_left_behind_between_batches():
    """Dense frames at 2.0, sparser ones at 2.0, the same at 1.5, fewer at 2.0 again: each result is a fresh handle's (mask or
    cand_max words that were not rewritten, counters left behind)."""
    synth = synth_module()
    dense = synth.render_batch(3, 4, 300, 200, pure_noise=True)[0].numpy()
    sparse = synth.render_batch(40, 4, 300, 200)[0].numpy()
    steps = [(2.0, dense), (2.0, sparse), (1.5, sparse), (2.0, sparse[:2])]
    one = new_detector()
    try:
        for n, (sigma, frames) in enumerate(steps):
            one.set_blur_sigma(sigma)
            got = run(one, frames)
            assert one.get_option("last_chain_front") == (0 if sigma == 1.5 else 1)
            if n == 0:
                assert sum(len(r) for r in got) == 225 + 236 + 254 + 238  # the helper's counts on the noise frames (533 on the others)
            fresh = new_detector(sigma)
            try:
                same_lists(got, run(fresh, frames), "step %d" % n)
            finally:
                fresh.close()
            if n == 1:
                orc = SigmaOracle(2.0)
                for i in range(4):
                    check_saddles(got[i], orc.refined_saddle_points(frames[i]), "step 1 frame %d" % i)
    finally:
        one.close()


# ---- 4. formats and strides -----------------------------------------------------------------------------------------------
def padded_batch(px, row_pad, frame_pad, offset):
    """px [N, H, row bytes] uint8 -> (flat uint8 buffer, offset of frame 0, row stride, frame stride): every row followed by
    row_pad bytes, every frame by frame_pad more, all padding 0xEE."""
    n, h, rb = px.shape
    rs = rb + row_pad
    fs = h * rs + frame_pad
    buf = np.full(offset + n * fs + 64, 0xEE, np.uint8)
    for f in range(n):
        for y in range(h):
            o = offset + f * fs + y * rs
            buf[o:o + rb] = px[f, y]
    return buf, offset, rs, fs


@pytest.mark.parametrize("name", ["L16", "RGB8", "BGRA8", "LF32", "L8 odd pitch"])
def test_formats_and_strides_at_sigma_2(name):
    import torch
    synth = synth_module()
    rng = np.random.default_rng(11)
    w, h = (317, 203) if name == "L8 odd pitch" else (320, 240)
    grey = np.stack([np.asarray(synth.render_frame(60 + i, 320, 240)[0]) for i in range(3)])[:, :h, :w]
    grey = np.ascontiguousarray(grey)
    if name == "L16":
        base = (grey.astype(np.uint16) * 257 + rng.integers(0, 60, grey.shape).astype(np.uint16)).astype(np.uint16)
        px, fmt, pads = base, L16, (6, 1000, 64)
    elif name in ("RGB8", "BGRA8"):
        base = np.stack([np.clip(grey.astype(np.int64) + d + rng.integers(-2, 3, grey.shape), 0, 255).astype(np.uint8) for d in (-3, 0, 4)], -1)
        if name == "RGB8":
            px, fmt, pads = base, RGB8, (5, 333, 3)
        else:
            px = np.concatenate([base[..., ::-1], rng.integers(0, 256, grey.shape + (1,), dtype=np.uint8)], -1)
            fmt, pads = BGRA8, (8, 404, 4)
    elif name == "LF32":
        base = (grey.astype(np.float32) / np.float32(255.0)).astype(np.float32)
        px, fmt, pads = base, LF32, (12, 2000, 16)
    else:
        base, px, fmt, pads = grey, grey, L8, (4, 0, 1)  # 317 + 4 = 321 bytes per row: the byte-row form
    raw = np.ascontiguousarray(px).view(np.uint8).reshape(3, h, -1)
    buf, off, rs, fs = padded_batch(raw, *pads)
    t = torch.from_numpy(buf).cuda()
    d = new_detector(2.0)
    try:
        d.saddles_batch_enqueue_ptr(t.data_ptr() + off, 3, w, h, rs, fs, fmt)
        res, status = d.saddles_batch_fetch()
        assert (status == 0).all() and d.get_option("last_chain_front") == 1
        orc = SigmaOracle(2.0)
        for i in range(3):
            ref = check_frame(d, orc, np.ascontiguousarray(base[i]), i, "%s frame %d" % (name, i))
            check_saddles(res[i], ref, "%s frame %d" % (name, i))
            assert len(ref) > 50
    finally:
        d.close()


# ---- 5. launch paths ------------------------------------------------------------------------------------------------------
def test_launch_paths_at_sigma_2(boards):
    orc = SigmaOracle(2.0)
    for option, value in (("sparse_path", 1), ("sparse_path", 2), ("sparse_path", 3), ("force_generic", 1)):
        d = new_detector(2.0, **{option: value})
        try:
            res = run(d, boards)
            assert d.get_option("last_chain_front") == 1
            if option == "sparse_path":
                assert d.get_option("last_sparse_path") == value
            for i in range(3):
                check_saddles(res[i], check_frame(d, orc, boards[i], i, "%s %d frame %d" % (option, value, i)), "%s %d frame %d" % (option, value, i))
        finally:
            d.close()


# ---- 6. small and awkward sizes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 8.0])
def test_small_and_awkward_sizes(det, sigma):
    """Seeded noise at every (W, H) of {2, 3, 8, 9, 31, 32, 33, 64, 65} x {2, 3, 9, 33, 65}; sigma 8.0 has radius 16, wider
    than the frames.  Most results are empty lists, as the helper's."""
    rng = np.random.default_rng(5)
    orc = SigmaOracle(sigma)
    det.set_blur_sigma(sigma)
    total = 0
    for w in (2, 3, 8, 9, 31, 32, 33, 64, 65):
        for h in (2, 3, 9, 33, 65):
            frames = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
            res = run(det, frames)
            for i in range(2):
                ref = check_frame(det, orc, frames[i], i, "%dx%d sigma %g frame %d" % (w, h, sigma, i))
                check_saddles(res[i], ref, "%dx%d sigma %g frame %d" % (w, h, sigma, i))
                total += len(ref)
    assert total > 0


# ---- 7. detect ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sigma", [("iphone.png", 1.0), ("EuRoC.png", 0.5)])
def test_detect(oracle, name, sigma):
    img = load_image(name)
    saddles, _ = sigma_oracle.refined_saddle_points(img, sigma)
    want = oracle.detect_tail(oracle.luma_u8(img), saddles)
    assert len(want) >= 30, len(want)
    d = new_detector(sigma)
    try:
        check_tags(d.detect(img), want, "%s agx_detect" % name)
        assert d.get_option("last_chain_front") == 1
        for tail in (0, 1):
            try:
                d.set_option("device_tail", tail)
            except Exception as e:
                if tail == 1 and getattr(e, "status", None) == AGX_ERR_STATE:
                    continue  # the device tail is not offered where this process's atan2f differs: nothing to run
                raise
            d.detect_batch_enqueue(dev(img[None]))
            got = d.detect_batch_fetch()
            assert len(got) == 1
            check_tags(got[0], want, "%s agx_detect_batch_enqueue, device_tail %d" % (name, tail))
    finally:
        d.close()


# ---- 8. refine of caller-given points on the handle's blur ----------------------------------------------------------------
def test_refine_points_on_the_blur_at_sigma_2(oracle):
    from tests.test_gpu_refine_points import MOVED, NOT_SADDLE, OUTSIDE, REFINED, check_points, gt_corners
    synth = synth_module()
    w, h = 320, 200
    fr, gt = synth.render_frame(0, w, h)
    frame = fr.numpy()
    rng = np.random.default_rng(2)
    g = gt_corners(gt, w, h)[:120]
    pts = np.concatenate([g + rng.uniform(-1, 1, g.shape), np.stack([rng.uniform(-3, w + 3, 200 - len(g)), rng.uniform(-3, h + 3, 200 - len(g))], 1)])
    pts = pts.astype(np.float32)
    assert pts.shape == (200, 2)
    blur = oracle.gaussian_blur_f32(oracle.luma_f32(frame), 2.0)
    d = new_detector(2.0)
    try:
        d.refine_points_enqueue(dev(frame[None]), dev(pts[None]))
        rec, st = d.refine_points_fetch()
        acc = check_points(oracle, blur, pts, rec[0], st[0], "sigma 2.0")
        assert 0 < acc.sum() < 200 and {REFINED, OUTSIDE} <= set(int(s) for s in st[0]) <= {REFINED, OUTSIDE, NOT_SADDLE, MOVED}
        d.set_blur_sigma(1.5)  # the same handle back on K1's blur
        d.refine_points_enqueue(dev(frame[None]), dev(pts[None]))
        rec, st = d.refine_points_fetch()
        check_points(oracle, oracle.gaussian_blur_f32(oracle.luma_f32(frame)), pts, rec[0], st[0], "sigma 1.5")
    finally:
        d.close()


# ---- 9. HIP graph ---------------------------------------------------------------------------------------------------------
def test_hip_graph_replays_at_sigma_2(boards):
    """One eager batch, two batches captured, replayed twice: every replay gives the eager run's lists (the front's launches
    are plain kernel nodes; every captured batch clears its own counters)."""
    import torch
    from aprilgrid_rs_amd import sharding
    device = torch.device("cuda", 0)
    frames = [dev(boards), dev(boards[::-1].copy())]
    bufs = [sharding.alloc_result_buffers(3, device) for _ in range(2)]
    d = new_detector(2.0)
    s = torch.cuda.Stream(device)

    def lists(b):
        sd, t = b[0].cpu().numpy(), b[1].cpu().numpy()
        assert (t[:, 2] == 0).all(), t
        return [sd[t[f, 1]: t[f, 1] + t[f, 0]].copy() for f in range(3)]

    try:
        with torch.cuda.stream(s):
            for _ in range(2):  # workspace, both counter sets, stream binding: all before the capture
                for i in range(2):
                    d.saddles_batch_enqueue_to(frames[i], *bufs[i])
        s.synchronize()
        eager = [lists(b) for b in bufs]
        orc = SigmaOracle(2.0)
        for f in range(3):
            ref = orc.refined_saddle_points(boards[f])
            got = np.zeros(len(eager[0][f]), ref.dtype)
            for k, name in enumerate(("x", "y", "k", "theta", "phi")):
                got[name] = eager[0][f][:, k]
            check_saddles(got, ref, "eager frame %d" % f)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(2):
                d.saddles_batch_enqueue_to(frames[i], *bufs[i])
        for rep in range(2):
            for b in bufs:
                b[0].zero_()
                b[1].zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for i in range(2):
                same_lists(lists(bufs[i]), eager[i], "replay %d batch %d" % (rep, i))
        assert d.get_option("last_chain_front") == 1
        del g
    finally:
        torch.cuda.synchronize()
        d.close()


# ---- 10. guard bytes ------------------------------------------------------------------------------------------------------
def test_guard_bytes_stay_intact():
    import aprilgrid_rs_amd as A
    os.environ["AGX_REDZONE_BYTES"] = str(1 << 16)
    try:
        d = A.TagDetector("t36h11", None, device=0)
    finally:
        del os.environ["AGX_REDZONE_BYTES"]
    rng = np.random.default_rng(10)
    try:
        # noise at sigma 0.5 and 8.0 has up to 1870 clusters in a 131 x 97 frame (the helper's count), more than the default
        # capacity of W * H / 8 = 1588: the overflow would be reported, not written -- the lists get room instead
        d.set_limits(max_clusters=4096)
        for w, h in ((67, 45), (33, 70), (131, 97)):
            frames = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
            for sigma in (0.5, 2.0, 8.0):
                d.set_blur_sigma(sigma)
                res = run(d, frames)
                r = d.debug_fetch(0, "redzones")
                assert r["buffers"] >= 20 and r["damaged_bytes"] == 0, (w, h, sigma, r)
                check_saddles(res[1], sigma_oracle.refined_saddle_points(frames[1], sigma)[0], "%dx%d sigma %g" % (w, h, sigma))
    finally:
        d.close()


# ---- 11. group ------------------------------------------------------------------------------------------------------------
def test_group_ranks_follow_their_detectors_sigma(boards):
    import torch
    import aprilgrid_rs_amd as A
    synth = synth_module()
    more = synth.render_batch(70, 3, 320, 240)[0].numpy()
    grp = A.DetectorGroup("t36h11", [0, 0], transport="peer")
    try:
        grp.set_blur_sigma(2.0)
        for r in range(2):
            v = C.c_float(0)
            assert grp._lib.agx_detector_get_blur_sigma(C.c_void_p(grp._lib.agx_group_detector(grp._g, r)), C.byref(v)) == AGX_OK
            assert v.value == 2.0
        per_rank = [dev(boards), dev(more)]
        torch.cuda.synchronize()
        grp.saddles_enqueue(per_rank)
        res, status = grp.saddles_fetch()
        assert (status == 0).all() and len(res) == 6
        orc = SigmaOracle(2.0)
        for i, img in enumerate(list(boards) + list(more)):
            check_saddles(res[i], orc.refined_saddle_points(img), "group frame %d" % i)
    finally:
        grp.close()


# ---- 12. arguments --------------------------------------------------------------------------------------------------------
def test_refused_sigmas_leave_the_value(boards):
    d = new_detector(2.0)
    try:
        want = run(d, boards)
        for bad in (0.0, -1.0, float("nan"), float("inf"), 8.01):
            assert d._lib.agx_detector_set_blur_sigma(d._h, bad) == AGX_ERR_ARG, bad
            assert d.blur_sigma == 2.0
        assert d._lib.agx_detector_get_blur_sigma(d._h, None) == AGX_ERR_ARG
        same_lists(run(d, boards), want, "after the refused values")
        assert d.get_option("last_chain_front") == 1
        d.set_blur_sigma(8.0)  # the largest sigma there is
        assert d.blur_sigma == 8.0
        with pytest.raises(Exception):
            new_detector(-2.0)
    finally:
        d.close()
