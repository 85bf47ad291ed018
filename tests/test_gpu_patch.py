"""The saddle chain and detect at a half_size_patch other than the reference's 2 (agx_detector_set_half_size_patch): flood
stages that only cluster, k_generic_cluster, k_refine_clusters<half> and the unchanged emission, against tests/patch_oracle.py --
the reference's refined_saddle_points composed from the oracle's pieces with the half in place of the 2 of src/detector.rs:430
(and a sigma in place of the 1.5 of :410), which tests/test_patch_cpu.py holds to the oracle's own chain at (1.5, 2).  The bar is
the chain's (tests/test_gpu_parity.py): planes, minima, cluster tables, centroids and x / y / k bit for bit, theta / phi within
tests.util.ANGLE_TOL_DEG, the unfiltered refine output included."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import patch_oracle
from tests.util import check_frame, check_saddles, check_tags, load_image, synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
L8, L16, RGB8 = 0, 1, 2
GENERIC_PATH, LARGE_RESULT = 16, 64  # AGX_FRAME_*

_SEEN = {}  # the helper's answers, computed once per (sigma, half, image) for the whole module


class PatchOracle:
    """What tests.util.check_frame asks of the oracle module, answered by the helper at one (sigma, half)."""

    def __init__(self, sigma, half):
        self.sigma, self.half = sigma, half

    def refined_saddle_points(self, img, params=None, debug=False):
        key = (float(self.sigma), self.half, img.shape, img.dtype.str, img.tobytes())
        if key not in _SEEN:
            _SEEN[key] = patch_oracle.refined_saddle_points(img, self.sigma, self.half, params)
        ref, d = _SEEN[key]
        return (ref, d) if debug else ref


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


def new_detector(sigma=None, half=None, **options):
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0, blur_sigma=sigma, half_size_patch=half)
    for k, v in options.items():
        d.set_option(k, v)
    return d


@pytest.fixture(scope="module")
def det():
    """One handle for the sweeps: it alternates between halves, sigmas and sizes."""
    d = new_detector()
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


def run_to(d, frames):
    """-> (lists, frame table) through caller-owned device buffers."""
    from aprilgrid_rs_amd import sharding
    import torch
    bufs = sharding.alloc_result_buffers(len(frames), torch.device("cuda", 0))
    d.saddles_batch_enqueue_to(dev(frames), *bufs)
    d.sync()
    sd, t = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    return [sd[t[f, 1]: t[f, 1] + t[f, 0]].copy() for f in range(len(frames))], t


def same_lists(a, b, what):
    assert len(a) == len(b), what
    for i in range(len(a)):
        assert a[i].tobytes() == b[i].tobytes(), "%s: frame %d" % (what, i)


# ---- 1. sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1.5, 3.0])
@pytest.mark.parametrize("half", [1, 3, 4])
def test_sweep(det, boards, half, sigma):
    orc = PatchOracle(sigma, half)
    det.set_blur_sigma(sigma)
    det.set_half_size_patch(half)
    assert det.half_size_patch == half
    res = run(det, boards)
    assert det.get_option("last_chain_refine") == 1 and det.get_option("last_chain_front") == (0 if sigma == 1.5 else 1)
    for i in range(3):
        ref = check_frame(det, orc, boards[i], i, "half %d sigma %g frame %d" % (half, sigma, i))
        check_saddles(res[i], ref, "half %d sigma %g frame %d" % (half, sigma, i))
        assert len(ref) >= 1
    if sigma == 1.5:
        assert tuple(len(r) for r in res) == {1: (202, 173, 192), 3: (161, 137, 151), 4: (151, 96, 147)}[half]
    img = load_image("EuRoC.png")
    got = det.refined_saddle_points(img, as_array=True)
    assert det.get_option("last_chain_refine") == 1
    ref = check_frame(det, orc, img, 0, "EuRoC.png at half %d sigma %g" % (half, sigma))
    check_saddles(got, ref, "EuRoC.png at half %d sigma %g" % (half, sigma))
    assert len(ref) >= 2


# ---- 2. half 2 on both paths ----------------------------------------------------------------------------------------------
def test_half_2_on_both_paths(boards):
    d = new_detector()
    try:
        assert d.half_size_patch == 2 and d.get_option("chain_refine_general") == 0
        d.set_option("chain_refine_general", 1)
        lists1, table1 = run_to(d, boards)
        assert d.get_option("last_chain_refine") == 1
        d.set_option("chain_refine_general", 0)
        lists0, table0 = run_to(d, boards)
        assert d.get_option("last_chain_refine") == 0
        same_lists(lists1, lists0, "chain_refine_general 1 against 0")
        assert (table0[:, 2] == 0).all() and np.array_equal(table1[:, [0, 2, 3]], table0[:, [0, 2, 3]])  # count, status, clusters
        assert sorted(table1[:, 1]) in ([0, 157, 334], [0, 157, 335], [0, 177, 334], [0, 177, 355], [0, 178, 335], [0, 178, 355])  # (lists packed in completion order)
        orc = PatchOracle(1.5, 2)
        for i in range(3):
            assert len(lists0[i]) == len(orc.refined_saddle_points(boards[i]))
        # one handle through 3, 2, 4, 2: every batch is a fresh handle's
        for n, half in enumerate((3, 2, 4, 2)):
            d.set_half_size_patch(half)
            got = run(d, boards)
            assert d.get_option("last_chain_refine") == (0 if half == 2 else 1)
            orc = PatchOracle(1.5, half)
            for i in range(3):
                check_saddles(got[i], check_frame(d, orc, boards[i], i, "step %d half %d frame %d" % (n, half, i)), "step %d half %d frame %d" % (n, half, i))
    finally:
        d.close()


# ---- 3. launch paths ------------------------------------------------------------------------------------------------------
def test_launch_paths_at_half_3(boards):
    orc = PatchOracle(1.5, 3)
    first = None
    for option, value in (("sparse_path", 1), ("sparse_path", 2), ("sparse_path", 3), ("force_generic", 1)):
        d = new_detector(None, 3, **{option: value})
        try:
            res = run(d, boards)
            assert d.get_option("last_chain_refine") == 1 and d.get_option("last_sparse_path") == 1
            if option == "sparse_path":
                assert d.get_option("sparse_path") == value
            for i in range(3):
                check_saddles(res[i], check_frame(d, orc, boards[i], i, "%s %d frame %d" % (option, value, i)), "%s %d frame %d" % (option, value, i))
            if first is None:
                first = res
            same_lists(res, first, "%s %d" % (option, value))
        finally:
            d.close()


# ---- 4. the generic path by itself ----------------------------------------------------------------------------------------
def test_generic_path_at_sigma_6_half_4(boards):
    orc = PatchOracle(6.0, 4)
    d = new_detector(6.0, 4)
    try:
        res = run(d, boards)
        assert d.get_option("last_chain_refine") == 1
        for i in range(3):
            check_saddles(res[i], check_frame(d, orc, boards[i], i, "frame %d" % i), "frame %d" % i)
        assert int(orc.refined_saddle_points(boards[0], debug=True)[1]["sizes"].max()) == 7756
        assert d.debug_fetch(0, "counters")["flags"] & GENERIC_PATH
        assert len(res[0]) == 1 and len(res[2]) == 0
        lists, table = run_to(d, boards)
        assert table[0, 2] & GENERIC_PATH and table[0, 0] == 1 and table[2, 0] == 0 and not (table[:, 2] & 7).any()
        assert table[2, 2] == 0
    finally:
        d.close()


# ---- 5. large lists -------------------------------------------------------------------------------------------------------
def test_large_lists_at_half_1():
    """Pure noise at 4 : 3 sizes in steps of 16 columns: 320 x 240 has 997 unfiltered records at half 1, 336 x 252 has 1091 --
    the smallest of them beyond the 1024 records that the emission ranks in one pass."""
    synth = synth_module()
    below = synth.render_batch(0, 1, 320, 240, pure_noise=True)[0].numpy()[0]
    frame = synth.render_batch(0, 1, 336, 252, pure_noise=True)[0].numpy()[0]
    orc = PatchOracle(1.5, 1)
    assert len(orc.refined_saddle_points(below, debug=True)[1]["refined"]) == 997
    assert len(orc.refined_saddle_points(frame, debug=True)[1]["refined"]) == 1091
    d = new_detector(None, 1)
    try:
        res = run(d, frame[None])
        ref = check_frame(d, orc, frame, 0, "336 x 252 noise")
        check_saddles(res[0], ref, "336 x 252 noise")
        assert d.debug_fetch(0, "counters")["flags"] & LARGE_RESULT and len(ref) == 954
        res = run(d, np.stack([frame, frame]))  # (several workgroups per frame emit the list together)
        for i in range(2):
            check_saddles(res[i], ref, "336 x 252 noise twice, frame %d" % i)
            assert d.debug_fetch(i, "counters")["flags"] & LARGE_RESULT
    finally:
        d.close()


# ---- 6. small and awkward sizes -------------------------------------------------------------------------------------------
def padded_batch(px, row_pad, frame_pad, offset):
    n, h, rb = px.shape
    rs = rb + row_pad
    fs = h * rs + frame_pad
    buf = np.full(offset + n * fs + 64, 0xEE, np.uint8)
    for f in range(n):
        for y in range(h):
            o = offset + f * fs + y * rs
            buf[o:o + rb] = px[f, y]
    return buf, offset, rs, fs


@pytest.mark.parametrize("half", [1, 4])
def test_small_and_awkward_sizes(det, half):
    import torch
    synth = synth_module()
    orc = PatchOracle(1.5, half)
    det.set_blur_sigma(1.5)
    det.set_half_size_patch(half)
    for w, h in ((2, 2), (5, 7), (16, 12), (17, 17), (33, 31), (64, 48)):
        frames = synth.render_batch(0, 3, w, h)[0].numpy()
        buf, off, rs, fs = padded_batch(frames, 3, 7, 1)  # unaligned rows, frames and base
        t = torch.from_numpy(buf).cuda()
        det.saddles_batch_enqueue_ptr(t.data_ptr() + off, 3, w, h, rs, fs, L8)
        res, status = det.saddles_batch_fetch()
        assert (status == 0).all() and det.get_option("last_chain_refine") == 1
        for i in range(3):
            ref = check_frame(det, orc, frames[i], i, "%dx%d half %d frame %d" % (w, h, half, i))
            check_saddles(res[i], ref, "%dx%d half %d frame %d" % (w, h, half, i))
            if w < 4 * half + 1 or h < 4 * half + 1:
                assert len(res[i]) == 0
        if (w, h) == (64, 48) and half == 4:
            c = orc.refined_saddle_points(frames[0], debug=True)[1]["centers"]
            rx, ry = np.round(c[:, 0]), np.round(c[:, 1])
            assert len(c) == 79 and int(((rx < 8) | (rx > w - 9) | (ry < 8) | (ry > h - 9)).sum()) == 20 and len(res[0]) == 3


# ---- 7. guard bytes -------------------------------------------------------------------------------------------------------
def test_guard_bytes_stay_intact(boards):
    import aprilgrid_rs_amd as A
    os.environ["AGX_REDZONE_BYTES"] = str(1 << 16)
    try:
        d = A.TagDetector("t36h11", None, device=0, half_size_patch=4)
    finally:
        del os.environ["AGX_REDZONE_BYTES"]
    try:
        orc = PatchOracle(1.5, 4)
        c = orc.refined_saddle_points(boards[2], debug=True)[1]["centers"]
        rx, ry = np.round(c[:, 0]), np.round(c[:, 1])
        assert int(((rx < 8) | (rx > 320 - 9) | (ry < 8) | (ry > 240 - 9)).sum()) == 24  # clusters whose window leaves the frame
        res = run(d, boards)
        r = d.debug_fetch(0, "redzones")
        assert r["buffers"] >= 20 and r["damaged_bytes"] == 0, r
        for i in range(3):
            check_saddles(res[i], orc.refined_saddle_points(boards[i]), "frame %d" % i)
        small = synth_module().render_batch(0, 3, 64, 48)[0].numpy()  # 20 of frame 0's 79 clusters at the border
        res = run(d, small)
        r = d.debug_fetch(0, "redzones")
        assert r["damaged_bytes"] == 0, r
        check_saddles(res[0], orc.refined_saddle_points(small[0]), "64 x 48")
    finally:
        d.close()


# ---- 8. detect ------------------------------------------------------------------------------------------------------------
def test_detect_at_sigma_3_half_3(oracle):
    img = load_image("EuRoC.png")
    saddles = PatchOracle(3.0, 3).refined_saddle_points(img)
    want = oracle.detect_tail(oracle.luma_u8(img), saddles)
    assert len(want) == 26
    d = new_detector(3.0, 3)
    try:
        check_tags(d.detect(img), want, "agx_detect")
        assert d.get_option("last_chain_refine") == 1
        for tail in (0, 1):
            try:
                d.set_option("device_tail", tail)
            except Exception as e:
                if tail == 1 and getattr(e, "status", None) == AGX_ERR_STATE:
                    continue  # the device tail is not offered where this process's atan2f differs: nothing to run
                raise
            d.detect_batch_enqueue(dev(img[None]))
            got = d.detect_batch_fetch()
            assert len(got) == 1 and d.get_option("last_chain_refine") == 1
            check_tags(got[0], want, "agx_detect_batch_enqueue, device_tail %d" % tail)
    finally:
        d.close()


# ---- 9. formats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["RGB8", "L16"])
def test_formats_at_half_3(name):
    synth = synth_module()
    rng = np.random.default_rng(11)
    grey = np.stack([np.asarray(synth.render_frame(60 + i, 320, 240)[0]) for i in range(3)])
    if name == "L16":
        px = (grey.astype(np.uint16) * 257 + rng.integers(0, 60, grey.shape).astype(np.uint16)).astype(np.uint16)
        fmt = L16
    else:
        px = np.stack([np.clip(grey.astype(np.int64) + d + rng.integers(-2, 3, grey.shape), 0, 255).astype(np.uint8) for d in (-3, 0, 4)], -1)
        fmt = RGB8
    orc = PatchOracle(1.5, 3)
    d = new_detector(None, 3)
    try:
        res = run(d, px, fmt)
        assert d.get_option("last_chain_refine") == 1
        for i in range(3):
            ref = check_frame(d, orc, np.ascontiguousarray(px[i]), i, "%s frame %d" % (name, i))
            check_saddles(res[i], ref, "%s frame %d" % (name, i))
            assert len(ref) > 50
    finally:
        d.close()


# ---- 10. HIP graph --------------------------------------------------------------------------------------------------------
def test_hip_graph_replays_at_half_3(boards):
    """One eager batch (workspace, counter sets, the refine constants), two batches captured, replayed twice: every replay
    gives the eager run's lists."""
    import torch
    from aprilgrid_rs_amd import sharding
    device = torch.device("cuda", 0)
    frames = [dev(boards), dev(boards[::-1].copy())]
    bufs = [sharding.alloc_result_buffers(3, device) for _ in range(2)]
    d = new_detector(None, 3)
    s = torch.cuda.Stream(device)

    def lists(b):
        sd, t = b[0].cpu().numpy(), b[1].cpu().numpy()
        assert (t[:, 2] == 0).all(), t
        return [sd[t[f, 1]: t[f, 1] + t[f, 0]].copy() for f in range(3)]

    try:
        with torch.cuda.stream(s):
            for _ in range(2):
                for i in range(2):
                    d.saddles_batch_enqueue_to(frames[i], *bufs[i])
        s.synchronize()
        eager = [lists(b) for b in bufs]
        orc = PatchOracle(1.5, 3)
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
        assert d.get_option("last_chain_refine") == 1
        del g
    finally:
        torch.cuda.synchronize()
        d.close()


# ---- 11. group ------------------------------------------------------------------------------------------------------------
def test_group_ranks_follow_their_detectors_half(boards):
    import torch
    import aprilgrid_rs_amd as A
    more = synth_module().render_batch(70, 3, 320, 240)[0].numpy()
    grp = A.DetectorGroup("t36h11", [0, 0], transport="peer")
    try:
        halves = (2, 4)
        for r in range(2):
            h = C.c_void_p(grp._lib.agx_group_detector(grp._g, r))
            assert grp._lib.agx_detector_set_half_size_patch(h, halves[r]) == AGX_OK
            v = C.c_int(0)
            assert grp._lib.agx_detector_get_half_size_patch(h, C.byref(v)) == AGX_OK and v.value == halves[r]
        per_rank = [dev(boards), dev(more)]
        torch.cuda.synchronize()
        grp.saddles_enqueue(per_rank)
        res, status = grp.saddles_fetch()
        assert (status == 0).all() and len(res) == 6
        for i, img in enumerate(list(boards) + list(more)):
            check_saddles(res[i], PatchOracle(1.5, halves[i // 3]).refined_saddle_points(img), "group frame %d" % i)
    finally:
        grp.close()


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------
def test_refused_values_and_what_is_not_governed(oracle, boards):
    d = new_detector(None, 4)
    try:
        for bad in (0, 5, -1):
            assert d._lib.agx_detector_set_half_size_patch(d._h, bad) == AGX_ERR_ARG, bad
            assert d.half_size_patch == 4
        assert d._lib.agx_detector_get_half_size_patch(d._h, None) == AGX_ERR_ARG
        with pytest.raises(Exception):
            new_detector(None, 5)
        # the half set between enqueue and fetch: the batch in flight is the one that was enqueued
        d.saddles_batch_enqueue(dev(boards))
        d.set_half_size_patch(1)
        res, status = d.saddles_batch_fetch()
        assert (status == 0).all()
        for i in range(3):
            check_saddles(res[i], PatchOracle(1.5, 4).refined_saddle_points(boards[i]), "in flight, frame %d" % i)
        d.set_half_size_patch(4)
        # agx_refine_points_enqueue is not governed: it refines at 2
        from tests.test_gpu_refine_points import check_points
        _, dd = PatchOracle(1.5, 2).refined_saddle_points(boards[0], debug=True)
        pts = np.ascontiguousarray(dd["centers"][:200], np.float32)
        d.refine_points_enqueue(dev(boards[:1]), dev(pts[None]))
        rec, st = d.refine_points_fetch()
        acc = check_points(oracle, dd["blur"], pts, rec[0], st[0], "refine_points on a handle at chain half 4")
        assert acc.sum() > 20
        assert d.half_size_patch == 4
    finally:
        d.close()
