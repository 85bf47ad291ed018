"""The homography sampling model on the device: k_positions_homography (agx_decode_positions_enqueue_m) and k_tag_maps
(agx_tag_maps_enqueue) -- reference src/image_util.rs:5-37, :39-70, src/detector.rs:42-72 -- against their host forms byte for byte
(tests/test_tag_homography_cpu.py holds those to the yardstick), the grid-stride loop, the painted perspective tags through the
chained stages, detect_staged(decode_model="homography") against the host composition, and graph capture."""
import numpy as np
import pytest

from tests import homography_oracle as HO
from tests import tag_cases as T
from tests.test_gpu_decode_stages import Guarded, SENT, dev, written

pytestmark = pytest.mark.gpu

DECODED, OUTSIDE, SKIPPED, DEGENERATE = 0, 1, 5, 6
AGX_OK, AGX_ERR_ARG, AGX_ERR_STATE = 0, -1, -7
W, H = T.TAIL_SIZE
MODELS = ("affine", "homography")


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def mixed_quads():
    """[3, 5, 4, 2]: trapezoids of several perspectives, and one quad of each refusal kind: a NaN corner, a corner outside the
    image, a bow-tie, three collinear corners, a concave quad"""
    rng = np.random.default_rng(11)
    q = np.zeros((15, 4, 2), np.float32)
    for i in range(15):
        q[i] = HO.trapezoid(rng.uniform(250, 550), rng.uniform(200, 400), rng.uniform(20, 250), rng.uniform(0.4, 1.0), turn=rng.uniform(0, 6.28),
                            lean=rng.uniform(-0.2, 0.2))
    q[1, 2, 0] = np.nan
    q[3] += np.float32(500)                                     # finite, beyond 800 x 600
    q[6] = q[6][[0, 2, 1, 3]]                                   # a bow-tie
    q[7] = [[100, 100], [150, 100], [200, 100], [150, 180]]     # three collinear corners
    q[8] = [[100, 100], [200, 100], [130, 130], [100, 200]]     # concave
    q[12, 0, 1] = -np.inf
    return q.reshape(3, 5, 4, 2)


def host_positions(quads, counts, pstatus, border, edge, margin, model):
    """-> (points, status, live) of the host form, with AGX_QUAD_SKIPPED where a corner's word is non-zero"""
    import aprilgrid_rs_amd as A
    n, qpf = quads.shape[:2]
    hp, hs = A.decode_positions(quads.reshape(n * qpf, 8), W, H, border, edge, margin, model=model)
    hp, hs = hp.reshape(n, qpf, edge * edge, 2), hs.reshape(n, qpf).copy()
    if pstatus is not None:
        hs[pstatus.reshape(n, qpf, 4).any(axis=2)] = SKIPPED
    return hp, hs, written(counts, qpf, n)


def records_of(quads):
    """The quads as agx_saddle records (stride 20): k, theta, phi are NaN and never read"""
    n, qpf = quads.shape[:2]
    r = np.full((n, 4 * qpf, 5), np.nan, np.float32)
    r[:, :, 0:2] = quads.reshape(n, 4 * qpf, 2)
    return r


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("stride,with_status", [(8, False), (20, False), (20, True)])  # (stride 8 with statuses: the C calls below)
def test_positions_and_maps_equal_the_host_forms(det, model, stride, with_status):
    import aprilgrid_rs_amd as A
    quads = mixed_quads()
    counts = [5, 4, 0]
    d_counts = dev(np.array(counts, np.int32))
    pstatus = None
    if with_status:
        pstatus = np.zeros((3, 20), np.int32)
        pstatus[0, 3], pstatus[1, 19] = 2, 1  # quads (0, 0) and (1, 4): the latter beyond its frame's count
    kw = {"quads": dev(quads)} if stride == 8 else {"refined": (dev(records_of(quads)), dev(pstatus if with_status else np.zeros((3, 20), np.int32)))}
    seen = set()
    for border, edge, margin in ((0, 1, 0.5), (1, 4, 0.0), (2, 5, 1.0), (2, 6, 0.5), (1, 8, 0.5), (0, 6, 0.25)):
        hp, hs, live = host_positions(quads, counts, pstatus, border, edge, margin, model)
        pts, st = Guarded((3, 5, edge * edge, 2), np.float32), Guarded((3, 5), np.uint32)
        det.decode_positions_enqueue(points=pts.t, status=st.t, img_size=(W, H), border_bits=border, edge_bits=edge, margin=margin, counts=d_counts,
                                     model=model, **kw)
        side = 2 * border + edge
        maps, mst = Guarded((3, 5, 9), np.float32), Guarded((3, 5), np.uint32)
        det.tag_maps_enqueue(maps=maps.t, status=mst.t, side_bits=side, margin=margin, model=model, counts=d_counts, **kw)
        det.sync()
        gp, gs = pts.host(), st.host()
        assert np.array_equal(gs[live], hs[live]) and (gs[~live] == SENT).all(), (border, edge, margin, gs, hs)
        ok = live & (hs == DECODED)
        assert gp[ok].tobytes() == hp[ok].tobytes(), (border, edge, margin)
        assert (gp[~ok].view(np.uint32) == SENT).all(), "a slot that is not DECODED, or beyond its frame's count, wrote a point"
        hm, hms = A.tag_maps(quads.reshape(15, 8), side, margin, model)
        hm, hms = hm.reshape(3, 5, 9), hms.reshape(3, 5).copy()
        if pstatus is not None:
            hms[pstatus.reshape(3, 5, 4).any(axis=2)] = SKIPPED
        gm, gms = maps.host(), mst.host()
        assert np.array_equal(gms[live], hms[live]) and (gms[~live] == SENT).all(), (border, edge, margin, gms, hms)
        ok = live & (hms == DECODED)
        assert gm[ok].tobytes() == hm[ok].tobytes() and (gm[~ok].view(np.uint32) == SENT).all(), (border, edge, margin)
        seen |= set(int(s) for s in gs[live]) | set(int(s) for s in gms[live])
    want = {DECODED, OUTSIDE} | ({DEGENERATE} if model == "homography" else set()) | ({SKIPPED} if with_status else set())
    assert seen == want, seen


def test_packed_quads_with_point_statuses_and_refused_arguments(det):
    """Stride 8 with d_point_status through the C calls; an unknown model, side_bits 0 and 41 and a degenerate square are
    AGX_ERR_ARG and leave the batch in flight where it is"""
    import ctypes as C
    import torch
    import aprilgrid_rs_amd as A
    lib, h = det._lib, det._h
    quads = mixed_quads()
    d_quads = dev(quads)
    pstatus = np.zeros((3, 20), np.int32)
    pstatus[0, 3], pstatus[2, 0] = 2, 1
    d_ps = dev(pstatus)
    pts, st = Guarded((3, 5, 36, 2), np.float32), Guarded((3, 5), np.uint32)
    maps, mst = Guarded((3, 5, 9), np.float32), Guarded((3, 5), np.uint32)
    P = lambda t: t.data_ptr()
    det._follow_torch_stream(d_quads)
    good_pos = [P(d_quads), 8, 3, 5, None, P(d_ps), W, H, 2, 6, C.c_float(0.5), P(pts.t), P(st.t), 1]
    good_map = [P(d_quads), 8, 3, 5, None, P(d_ps), 10, C.c_float(0.5), 1, P(maps.t), P(mst.t)]
    assert lib.agx_decode_positions_enqueue_m(h, *good_pos) == AGX_OK and lib.agx_tag_maps_enqueue(h, *good_map) == AGX_OK
    det.sync()
    hp, hs, _ = host_positions(quads, None, pstatus, 2, 6, 0.5, "homography")
    gp, gs = pts.host(), st.host()
    assert np.array_equal(gs, hs) and gp[hs == DECODED].tobytes() == hp[hs == DECODED].tobytes() and (gp[hs != DECODED].view(np.uint32) == SENT).all()
    assert gs[0, 0] == SKIPPED and gs[2, 0] == SKIPPED
    hm, hms = A.tag_maps(quads.reshape(15, 8), 10, 0.5, "homography")
    hms = hms.reshape(3, 5).copy()
    hms[pstatus.reshape(3, 5, 4).any(axis=2)] = SKIPPED
    assert np.array_equal(mst.host(), hms) and maps.host()[hms == DECODED].tobytes() == hm.reshape(3, 5, 9)[hms == DECODED].tobytes()
    # refusals, with a saddle batch in flight
    frames = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    det.saddles_batch_enqueue(frames)
    bad_pos = {"model 2": {13: 2}, "model -1": {13: -1}, "edge 9": {9: 9}, "degenerate square": {8: 0, 9: 1, 10: C.c_float(0.0)}, "null points": {11: None},
               "stride 6": {1: 6}}
    bad_map = {"model 2": {8: 2}, "side 0": {6: 0}, "side 41": {6: 41}, "degenerate square": {6: 1, 7: C.c_float(0.0)}, "margin nan": {7: C.c_float(float("nan"))},
               "null maps": {9: None}, "misaligned maps": {9: P(maps.t) + 2}, "no frames": {2: 0}, "no quads per frame": {3: 0}, "stride 4": {1: 4},
               "2^29 slots": {2: 1 << 15, 3: 1 << 14}}
    for fn, good, bad in ((lib.agx_decode_positions_enqueue_m, good_pos, bad_pos), (lib.agx_tag_maps_enqueue, good_map, bad_map)):
        for what, change in bad.items():
            a = list(good)
            for i, v in change.items():
                a[i] = v
            assert fn(h, *a) == AGX_ERR_ARG, what
        assert fn(None, *good) == AGX_ERR_ARG
    res, fst = det.saddles_batch_fetch()  # still in flight
    assert len(res) == 2 and (fst == 0).all()
    for fn, good in ((lib.agx_decode_positions_enqueue_m, good_pos), (lib.agx_tag_maps_enqueue, good_map)):
        det.saddles_batch_enqueue(frames)
        assert fn(h, *good) == AGX_OK  # replaces the batch, has nothing to fetch
        assert lib.agx_decode_quads_fetch(h, None, None, None) == AGX_ERR_STATE
    det.sync()


@pytest.mark.parametrize("model", MODELS)
def test_the_grid_stride_loop(det, model):
    """One frame of 40 000 quads: past 2048 workgroups x 16 slots, so every row takes a second turn"""
    import aprilgrid_rs_amd as A
    base = mixed_quads().reshape(15, 4, 2)
    n = 40000
    quads = np.ascontiguousarray(base[np.arange(n) % 15]).reshape(1, n, 4, 2)
    d_quads = dev(quads)
    pts, st = Guarded((1, n, 36, 2), np.float32), Guarded((1, n), np.uint32)
    maps, mst = Guarded((1, n, 9), np.float32), Guarded((1, n), np.uint32)
    det.decode_positions_enqueue(d_quads, pts.t, st.t, img_size=(W, H), model=model)
    det.tag_maps_enqueue(d_quads, maps.t, mst.t, side_bits=10, margin=0.5, model=model)
    det.sync()
    hp, hs = A.decode_positions(base.reshape(15, 8), W, H, 2, 6, 0.5, model=model)
    hm, hms = A.tag_maps(base.reshape(15, 8), 10, 0.5, model)
    idx = np.arange(n) % 15
    gp, gs, gm, gms = pts.host()[0], st.host()[0], maps.host()[0], mst.host()[0]
    assert np.array_equal(gs, hs[idx]) and np.array_equal(gms, hms[idx])
    ok = gs == DECODED
    assert gp[ok].tobytes() == hp[idx][ok].tobytes() and (gp[~ok].view(np.uint32) == SENT).all()
    ok = gms == DECODED
    assert gm[ok].tobytes() == hm.reshape(15, 9)[idx][ok].tobytes() and (gm[~ok].view(np.uint32) == SENT).all()


def test_painted_perspective_tags_through_the_chained_stages():
    """decode_positions_enqueue(model="homography") -> bit_code_enqueue -> best_tag_enqueue with no sync in between: the painted
    ids at the four rotations of the quad, handed on to collect_tags_enqueue; decode_quads_staged(model="affine") stays the
    fused kernel's result"""
    import torch
    import aprilgrid_rs_amd as A
    i32 = dict(dtype=torch.int32, device="cuda")
    for fam in T.FAMILIES:
        plane, _, quad, code = HO.painted_case(fam)
        edge, border, thres, _ = T.family(fam)
        quads = np.stack([np.roll(quad, -r, axis=0) for r in range(4)]).reshape(1, 4, 4, 2)
        d_plane, d_quads = dev(plane[None]), dev(quads)
        d = A.TagDetector(fam, None, device=0)
        try:
            pts, st, bits = Guarded((1, 4, edge * edge, 2), np.float32), Guarded((1, 4), np.uint32), Guarded((1, 4), np.uint64)
            ids, rots, tags = Guarded((1, 4), np.uint32), Guarded((1, 4), np.uint32), Guarded((1, 4, 9), np.uint32)
            d.decode_positions_enqueue(d_quads, pts.t, st.t, img_size=(W, H), model="homography")
            d.bit_code_enqueue(d_plane, pts.t, bits.t, st.t, status_in=st.t)
            d.best_tag_enqueue(bits.t, ids.t, rots.t, st.t, status_in=st.t, quads=d_quads, tags=tags.t)
            # one board of four "quads" whose saddle numbers are all different: every decoded quad takes or keeps a row
            bq = dev(np.arange(16, dtype=np.int32).reshape(1, 4, 4))
            tt, nt, ts = torch.zeros((1, 8, 9), **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
            d.collect_tags_enqueue(bq, dev(np.array([4], np.int32)), dev(np.zeros(1, np.int32)), tags.t, st.t, None, tt, nt, ts, reset=True,
                                   saddles_per_frame=16)
            d.sync()
            assert (st.host() == DECODED).all() and (ids.host() == code).all() and sorted(rots.host()[0]) == [0, 1, 2, 3], (fam, st.host(), ids.host())
            hp, hs = A.decode_positions(quads.reshape(4, 8), W, H, border, edge, 0.5, model="homography")
            assert pts.host().tobytes() == hp.tobytes()
            hb, hs = A.bit_code(plane, hp, 10, 3, status_in=hs)
            _, _, _, ht = A.best_tag(hb, thres, tag_family=fam, status_in=hs, quads=quads.reshape(4, 8))
            assert tags.host().tobytes() == ht.tobytes() and bits.host().tobytes() == hb.tobytes()
            assert int(nt.cpu()[0]) == 1 and int(ts.cpu()[0]) == 0 and int(tt.cpu()[0, 0, 0]) == code
            assert tt.cpu().numpy()[0, 0].tobytes() == tags.host()[0, 3].tobytes()  # the last quad's corners stay
            # the existing path, untouched: the staged chain at affine is the fused kernel, and neither decodes the painted id
            d.decode_quads_enqueue(d_plane, d_quads)
            ftags, fst, fbits = d.decode_quads_fetch()
            stags, sst, sbits, _ = d.decode_quads_staged(d_plane, d_quads, model="affine")
            assert stags.tobytes() == ftags.tobytes() and np.array_equal(sst, fst) and np.array_equal(sbits, fbits)
            assert all(s != DECODED or t["id"] != code for s, t in zip(fst[0], ftags[0]))
            htags, hst, _, _ = d.decode_quads_staged(d_plane, d_quads, model="homography")
            assert (hst == DECODED).all() and htags.tobytes() == ht.tobytes()
        finally:
            d.close()


def test_detect_staged_with_the_homography_equals_the_host_composition(det):
    """Four synthetic frames: the result equals find_board_tail -> decode_positions(model="homography") -> bit_code -> best_tag ->
    collect_tags per round on the device's own filtered saddle lists.  (Nothing is claimed against the affine result.)"""
    import aprilgrid_rs_amd as A
    from tests.test_collect_tags_cpu import N_CODES, TAG, T_OK
    from tests.test_gpu_collect_tags import SH, SW, stages_for_the_host_loop
    from tests.util import bits_equal, synth_module
    frames, _ = synth_module().render_batch(40, 4, SW, SH, device="cuda")
    got = det.detect_staged(frames, decode_model="homography")
    _, records, words, counts = stages_for_the_host_loop(det, frames)
    host = frames.cpu().numpy()
    edge, border, thres, _ = det._family_info()
    rounds = det.detector_params.max_num_of_boards
    for f in range(4):
        c = int(counts[f])
        rec = np.ascontiguousarray(records[f, :c], np.float32).view(A.SADDLE_DTYPE).reshape(-1)
        w = np.array(words[f, :c], np.uint32)
        luma = A.TagDetector.luma8(host[f])
        tags, n_tags, status = None, 0, T_OK
        for _ in range(rounds):
            listed = np.flatnonzero(w == 0)
            quads, bstatus, _n = A.find_board_tail(rec[listed], cap=1024)
            quads = listed[quads.astype(np.int64)].astype(np.uint32).reshape(-1, 4)
            if len(quads):
                pts = np.stack([rec["x"][quads], rec["y"][quads]], axis=-1)
                hp, hs = A.decode_positions(pts, SW, SH, border, edge, 0.5, model="homography")
                hb, hs = A.bit_code(luma, hp, 10, 3, status_in=hs)
                _, _, qstatus, qtags = A.best_tag(hb, thres, tag_family="t36h11", status_in=hs, quads=pts)
            else:
                qtags, qstatus = np.zeros(0, TAG), np.zeros(0, np.uint32)
            tags, n_tags, status, w = A.collect_tags("t36h11", quads, bstatus, qtags, qstatus, len(w), w, tags, n_tags, status, N_CODES)
        assert status == T_OK and n_tags > 4
        rows = tags[:n_tags]
        assert list(got[f]) == [int(t) for t in rows["id"]], "frame %d: ids or their order" % f
        for i, t in enumerate(got[f]):
            assert bits_equal(got[f][t], rows["xy"][i].reshape(4, 2)), "frame %d: corners of tag %d" % (f, t)


@pytest.mark.parametrize("model", MODELS)
def test_an_m_batch_can_be_captured_into_a_graph(model):
    import torch
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    try:
        d_quads = dev(mixed_quads())
        pts, st = Guarded((3, 5, 36, 2), np.float32), Guarded((3, 5), np.uint32)
        with torch.cuda.stream(s):
            for _ in range(2):  # the stream binding: before the capture
                d.decode_positions_enqueue(d_quads, pts.t, st.t, img_size=(W, H), model=model)
        s.synchronize()
        eager = (pts.host(), st.host())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d.decode_positions_enqueue(d_quads, pts.t, st.t, img_size=(W, H), model=model)
        pts.raw.fill_(SENT), st.raw.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert pts.host().tobytes() == eager[0].tobytes() and st.host().tobytes() == eager[1].tobytes()
        assert (eager[1] == DECODED).sum() >= 8
        del g
    finally:
        torch.cuda.synchronize()
        d.close()
