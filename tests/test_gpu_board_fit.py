"""agx_board_fit_enqueue (k_board_fit) on the GPU: every output array against the host form agx_board_fit_tail byte for byte, FILL
bytes beyond and between what a frame may write included (tests/test_board_fit_cpu.py holds the host form to a numpy float64
lstsq fit); the table shapes at which the kernel's lane stride, its frames per workgroup and its LDS staging turn over; the
chain detect -> fit -> snap with nothing but the stream between; the batch state and the refused arguments; TagDetector.detect_recovered
and recover_tags_enqueue against their restatement over the host forms (tests/board_fit_cases.py: recovered_host)."""
import numpy as np
import pytest

from tests import board_fit_cases as BC
from tests.board_fit_cases import FEW, INPUT, LOOSE, OK, SINGULAR, Batch, cases

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

pytestmark = pytest.mark.gpu

FRAMES_PER_WG = 2  # csrc/board_fit.h: FIT_FRAMES_PER_WG
MISSING = _ffi.AGX_FIT_PREDICT_MISSING
KEYS = ("h", "err_sq", "row_status", "n_inliers", "rms", "pred", "n_pred", "status")


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_outputs(det, b):
    """b's frames through agx_board_fit_enqueue into the same FILL-filled arrays the host form is given -> those arrays."""
    import torch
    host = b.empty_outputs()
    d = {k: dev(v.view(np.int32).reshape(v.shape[0], -1, 9) if k == "pred" else v) for k, v in host.items()}
    table = dev(b.table().view(np.int32).reshape(b.n, b.tpf, 9))
    counts = dev(np.array(b.counts, np.int32))
    st = None if b.tag_status is None else dev(np.array(b.tag_status, np.int32))
    n = b.n
    det.board_fit_enqueue(table, counts, b.cols, b.rows, b.size, d["h"][:n], d["err_sq"][:n], d["row_status"][:n], d["n_inliers"][:n], d["rms"][:n],
                          d["pred"][:n], d["n_pred"][:n], d["status"][:n], first_id=b.first_id, spacing_ratio=b.s, max_err_sq=b.max_err_sq,
                          max_drop=b.max_drop, min_tags=b.min_tags, predict_missing=bool(b.flags & MISSING), tag_status=st)
    det.sync()
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in KEYS}


def same_bytes(det, b):
    want, got = b.host(), device_outputs(det, b)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), "%s: %s differs from the host form" % (b.name, k)
    return want


@pytest.mark.parametrize("name", sorted(cases()))
def test_every_cpu_case_gives_the_host_forms_bytes(det, name):
    same_bytes(det, cases()[name])


def five_statuses():
    t = cases()["frame0"].tables[0]
    two = cases()["two_wrong_drop1"].tables[0]
    flat = cases()["four_equal_corners"].tables[0]
    bad = cases()["on_board_nan"].tables[0]
    return [t, two, t[:0], flat, bad, t[:13]], [OK, LOOSE, FEW, SINGULAR, INPUT, OK]


def test_one_launch_with_all_five_frame_statuses(det):
    tables, status = five_statuses()
    for flags in (0, MISSING):
        want = same_bytes(det, Batch("mixed", tables, 7, 4, (800, 600), max_drop=1, flags=flags, tpf=40))
        assert want["status"][:6].tolist() == status and BC.untouched(want["status"][6:])
        for f in (2, 3, 4):  # refused in the middle of the batch: their slices stay FILL
            assert all(BC.untouched(want[k][f]) for k in ("h", "err_sq", "row_status", "rms", "pred"))


def big_table(n_on, n_off, cols=24, rows=24, size=(1280, 800), first_id=3, s=0.3):
    """n_on tags of the 24 x 24 layout under a tilted pose with 0.05 px of noise, n_off rows with ids beyond it in between."""
    rng = np.random.RandomState(5)
    ids = rng.permutation(cols * rows)[:n_on]
    t = BC.exact_table(cols, rows, ids, BC.pose(cols, rows, size, s=s, tilt=0.01), first_id=first_id, s=s, noise=0.05)
    off = BC.exact_table(cols, rows, range(n_off), BC.pose(cols, rows, size, s=s), first_id=first_id, s=s)
    off["id"] = BC.wrapped_ids(first_id, cols * rows + np.arange(n_off))
    out = np.concatenate([t, off])
    return out[rng.permutation(len(out))]


@pytest.mark.parametrize("tpf", (1, 63, 64, 65, 587))
def test_rows_per_frame_around_the_lane_stride_and_at_the_largest_family(det, tpf):
    full = big_table(min(tpf, 576), max(tpf - 576, 0))
    assert len(full) == tpf
    tables = [full, full[:tpf // 2], full[:max(tpf - 1, 0)]]
    want = same_bytes(det, Batch("tpf%d" % tpf, tables, 24, 24, (1280, 800), first_id=3, max_drop=2, flags=MISSING, tpf=tpf))
    assert want["status"][0] == OK and want["n_inliers"][0] == min(tpf, 576) and want["n_pred"][0] == 576 - min(tpf, 576)


@pytest.mark.parametrize("tpf", (65, 587))
def test_a_wrapping_id_window_across_several_passes_of_64_tags(det, tpf):
    """The 24 x 24 layout from 0xFFFFFF00 at spacing ratio 1: its 576 ids pass 2^32 after 256 tags, so the member bitmap in LDS
    and the ballot compaction of pred run on wrapped ids over nine passes of 64 tags; at 587 rows the 11 off-board ids follow the
    window's wrapped end."""
    first = 0xFFFFFF00
    full = big_table(min(tpf, 576), max(tpf - 576, 0), first_id=first, s=1.0)
    assert len(full) == tpf and full["id"].max() >= first and full["id"].min() < 576 - 256
    tables = [full, full[:tpf // 2], full[:tpf - 1]]
    want = same_bytes(det, Batch("wrap_tpf%d" % tpf, tables, 24, 24, (1280, 800), first_id=first, s=1.0, max_drop=2, flags=MISSING, tpf=tpf))
    n_on = min(tpf, 576)
    assert want["status"][0] == OK and want["n_inliers"][0] == n_on and want["n_pred"][0] == 576 - n_on
    assert (want["row_status"][0] == BC.OFF_BOARD).sum() == tpf - n_on
    have = set(full["id"].tolist())
    assert want["pred"][0, :576 - n_on]["id"].tolist() == [i for i in BC.wrapped_ids(first, np.arange(576)).tolist() if i not in have]


@pytest.mark.parametrize("n", (1, 3, 2 * FRAMES_PER_WG + 1))
def test_frame_counts_around_the_frames_of_a_workgroup(det, n):
    full = big_table(576, 0)
    tables = [full[:576 - 37 * f] for f in range(n)]
    tables[-1] = BC.swap_id(tables[-1], 4, int(tables[-1]["id"][9]))  # the last frame, alone in its workgroup, has a wrong id to drop
    want = same_bytes(det, Batch("frames%d" % n, tables, 24, 24, (1280, 800), first_id=3, max_drop=1, tpf=576))
    assert (want["status"][:n] == OK).all() and want["n_inliers"][n - 1] == len(tables[-1]) - 1


def test_detect_feeds_the_fit_feeds_the_snap_on_one_stream(det):
    import torch
    from oracle import oracle as O
    img, gt, tags, (w, h, rows, cols) = BC.frame(0)
    n, cap, nb = 3, 64, rows * cols
    frames = dev(np.stack([img] * n))
    lists = O.refined_saddle_points(img)
    rec = np.ascontiguousarray(lists).view(np.float32).reshape(-1, 5)
    saddles, scounts = dev(np.stack([rec] * n)), dev(np.full(n, len(rec), np.int32))
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    table, counts, status = torch.zeros((n, cap, 9), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
    fit = dict(h=torch.zeros((n, 9), dtype=torch.float64, device="cuda"), err_sq=torch.zeros((n, cap), **f32),
               row_status=torch.zeros((n, cap), **i32), n_inliers=torch.zeros(n, **i32), rms=torch.zeros(n, **f32),
               pred=torch.zeros((n, nb, 9), **i32), n_pred=torch.zeros(n, **i32), status=torch.zeros(n, **i32))
    slots, kept, nkept, sst = torch.zeros((n, nb, 4), **i32), torch.zeros((n, nb, 4), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
    try:
        det.set_option("device_tail", 1)  # the table is final in stream order: no host step at all
        final = True
    except A.AgxError:
        final = False  # (this host's libm is not the kernel's: the host tail writes the table at the fetch)
    det.detect_batch_enqueue(frames, cap, out=(table, counts, status))
    if not final:
        det.detect_batch_fetch()
    det.board_fit_enqueue(table, counts, cols, rows, (w, h), predict_missing=True, max_drop=2, tag_status=status, **fit)
    det.snap_points_enqueue(saddles, fit["pred"], slots, kept, nkept, sst, 9.0, counts=scounts, row_counts=fit["n_pred"], reverse=True)
    with pytest.raises(A.AgxError) as e:  # the fit replaced the detect batch: nothing of any kind is fetchable
        det.detect_batch_fetch()
    assert e.value.status == _ffi.AGX_ERR_STATE
    det.sync()
    if final:
        det.set_option("device_tail", -1)
    got_counts = counts.cpu().numpy()
    assert (got_counts == len(tags)).all() and (status.cpu().numpy() == 0).all()
    for f in range(n):
        rows_f = table[f, :got_counts[f]].cpu().numpy().view(BC.TAG).reshape(-1)
        assert sorted(rows_f["id"].tolist()) == sorted(tags)
        want = Batch("chain", [rows_f], cols, rows, (w, h), max_drop=2, flags=MISSING, tpf=cap).host()
        assert want["status"][0] == OK and int(fit["status"][f]) == OK
        k = int(want["n_pred"][0])
        assert int(fit["n_pred"][f]) == k == nb - len(tags)
        assert fit["pred"][f, :k].cpu().numpy().tobytes() == want["pred"][0, :k].tobytes() and fit["h"][f].cpu().numpy().tobytes() == want["h"][0].tobytes()
        s_slots, _d, s_rows, _i, s_st = A.snap_points(lists, want["pred"][0, :k], 9.0, reverse=True)
        assert s_st == _ffi.AGX_SNAP_OK and int(sst[f]) == _ffi.AGX_SNAP_OK and int(nkept[f]) == len(s_rows)
        assert np.array_equal(slots[f, :k].cpu().numpy().view(np.uint32), s_slots)
        assert np.array_equal(kept[f, :len(s_rows)].cpu().numpy().view(np.uint32), s_rows)


def test_refused_arguments_leave_the_batch_in_flight(det):
    import torch
    t = cases()["frame0"].tables[0]
    b = Batch("args", [t], 7, 4, (800, 600))
    d = {k: dev(v.view(np.int32).reshape(v.shape[0], -1, 9) if k == "pred" else v) for k, v in b.empty_outputs().items()}
    table, counts = dev(b.table().view(np.int32).reshape(1, b.tpf, 9)), dev(np.array(b.counts, np.int32))
    det.saddles_batch_enqueue(torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda"))

    def call(n=1, tags=table.data_ptr(), tpf=b.tpf, counts=counts.data_ptr(), cols=7, rows=4, s=0.3, img_w=800, img_h=600, err=4.0, min_tags=1, flags=0,
             **ptr):
        p = {k: d[k].data_ptr() for k in KEYS}
        p.update(ptr)
        return det._lib.agx_board_fit_enqueue(det._h, n, tags, tpf, counts, None, cols, rows, 0, float(s), img_w, img_h, float(err), 0, min_tags, flags,
                                              *[p[k] for k in KEYS])

    E = _ffi.AGX_ERR_ARG
    for kw in ([dict(n=0), dict(tags=None), dict(counts=None), dict(tpf=0), dict(cols=0), dict(rows=0), dict(cols=64, rows=65), dict(s=np.nan),
                dict(s=np.inf), dict(s=-1.0), dict(img_w=0), dict(img_h=0), dict(err=-1.0), dict(err=np.nan), dict(min_tags=0), dict(flags=2),
                dict(h_=1), dict(n=1 << 14, tpf=1 << 13), dict(tags=table.data_ptr() + 2)] + [{k: None} for k in KEYS]):
        if "h_" in kw:
            kw = dict(h=d["h"].data_ptr() + 4)  # 4-byte aligned is not enough for doubles
        assert call(**kw) == E, kw
    res, _ = det.saddles_batch_fetch()  # still there
    assert len(res) == 1
    assert all(BC.untouched(d[k].cpu().numpy()) for k in KEYS)
    assert call() == _ffi.AGX_OK
    det.sync()
    with pytest.raises(A.AgxError) as e:
        det.saddles_batch_fetch()
    assert e.value.status == _ffi.AGX_ERR_STATE
    assert int(d["status"][0]) == OK and BC.untouched(d["status"][1:].cpu().numpy())


# ---- recovery on the device against its restatement over the host forms -------------------------------------------------------------
def same_tags(got, want, what):
    assert list(got) == list(want), "%s: ids %s, host %s" % (what, list(got), list(want))
    for t in want:
        assert np.array_equal(np.asarray(got[t], np.float32).view(np.uint32), want[t].view(np.uint32)), "%s: corners of tag %d" % (what, t)


@pytest.mark.parametrize("k", (0, 1))
def test_detect_recovered_equals_the_host_restatement(det, k):
    from oracle import oracle as O
    img, gt, tags, (w, h, rows, cols) = BC.frame(k)
    want, fit = BC.recovered_host(img, O.refined_saddle_points(img), tags, cols, rows)
    got, fits = det.detect_recovered(dev(np.stack([img, img])), cols, rows, return_fit=True)
    for f in range(2):
        same_tags(got[f], want, "frame %d.%d" % (k, f))
        assert fits[f]["status"] == fit["status"] == OK and fits[f]["recovered"] == len(want) - len(tags) and fits[f]["n_inliers"] == len(tags)
        # the table's rows are detect's in detect's order, so the fit's numbers are the host form's bytes
        assert fits[f]["H"].tobytes() == fit["H"].tobytes() and fits[f]["err_sq"].tobytes() == fit["err_sq"].tobytes()
        assert fits[f]["row_status"].tolist() == fit["row_status"].tolist() and np.float32(fits[f]["rms"]) == np.float32(fit["rms"])
    assert det.detect_recovered(dev(img[None]), cols, rows)[0].keys() == want.keys()


def test_a_refused_fit_keeps_detect_staged_result(det):
    img, gt, tags, (w, h, rows, cols) = BC.frame(1)
    got, fits = det.detect_recovered(dev(img[None]), cols, rows, min_tags=len(tags) + 1, return_fit=True)
    same_tags(got[0], tags, "min_tags above the count")
    assert fits[0]["status"] == FEW and fits[0]["H"] is None and fits[0]["recovered"] == 0


def test_tags_taken_out_of_the_table_are_recovered_on_the_device(det):
    """recover_tags_enqueue on caller-given tables: the gather, the decode, the acceptance by predicted id and the collect, with
    tags to bring back -- three frames in one batch: tags taken out, a row under a wrong id, nothing missing but 0 and 27."""
    import torch
    from oracle import oracle as O
    img, gt, tags, (w, h, rows, cols) = BC.frame(0)
    s = O.refined_saddle_points(img)
    ids = list(tags)
    tables = [{t: xy for t, xy in tags.items() if t not in (9, 17, 12)}, {(27 if t == ids[5] else t): xy for t, xy in tags.items()}, dict(tags)]
    n, tpf = len(tables), 40
    table = np.zeros((n, tpf), BC.TAG)
    for f, t in enumerate(tables):
        table[f, :len(t)] = BC.tag_rows(t)
    d_tags, d_n = dev(table.view(np.int32).reshape(n, tpf, 9)), dev(np.array([len(t) for t in tables], np.int32))
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    rec = np.ascontiguousarray(s).view(np.float32).reshape(-1, 5)
    fit = det.recover_tags_enqueue(dev(np.stack([img] * n)), dev(np.stack([rec] * n)), dev(np.full(n, len(rec), np.int32)), None, d_tags, d_n, d_st,
                                   cols, rows)
    det.sync()
    assert d_st.cpu().tolist() == [0] * n and fit["recovered"].cpu().tolist() == [3, 1, 0] and fit["status"].cpu().tolist() == [OK] * n
    out, counts = d_tags.cpu().numpy().view(BC.TAG).reshape(n, tpf), d_n.cpu().numpy()
    for f, t in enumerate(tables):
        want, _ = BC.recovered_host(img, s, t, cols, rows)
        got = {int(r["id"]): r["xy"].reshape(4, 2) for r in out[f, :counts[f]]}
        same_tags(got, want, "table %d" % f)
    assert fit["row_status"][1, :len(ids)].cpu().tolist() == [1 if r == 5 else 0 for r in range(len(ids))]
