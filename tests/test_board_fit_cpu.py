"""agx_board_fit_tail, the host form of the board fit (csrc/board_fit_math.h), without a device: the corner convention against
the renderer's ground truth, the fit against a numpy float64 lstsq restatement, the outlier rounds, every frame status, the
limits of the table and the layout, what a refused frame leaves untouched, and the recovery of missing tags restated over the
host forms.  tests/board_fit_cases.py holds the cases; the
GPU suite runs the same ones for byte parity."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi
from tests import board_fit_cases as BC
from tests.board_fit_cases import FEW, INLIER, INPUT, LOOSE, OFF_BOARD, OK, OUTLIER, SINGULAR, cases
from tests.util import ROOT

TOL = 1e-3  # px: the project's stated tolerance against the float64 yardstick


def run(name):
    b = cases()[name]
    return b, b.host()


def pred_corners(out, f=0):
    n = int(out["n_pred"][f])
    return out["pred"][f, :n]["id"], out["pred"][f, :n]["xy"].reshape(n, 4, 2).astype(np.float64)


@pytest.mark.parametrize("k", range(3))
def test_detects_corner_j_is_ground_truth_corner_3_2_1_0(k):
    """The correspondence pin: xy[j] of every tag the oracle detects is nearest to ground truth [3, 2, 1, 0][j]."""
    _, gt, tags, _ = BC.frame(k)
    assert len(tags) >= 26
    for t, xy in tags.items():
        d = np.hypot(xy[:, None, 0] - gt[t][None, :, 0], xy[:, None, 1] - gt[t][None, :, 1])
        assert d.argmin(axis=1).tolist() == BC.GT_ORDER, (t, d)


@pytest.mark.parametrize("k", range(3))
def test_the_fit_is_the_float64_lstsq_fit(k):
    b, out = run("frame%d" % k)
    assert out["status"][0] == OK and out["n_inliers"][0] == len(b.tables[0]) and out["n_pred"][0] == b.cols * b.rows
    H, want = BC.numpy_fit(b.tables[0], b.cols, b.rows, b.size)
    got = BC.project(out["h"][0], BC.board_points(b.cols, b.rows))
    worst = np.abs(got - want).max()
    print("frame %d: H-projected corners against lstsq: %.3e px" % (k, worst))
    assert worst <= TOL
    ids, pred = pred_corners(out)
    assert ids.tolist() == list(range(b.cols * b.rows))
    assert np.abs(pred - want).max() <= TOL
    # the rows' residuals and the rms are those of the yardstick's projection
    det = b.tables[0]["xy"].reshape(-1, 4, 2).astype(np.float64)
    e = ((det - want[b.tables[0]["id"]]) ** 2).sum(axis=2)
    assert np.allclose(out["err_sq"][0, :len(det)], e.max(axis=1), rtol=1e-3, atol=1e-6)
    assert np.isclose(out["rms"][0], np.sqrt(e.mean()), rtol=1e-3)
    assert abs(out["h"][0, 8] - 1.0) < 0.5 and np.isfinite(out["h"][0]).all()


@pytest.mark.parametrize("k", range(3))
def test_predicted_corners_are_nearer_to_ground_truth_than_detected_ones(k):
    _, gt, tags, _ = BC.frame(k)
    b, out = run("frame%d" % k)
    ids, pred = pred_corners(out)
    worst_pred = max(np.hypot(*(pred[i] - gt[int(t)][BC.GT_ORDER]).T).max() for i, t in enumerate(ids))
    worst_det = max(np.hypot(*(tags[t] - gt[t][BC.GT_ORDER]).T).max() for t in tags)
    print("frame %d: worst predicted corner %.4f px, worst detected corner %.4f px" % (k, worst_pred, worst_det))
    assert sorted(ids.tolist()) == sorted(gt) and worst_pred < worst_det


def test_predict_missing_holds_the_tags_that_are_not_inlier_rows():
    b, out = run("frame0_missing")
    full = run("frame0")[1]
    ids, _ = pred_corners(out)
    assert ids.tolist() == [0, 27] and out["status"][0] == OK
    assert out["pred"][0, :2].tobytes() == full["pred"][0, [0, 27]].tobytes()
    assert BC.untouched(out["pred"][0, 2:])
    for k in (1, 2):
        assert run("frame%d_missing" % k)[1]["n_pred"][0] == 0


def test_a_tag_under_a_wrong_id_is_dropped_in_one_round():
    b, out = run("wrong_id")
    n = len(b.tables[0])
    assert out["status"][0] == OK and out["n_inliers"][0] == n - 1
    want = np.full(n, INLIER)
    want[5] = OUTLIER
    assert out["row_status"][0, :n].tolist() == want.tolist()
    assert out["err_sq"][0, 5] > 100.0 ** 2 and out["err_sq"][0, :n][want == INLIER].max() < 0.2 ** 2
    ids, pred = pred_corners(out)
    lost = int(cases()["frame0"].tables[0]["id"][5])  # the tag whose corners went under id 27
    assert ids.tolist() == [0, lost, 27]  # the dropped row's id is predicted, not believed; so is the tag it really was
    clean = run("wrong_id_without")[1]
    assert clean["status"][0] == OK
    _, all_pred = pred_corners(clean)
    assert np.abs(pred - all_pred[[0, lost, 27]]).max() <= TOL
    assert out["h"][0].tobytes() == clean["h"][0].tobytes() or np.abs(out["h"][0] - clean["h"][0]).max() < 1e-6


def test_drop_limits_and_loose():
    b, out = run("two_wrong_drop1")
    n = len(b.tables[0])
    assert out["status"][0] == LOOSE and out["n_inliers"][0] == n - 1 and (out["row_status"][0, :n] == OUTLIER).sum() == 1
    assert out["n_pred"][0] == b.cols * b.rows and np.isfinite(out["h"][0]).all() and out["rms"][0] > 1.0
    b, out = run("two_wrong_drop2")
    assert out["status"][0] == OK and np.flatnonzero(out["row_status"][0, :n] == OUTLIER).tolist() == [5, 11] and out["rms"][0] < 0.1
    b, out = run("wrong_drop0")
    assert out["status"][0] == LOOSE and out["n_inliers"][0] == n and (out["row_status"][0, :n] == INLIER).all()


def test_of_two_rows_with_byte_equal_residuals_the_lower_goes_first():
    b, out = run("tie_drop1")
    n = len(b.tables[0])
    assert out["err_sq"][0, 5].tobytes() == out["err_sq"][0, 9].tobytes()
    assert out["status"][0] == LOOSE and np.flatnonzero(out["row_status"][0, :n] == OUTLIER).tolist() == [5]
    b, out = run("tie_drop2")
    assert out["status"][0] == OK and np.flatnonzero(out["row_status"][0, :n] == OUTLIER).tolist() == [5, 9]


REFUSED = [("count0", FEW), ("min_tags_missed", FEW), ("min_tags_missed_after_drop", FEW), ("on_board_nan", INPUT), ("on_board_inf", INPUT),
           ("on_board_minus_inf", INPUT), ("four_equal_corners", SINGULAR), ("four_equal_corners_centre", SINGULAR), ("tag_status", INPUT),
           ("count_above_rows", INPUT)]


@pytest.mark.parametrize("name,status", REFUSED)
def test_a_refused_frame_writes_its_status_and_two_zero_counts_only(name, status):
    b, out = run(name)
    assert out["status"][0] == status and out["n_inliers"][0] == 0 and out["n_pred"][0] == 0
    for k in ("h", "err_sq", "row_status", "rms", "pred"):
        assert BC.untouched(out[k]), k
    for k in ("status", "n_inliers", "n_pred"):
        assert BC.untouched(out[k][1:]), k


def test_min_tags_on_the_inlier_count_is_enough():
    b, out = run("min_tags_met")
    assert out["status"][0] == OK and out["n_inliers"][0] == b.min_tags


def test_a_single_tag_is_reproduced():
    b, out = run("single_tag")
    assert out["status"][0] == OK and out["n_inliers"][0] == 1
    ids, pred = pred_corners(out)
    t = int(b.tables[0]["id"][0])
    assert np.abs(pred[t] - b.tables[0]["xy"][0].reshape(4, 2)).max() <= TOL and out["err_sq"][0, 0] <= TOL ** 2


def test_off_board_rows_are_marked_and_never_fitted():
    b, out = run("off_board")
    ids = b.tables[0]["id"]
    on = (ids >= 107) & (ids < 107 + 14)
    assert on.sum() >= 10 and (~on).sum() >= 5 and ids.min() < 107 and ids.max() >= 121
    n = len(ids)
    assert out["status"][0] == OK and out["rms"][0] < 0.1  # (two rows of the printed board are a board)
    assert (out["row_status"][0, :n][~on] == OFF_BOARD).all() and (out["row_status"][0, :n][on] == INLIER).all()
    assert out["n_inliers"][0] == on.sum()
    assert BC.untouched(out["err_sq"][0, :n][~on]) and not BC.untouched(out["err_sq"][0, :n][on])
    pid, _ = pred_corners(out)
    assert pid.tolist() == list(range(107, 121))
    for name in ("nan", "inf", "minus_inf"):  # a corner that is not finite in an off-board row is never read
        bad = run("off_board_" + name)[1]
        for k in out:
            assert bad[k].tobytes() == out[k].tobytes(), (name, k)


def wrap_fit(name, s):
    """A case on the wrapping 7 x 4 layout -> (batch, outputs, the lstsq yardstick's corners, the exact homography's corners);
    the yardstick does its own modular id subtraction, and H is held to it."""
    b, out = run(name)
    assert (b.cols, b.rows, b.first_id, b.s) == (7, 4, 0xFFFFFFF0, s) and out["status"][0] == OK
    _, want = BC.numpy_fit(b.tables[0], 7, 4, b.size, first_id=b.first_id, s=s)
    P = BC.board_points(7, 4, s)
    worst = np.abs(BC.project(out["h"][0], P) - want).max()
    exact = BC.project(BC.pose(7, 4, b.size, s=s, tilt=BC.WRAP_TILT), P)
    print("%s: H-projected corners against lstsq %.3e px, lstsq against the exact homography %.3e px" % (name, worst, np.abs(want - exact).max()))
    assert worst <= TOL
    return b, out, want, exact


@pytest.mark.parametrize("s", BC.WRAP_RATIOS)
def test_spacing_ratios_with_an_id_window_that_passes_2_to_the_32(s):
    """first_id = 0xFFFFFFF0: the layout's 28 ids run through 0xFFFFFFFF, wrap to 0 and end at 11 (fit_on_board's wrapping
    subtraction, the prediction's first_id + t), at spacing ratios the other cases never take: 0, -0.5 and 1."""
    b, out, want, exact = wrap_fit("wrap_s%g" % s, s)
    layout = [(0xFFFFFFF0 + t) % (1 << 32) for t in range(28)]
    assert b.tables[0]["id"].tolist() == layout and layout[15:17] == [0xFFFFFFFF, 0] and layout[-1] == 11
    assert out["n_inliers"][0] == 28 and (out["row_status"][0, :28] == INLIER).all()
    ids, pred = pred_corners(out)
    assert ids.dtype == np.uint32 and ids.tolist() == layout
    assert np.abs(pred - want).max() <= TOL and np.abs(pred - exact).max() <= TOL
    assert out["err_sq"][0, :28].max() <= TOL ** 2 and out["rms"][0] <= TOL


def test_missing_tags_on_either_side_of_the_wrap_are_predicted():
    b, out, want, exact = wrap_fit("wrap_s1_missing", 1.0)
    gone = list(BC.WRAP_GONE)
    ids, pred = pred_corners(out)
    assert out["n_inliers"][0] == 24 and ids.tolist() == [(0xFFFFFFF0 + t) % (1 << 32) for t in gone] == [0xFFFFFFF3, 0xFFFFFFFF, 0, 6]
    d = np.abs(pred - exact[gone]).max()
    print("wrap_s1_missing: predicted corners of the missing tags against the exact homography %.3e px" % d)
    assert d <= TOL and np.abs(pred - want[gone]).max() <= TOL
    assert BC.untouched(out["pred"][0, 4:])


def test_ids_next_to_a_wrapped_window_are_off_the_board():
    b, out, want, exact = wrap_fit("wrap_off_board", 1.0)
    ids = b.tables[0]["id"].tolist()
    assert (ids[0], ids[-1]) == (0xFFFFFFEF, 12) == BC.WRAP_OFF_IDS and len(ids) == 30
    assert out["row_status"][0, :30].tolist() == [OFF_BOARD] + [INLIER] * 28 + [OFF_BOARD] and out["n_inliers"][0] == 28
    assert BC.untouched(out["err_sq"][0, [0, 29]]) and out["err_sq"][0, 1:29].max() <= TOL ** 2
    assert np.abs(pred_corners(out)[1] - exact).max() <= TOL


def test_a_steep_pose_predicts_nan_where_w_is_not_positive():
    b, out = run("steep")
    assert out["status"][0] == OK and out["rms"][0] < 1e-3
    ids, pred = pred_corners(out)
    P = BC.board_points(8, 8)
    w = 1.0 - BC.STEEP_TILT * P[..., 1]
    nan = np.isnan(pred).all(axis=2)
    assert (np.isnan(pred).any(axis=2) == nan).all()
    assert np.abs(w).min() > 0.05  # (no corner of the layout lies near the horizon: the nearest rows have w = 0.064 and -0.056)
    assert (nan == (w <= 0)).all() and nan.any() and not nan.all()
    want = BC.project(BC.pose(8, 8, (800, 600), tilt=BC.STEEP_TILT), P)
    near = w > 0.5
    assert np.abs(pred[near] - want[near]).max() < 0.01


def test_layouts_of_one_tag_and_of_4096():
    b, out = run("layout_1x1")
    assert out["status"][0] == OK and out["n_pred"][0] == 1 and out["pred"][0, 0]["id"] == 7
    assert np.abs(out["pred"][0, 0]["xy"] - b.tables[0]["xy"][0]).max() <= TOL
    b, out = run("layout_64x64")
    assert out["status"][0] == OK and out["n_pred"][0] == 4096 - 7
    ids, pred = pred_corners(out)
    assert sorted(set(range(4096)) - set(ids.tolist())) == sorted(b.tables[0]["id"].tolist())
    _, want = BC.numpy_fit(b.tables[0], 64, 64, b.size)
    assert np.abs(pred - want[ids]).max() <= TOL


@pytest.mark.parametrize("n", (63, 64, 65))
def test_counts_where_the_lane_stride_wraps(n):
    b, out = run("count%d" % n)
    assert out["status"][0] == OK and out["n_inliers"][0] == n
    _, want = BC.numpy_fit(b.tables[0], b.cols, b.rows, b.size)
    assert np.abs(pred_corners(out)[1] - want).max() <= TOL


def test_argument_rules():
    t = BC.tag_rows(BC.frame(0)[2])
    good = dict(tags=t.ctypes.data, tpf=len(t), n=len(t), st=0, cols=7, rows=4, first=0, s=0.3, w=800, h=600, err=4.0, drop=0, min=1, flags=0)
    order = list(good)
    b = BC.Batch("args", [t], 7, 4, (800, 600))
    u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def call(null=(), offset=None, **kw):
        out = b.empty_outputs()
        a = dict(good, **kw)
        ptr = {k: out[k].ctypes.data for k in out}
        if offset:
            ptr[offset[0]] += offset[1]
        for k in null:
            ptr[k] = None
        rc = _ffi.lib().agx_board_fit_tail(*[a[k] for k in order], ptr["h"], ptr["err_sq"], ptr["row_status"], C.cast(ptr["n_inliers"], u32),
                                           C.cast(ptr["rms"], f32), ptr["pred"], C.cast(ptr["n_pred"], u32), C.cast(ptr["status"], u32))
        if rc != _ffi.AGX_OK:
            assert all(BC.untouched(v) for v in out.values())
        return rc

    assert call() == _ffi.AGX_OK
    for kw in (dict(cols=0), dict(rows=0), dict(cols=65, rows=64), dict(cols=4097, rows=1), dict(s=float("nan")), dict(s=float("inf")), dict(s=-1.0),
               dict(s=-2.0), dict(w=0), dict(h=-1), dict(err=-1.0), dict(err=float("nan")), dict(min=0), dict(flags=2), dict(flags=-1),
               dict(tags=None)):
        assert call(**kw) == _ffi.AGX_ERR_ARG, kw
    for k in ("h", "err_sq", "row_status", "n_inliers", "rms", "pred", "n_pred", "status"):
        assert call(null=(k,)) == _ffi.AGX_ERR_ARG, k
    assert call(offset=("h", 4)) == _ffi.AGX_ERR_ARG and call(offset=("pred", 2)) == _ffi.AGX_ERR_ARG and call(offset=("err_sq", 1)) == _ffi.AGX_ERR_ARG
    assert call(s=-0.5) == _ffi.AGX_OK and call(err=float("inf")) == _ffi.AGX_OK  # (rows * cols = 4096: the case layout_64x64)
    assert call(tpf=1 << 27) == _ffi.AGX_ERR_ARG


def test_the_python_host_form_returns_the_same_numbers():
    b, out = run("wrong_id")
    fit = A.TagDetector.board_fit(b.tables[0], b.cols, b.rows, b.size, max_drop=1, predict_missing=True)
    n = len(b.tables[0])
    assert fit["status"] == OK and fit["n_inliers"] == n - 1 and fit["H"].tobytes() == out["h"][0].tobytes()
    assert fit["err_sq"].tobytes() == out["err_sq"][0, :n].tobytes() and fit["row_status"].tolist() == out["row_status"][0, :n].tolist()
    assert len(fit["pred"]) == 3 and fit["pred"].tobytes() == out["pred"][0, :3].tobytes() and np.float32(fit["rms"]).tobytes() == out["rms"][0].tobytes()
    tags = {int(r["id"]): r["xy"].reshape(4, 2) for r in b.tables[0]}
    assert A.board_fit(tags, b.cols, b.rows, b.size, max_drop=1, predict_missing=True)["H"].tobytes() == fit["H"].tobytes()
    assert A.board_fit({}, 7, 4, (800, 600)) == {"status": FEW, "n_inliers": 0, "n_pred": 0}
    with pytest.raises(A.AgxError):
        A.board_fit(tags, 0, 4, (800, 600))


def test_constants_and_declarations_agree_in_header_python_and_rust():
    hdr = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    names = ("AGX_FIT_PREDICT_MISSING", "AGX_FIT_OK", "AGX_FIT_LOOSE", "AGX_FIT_FEW", "AGX_FIT_SINGULAR", "AGX_FIT_INPUT", "AGX_FIT_ROW_INLIER",
             "AGX_FIT_ROW_OUTLIER", "AGX_FIT_ROW_OFF_BOARD")
    for n in names:
        v = int(re.search(r"\b%s\s*=\s*(\d+)" % n, hdr).group(1))
        assert getattr(_ffi, n) == v and re.search(r"pub const %s: c_int = %d;" % (n, v), ffi), n
    for f in ("agx_board_fit_enqueue", "agx_board_fit_tail"):
        assert f in _ffi.SYMBOLS and ("pub fn %s(" % f) in ffi
        assert len(_ffi.SYMBOLS[f][1]) == len(re.search(r"int %s\((.*?)\);" % f, hdr, flags=re.S).group(1).split(","))
    assert "pub fn board_fit_tail" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


# ---- recovery: detect_recovered restated over the host forms (tests/board_fit_cases.py: recovered_host) -----------------------------
def frame_saddles(k):
    from oracle import oracle as O
    return O.refined_saddle_points(BC.frame(k)[0])


def test_recovery_on_the_4x7_frame_keeps_detects_tags_and_reaches_26_of_28():
    """Pinned: 26.  Tags 0 and 27 stay missing because each of them reaches beyond the 800 x 600 frame -- two of their predicted
    corners lie outside the image or have no saddle within tens of pixels -- and a corner without a saddle cannot snap."""
    img, gt, tags, (w, h, rows, cols) = BC.frame(0)
    s = frame_saddles(0)
    got, fit = BC.recovered_host(img, s, tags, cols, rows)
    assert fit["status"] == OK and fit["pred"]["id"].tolist() == [0, 27]
    assert list(got)[:len(tags)] == list(tags) and all(np.array_equal(got[t].view(np.uint32), tags[t].view(np.uint32)) for t in tags)
    assert len(got) == 26
    sx = np.stack([s["x"], s["y"]], axis=1).astype(np.float64)
    for p in fit["pred"]:
        d = [np.hypot(*(sx - c).T).min() for c in p["xy"].reshape(4, 2).astype(np.float64)]
        assert sum(x > 20.0 for x in d) == 2 and sum(x < 0.1 for x in d) == 2, (int(p["id"]), d)


@pytest.mark.parametrize("k,gone", [(0, (9, 17, 12)), (1, (0, 35, 14, 15)), (2, (55,))])
def test_tags_taken_out_of_detects_table_come_back_bit_for_bit(k, gone):
    img, gt, tags, (w, h, rows, cols) = BC.frame(k)
    assert all(t in tags for t in gone)
    less = {t: xy for t, xy in tags.items() if t not in gone}
    got, fit = BC.recovered_host(img, frame_saddles(k), less, cols, rows)
    assert fit["status"] == OK and sorted(got) == sorted(tags) and list(got)[:len(less)] == list(less)
    for t in tags:  # the same saddles through the same decode: detect's corners
        assert np.array_equal(got[t].view(np.uint32), tags[t].view(np.uint32)), t
    for t in gone:
        assert t in gt and np.hypot(*(got[t] - gt[t][BC.GT_ORDER]).T).max() <= 0.5


def test_a_row_under_a_wrong_id_stays_and_the_tag_it_hid_is_recovered():
    img, gt, tags, (w, h, rows, cols) = BC.frame(0)
    ids = list(tags)
    hidden = ids[5]
    wrong = {(27 if t == hidden else t): xy for t, xy in tags.items()}  # row 5 under id 27, which detect misses
    got, fit = BC.recovered_host(img, frame_saddles(0), wrong, cols, rows)
    assert fit["status"] == OK and fit["row_status"].tolist() == [OUTLIER if r == 5 else INLIER for r in range(len(ids))]
    assert list(got)[:len(ids)] == list(wrong) and np.array_equal(got[27], tags[hidden])  # reported, not removed
    assert len(got) == len(ids) + 1 and np.array_equal(got[hidden].view(np.uint32), tags[hidden].view(np.uint32))


def test_recovery_changes_nothing_where_detect_has_every_tag():
    from tests.test_find_boards_cpu import golden_list
    from tests.util import ALL_IMAGES, load_image
    from oracle import oracle as O
    for name in ALL_IMAGES:
        if name == "two_boards.png":
            continue
        s, luma = golden_list(name), A.TagDetector.luma8(load_image(name))
        tags = A.TagDetector.detect_tail("t36h11", s, luma)
        cols = 11 if name == "iphone.png" else 6
        got, fit = BC.recovered_host(luma, s, tags, cols, 6)
        assert fit["status"] in (OK, LOOSE) and len(tags) == cols * 6, name  # (real lenses: the residuals are pixels, not hundredths)
        assert list(got) == list(tags) and all(np.array_equal(got[t], tags[t]) for t in tags), name
    for seed, n in ((7, 5), (12, 6)):
        img, gt = BC.synth.render_frame(seed, 800, 600, spec=BC.synth.BoardSpec(rows=n, cols=n))
        img = np.ascontiguousarray(img.numpy())
        tags = O.detect(img)
        got, fit = BC.recovered_host(img, O.refined_saddle_points(img), tags, n, n)
        assert fit["status"] == OK and len(tags) == n * n
        assert list(got) == list(tags) and all(np.array_equal(got[t], tags[t]) for t in tags)


def test_one_small_far_tag_is_weak_but_not_singular():
    b, out = run("far_tag_64x64")
    assert out["status"][0] == OK and out["n_inliers"][0] == 1 and out["err_sq"][0, 0] <= TOL ** 2
    assert np.abs(out["pred"][0, 4095]["xy"] - b.tables[0]["xy"][0]).max() <= TOL


def test_more_rows_than_the_kernel_stages_is_input_whatever_the_table_holds():
    b, out = run("count_641")
    assert b.tpf == 700 and out["status"][0] == INPUT and out["n_inliers"][0] == 0 and out["n_pred"][0] == 0
    assert all(BC.untouched(out[k]) for k in ("h", "err_sq", "row_status", "rms", "pred"))
    b, out = run("count_640")
    assert out["status"][0] == OK and out["n_inliers"][0] == 640
