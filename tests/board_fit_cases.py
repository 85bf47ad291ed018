"""What tests/test_board_fit_cpu.py and tests/test_gpu_board_fit.py share: the three rendered frames of the issue with the oracle's
tags and the ground truth, the numpy float64 yardstick of the fit (the same normalised system, solved with lstsq), tables made
from an exact homography, a batch of frames answered by agx_board_fit_tail into sentinel-filled arrays, and the list of cases
both suites run."""
import ctypes as C
import functools

import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi, synth

TAG = A.TagDetector.TAG_DTYPE
OX, OY = (0.0, 1.0, 1.0, 0.0), (0.0, 0.0, 1.0, 1.0)
GT_ORDER = [3, 2, 1, 0]  # detect's xy[j] is synth's ground-truth corner GT_ORDER[j]: BL, BR, TR, TL of the upright tag
FRAMES = ((3, 800, 600, 4, 7), (12, 800, 600, 6, 6), (5, 1280, 800, 10, 10))  # seed, width, height, rows, cols
FILL = 0xA5
STEEP_TILT = 0.12
OK, LOOSE, FEW, SINGULAR, INPUT = _ffi.AGX_FIT_OK, _ffi.AGX_FIT_LOOSE, _ffi.AGX_FIT_FEW, _ffi.AGX_FIT_SINGULAR, _ffi.AGX_FIT_INPUT
INLIER, OUTLIER, OFF_BOARD = _ffi.AGX_FIT_ROW_INLIER, _ffi.AGX_FIT_ROW_OUTLIER, _ffi.AGX_FIT_ROW_OFF_BOARD


@functools.lru_cache(maxsize=None)
def frame(k):
    """Frame k of FRAMES -> (luma uint8 [h, w], ground truth {id: 4x2}, the oracle's detect {id: 4x2 float32}, (w, h, rows, cols))."""
    from oracle import oracle as O
    seed, w, h, rows, cols = FRAMES[k]
    img, gt = synth.render_frame(seed, w, h, spec=synth.BoardSpec(rows=rows, cols=cols))
    img = np.ascontiguousarray(img.numpy())
    return img, gt, O.detect(img), (w, h, rows, cols)


def tag_rows(tags):
    """{id: 4x2 corners} -> TAG rows in dict order."""
    out = np.zeros(len(tags), TAG)
    for i, (t, xy) in enumerate(tags.items()):
        out["id"][i] = t
        out["xy"][i] = np.asarray(xy, np.float32).reshape(8)
    return out


def board_points(cols, rows, s=0.3):
    """[rows*cols, 4, 2] float64: Kalibr's board point of corner j of the layout's tag t, in tag sides."""
    t = np.arange(rows * cols)
    r, c = t // cols, t % cols
    return np.stack([c[:, None] * (1.0 + s) + np.array(OX), r[:, None] * (1.0 + s) + np.array(OY)], axis=-1)


def project(H, pts):
    p = np.concatenate([pts, np.ones(pts.shape[:-1] + (1,))], axis=-1) @ np.asarray(H, np.float64).reshape(3, 3).T
    return p[..., :2] / p[..., 2:]


def numpy_fit(table, cols, rows, size, first_id=0, s=0.3, keep=None):
    """The yardstick: the same normalised system over the on-board rows of `table` (keep: a bool per row), float64, solved with
    numpy.linalg.lstsq -> (H [3, 3] board units -> pixels, predicted corners [rows*cols, 4, 2] float64)."""
    w, h = size
    bw, bh = cols * (1.0 + s) - s, rows * (1.0 + s) - s
    sb, si = 2.0 / max(bw, bh), 2.0 / max(w, h)
    P = board_points(cols, rows, s)
    a, b = [], []
    for i, row in enumerate(table):
        t = (int(row["id"]) - int(first_id)) % (1 << 32)  # the window may pass 2^32: id 3 is tag 19 of a layout from 0xFFFFFFF0
        if not 0 <= t < rows * cols or (keep is not None and not keep[i]):
            continue
        for j in range(4):
            x, y = (P[t, j, 0] - bw / 2) * sb, (P[t, j, 1] - bh / 2) * sb
            u, v = (float(row["xy"][2 * j]) - w / 2) * si, (float(row["xy"][2 * j + 1]) - h / 2) * si
            a += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
            b += [u, v]
    sol = np.linalg.lstsq(np.array(a, np.float64), np.array(b, np.float64), rcond=None)[0]
    Hn = np.append(sol, 1.0).reshape(3, 3)
    Tb = np.array([[sb, 0, -sb * bw / 2], [0, sb, -sb * bh / 2], [0, 0, 1]])
    Ti = np.array([[1 / si, 0, w / 2], [0, 1 / si, h / 2], [0, 0, 1]])
    H = Ti @ Hn @ Tb
    return H, project(H, P)


def exact_table(cols, rows, ids, H, first_id=0, s=0.3, noise=0.0, seed=1):
    """TAG rows of the layout's tags `ids` (offsets from first_id) under the homography H, rounded to float32, each coordinate
    moved by up to `noise` px (a fixed pseudo-random sequence)."""
    P = project(H, board_points(cols, rows, s)[np.asarray(ids, np.int64)])
    rng = np.random.RandomState(seed)
    P = P + noise * (2.0 * rng.rand(*P.shape) - 1.0)
    out = np.zeros(len(ids), TAG)
    out["id"] = wrapped_ids(first_id, ids)
    out["xy"] = P.reshape(len(ids), 8).astype(np.float32)
    return out


def wrapped_ids(first_id, t):
    """The ids of the layout's tags t: (first_id + t) mod 2^32 as uint32, computed in int64."""
    return ((np.asarray(t, np.int64) + int(first_id)) & 0xFFFFFFFF).astype(np.uint32)


def pose(cols, rows, size, s=0.3, tilt=0.0):
    """A homography that puts the layout into the middle of the image, w = 1 - tilt * Y (Y in tag sides)."""
    w, h = size
    bw, bh = cols * (1.0 + s) - s, rows * (1.0 + s) - s
    k = 0.7 * min(w / bw, h / bh)
    return np.array([[k, 0.1 * k, 0.5 * w - 0.55 * k * bw], [-0.1 * k, k, 0.5 * h - 0.45 * k * bh], [0.0, -tilt, 1.0]])


class Batch:
    """Frames that share one call's scalars.  tables: one TAG array per frame (its rows; the count is their number unless
    counts says otherwise); tpf: rows per frame of the device table."""

    def __init__(self, name, tables, cols, rows, size, first_id=0, s=0.3, max_err_sq=4.0, max_drop=0, min_tags=1, flags=0, counts=None,
                 tag_status=None, tpf=None):
        self.name, self.tables, self.cols, self.rows, self.size = name, [np.ascontiguousarray(t, TAG) for t in tables], cols, rows, size
        self.first_id, self.s, self.max_err_sq, self.max_drop, self.min_tags, self.flags = first_id, s, max_err_sq, max_drop, min_tags, flags
        self.counts = [len(t) for t in self.tables] if counts is None else list(counts)
        self.tag_status = tag_status
        self.tpf = max([len(t) for t in self.tables] + [1]) if tpf is None else tpf
        self.n = len(self.tables)

    def table(self):
        """[n, tpf] TAG: the device table, rows beyond a frame's own filled with FILL bytes."""
        t = np.full((self.n, self.tpf), 0, TAG)
        t.view(np.uint8)[...] = FILL
        for f, rows in enumerate(self.tables):
            t[f, :len(rows)] = rows
        return t

    def scalars(self):
        return (self.cols, self.rows, self.first_id, float(self.s), int(self.size[0]), int(self.size[1]), float(self.max_err_sq), self.max_drop,
                self.min_tags, self.flags)

    def empty_outputs(self):
        """Every output array, one frame of room more than the call is told about, every byte FILL."""
        n, nb = self.n + 1, self.cols * self.rows
        shapes = dict(h=((n, 9), np.float64), err_sq=((n, self.tpf), np.float32), row_status=((n, self.tpf), np.uint32),
                      n_inliers=((n,), np.uint32), rms=((n,), np.float32), pred=((n, nb), TAG), n_pred=((n,), np.uint32),
                      status=((n,), np.uint32))
        out = {}
        for k, (shape, dt) in shapes.items():
            a = np.zeros(shape, dt)
            a.view(np.uint8)[...] = FILL
            out[k] = a
        return out

    def host(self):
        """agx_board_fit_tail frame by frame into empty_outputs()."""
        out, table = self.empty_outputs(), self.table()
        u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        for f in range(self.n):
            st = _ffi.AGX_TAGS_OK if self.tag_status is None else self.tag_status[f]
            rc = _ffi.lib().agx_board_fit_tail(
                table[f].ctypes.data, self.tpf, self.counts[f], st, *self.scalars(), out["h"][f].ctypes.data, out["err_sq"][f].ctypes.data,
                out["row_status"][f].ctypes.data, C.cast(out["n_inliers"][f:].ctypes.data, u32), C.cast(out["rms"][f:].ctypes.data, f32),
                out["pred"][f].ctypes.data, C.cast(out["n_pred"][f:].ctypes.data, u32), C.cast(out["status"][f:].ctypes.data, u32))
            assert rc == _ffi.AGX_OK, (self.name, f, rc)
        return out


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def swap_id(table, row, new_id):
    t = table.copy()
    t["id"][row] = new_id
    return t


WRAP_FIRST_ID = 0xFFFFFFF0
WRAP_RATIOS = (0.0, -0.5, 1.0)
WRAP_GONE = (3, 15, 16, 22)  # tags of the 7 x 4 layout taken out on either side of the wrap: ids 0xFFFFFFF3, 0xFFFFFFFF, 0, 6
WRAP_OFF_IDS = (0xFFFFFFEF, 12)
WRAP_TILT = 0.02


def wrap_table(s):
    """Every tag of the 7 x 4 layout from WRAP_FIRST_ID at spacing ratio s under pose(7, 4, (800, 600), s, WRAP_TILT), exact."""
    return exact_table(7, 4, range(28), pose(7, 4, (800, 600), s=s, tilt=WRAP_TILT), first_id=WRAP_FIRST_ID, s=s)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the CPU suite, which the GPU suite runs again for byte parity: name -> Batch."""
    out = []
    for k in range(3):
        _, _, tags, (w, h, rows, cols) = frame(k)
        t = tag_rows(tags)
        out.append(Batch("frame%d" % k, [t], cols, rows, (w, h)))
        out.append(Batch("frame%d_missing" % k, [t], cols, rows, (w, h), flags=_ffi.AGX_FIT_PREDICT_MISSING))
    _, _, tags, (w, h, rows, cols) = frame(0)  # 4 x 7: ids 0 and 27 are not detected
    t = tag_rows(tags)
    one, two = swap_id(t, 5, 27), swap_id(swap_id(t, 5, 27), 11, 0)
    out.append(Batch("wrong_id", [one], cols, rows, (w, h), max_drop=1, flags=_ffi.AGX_FIT_PREDICT_MISSING))
    out.append(Batch("wrong_id_without", [np.delete(t, 5)], cols, rows, (w, h), max_drop=1))
    out.append(Batch("two_wrong_drop1", [two], cols, rows, (w, h), max_drop=1))
    out.append(Batch("two_wrong_drop2", [two], cols, rows, (w, h), max_drop=2))
    out.append(Batch("wrong_drop0", [one], cols, rows, (w, h), max_drop=0))
    tie = np.concatenate([one[:9], one[5:6], one[9:]])  # the wrong row twice: rows 5 and 9, byte-equal residuals in every round
    out.append(Batch("tie_drop1", [tie], cols, rows, (w, h), max_drop=1))
    out.append(Batch("tie_drop2", [tie], cols, rows, (w, h), max_drop=2))
    out.append(Batch("count0", [t[:0]], cols, rows, (w, h)))
    out.append(Batch("min_tags_met", [t], cols, rows, (w, h), min_tags=len(t)))
    out.append(Batch("min_tags_missed", [t], cols, rows, (w, h), min_tags=len(t) + 1))
    out.append(Batch("min_tags_missed_after_drop", [one], cols, rows, (w, h), max_drop=1, min_tags=len(t)))
    out.append(Batch("single_tag", [t[3:4]], cols, rows, (w, h)))
    off = t.copy()
    off["id"] += 100  # the layout's two middle rows as a board of their own, first_id 107: ids 101 .. 106 lie below it, 121 .. 126 above
    out.append(Batch("off_board", [off], cols, 2, (w, h), first_id=107))
    for name, value in (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf)):
        bad = t.copy()
        bad["xy"][7, 5] = value
        out.append(Batch("on_board_" + name, [bad], cols, rows, (w, h)))
        bad = off.copy()
        bad["xy"][int(np.argmin(off["id"])), 2] = value  # id 101, below first_id
        out.append(Batch("off_board_" + name, [bad], cols, 2, (w, h), first_id=107))
    flat = t[3:4].copy()
    flat["xy"][0] = np.tile(np.float32([100.0, 50.0]), 4)
    out.append(Batch("four_equal_corners", [flat], cols, rows, (w, h)))
    flat = flat.copy()
    flat["xy"][0] = np.tile(np.float32([400.0, 300.0]), 4)  # the image's centre: exact zeros
    out.append(Batch("four_equal_corners_centre", [flat], cols, rows, (w, h)))
    out.append(Batch("tag_status", [t], cols, rows, (w, h), tag_status=[_ffi.AGX_TAGS_CAPACITY]))
    out.append(Batch("count_above_rows", [t], cols, rows, (w, h), counts=[len(t) + 1]))
    # a steep pose: w = 1 - 0.12 Y reaches 0 at Y = 8.33 of the 8 x 8 layout's 10.1 tag sides (the centre, where the fit's scale is
    # fixed, stays in front of the horizon); the table holds the three near rows
    steep = pose(8, 8, (800, 600), tilt=STEEP_TILT)
    out.append(Batch("steep", [exact_table(8, 8, range(24), steep)], 8, 8, (800, 600)))
    out.append(Batch("layout_1x1", [exact_table(1, 1, [0], pose(1, 1, (640, 480), tilt=0.05), first_id=7)], 1, 1, (640, 480), first_id=7))
    ids = [0, 63, 2000, 4032, 4095, 1234, 77]
    out.append(Batch("layout_64x64", [exact_table(64, 64, ids, pose(64, 64, (1280, 800), tilt=0.002), noise=0.05)], 64, 64, (1280, 800),
                     flags=_ffi.AGX_FIT_PREDICT_MISSING))
    # one small tag in the far corner of the 64 x 64 layout: weak (its board points span 1/83 of the normalised range) but valid --
    # the relative pivot threshold of AGX_FIT_SINGULAR must not take it for four coincident corners
    out.append(Batch("far_tag_64x64", [exact_table(64, 64, [4095], pose(64, 64, (1280, 800), tilt=0.002))], 64, 64, (1280, 800)))
    # more rows than the kernel stages (640), within the table's rows per frame: AGX_FIT_INPUT
    many = exact_table(64, 64, range(650), pose(64, 64, (1280, 800)))
    out.append(Batch("count_641", [many[:641]], 64, 64, (1280, 800), tpf=700))
    out.append(Batch("count_640", [many[:640]], 64, 64, (1280, 800), tpf=700))
    # the id window past 2^32, at the spacing ratios 0 (tags edge to edge), -0.5 (overlapping) and 1: the 7 x 4 layout from
    # 0xFFFFFFF0, whose 28 ids run through 0xFFFFFFFF, wrap to 0 and end at 11
    for s in WRAP_RATIOS:
        out.append(Batch("wrap_s%g" % s, [wrap_table(s)], 7, 4, (800, 600), first_id=WRAP_FIRST_ID, s=s))
    keep = [t for t in range(28) if t not in WRAP_GONE]
    out.append(Batch("wrap_s1_missing", [wrap_table(1.0)[keep]], 7, 4, (800, 600), first_id=WRAP_FIRST_ID, s=1.0, flags=_ffi.AGX_FIT_PREDICT_MISSING))
    off = wrap_table(1.0)[[5, 20]]
    off["id"] = WRAP_OFF_IDS  # the ids next to the window on either side: first_id - 1 and first_id + 28 mod 2^32
    off["xy"][0, 1] = np.nan  # never read
    out.append(Batch("wrap_off_board", [np.concatenate([off[:1], wrap_table(1.0), off[1:]])], 7, 4, (800, 600), first_id=WRAP_FIRST_ID, s=1.0))
    _, _, tags, (w, h, rows, cols) = frame(2)  # 100 tags: the lane stride wraps at 64
    t = tag_rows(tags)
    for n in (63, 64, 65):
        out.append(Batch("count%d" % n, [t[:n]], cols, rows, (w, h)))
    return {b.name: b for b in out}


def recovered_host(luma, saddles, tags, cols, rows, first_id=0, s=0.3, max_dist=3.0, max_err=2.0, max_drop=4, min_tags=2, family="t36h11"):
    """TagDetector.detect_recovered restated over the host forms for one frame: tags ({id: 4x2}, detect's result on these saddles) ->
    board_fit with the missing tags predicted -> snap_points of the predicted rows, back to front, onto the listed saddles ->
    decode_quads_tail of the snapped quads -> only a quad that decoded to the id predicted for it counts -> collect_tags into the
    frame's table.  -> ({id: 4x2 corners} in row order, the fit (board_fit's dict))."""
    saddles = np.ascontiguousarray(saddles, A.SADDLE_DTYPE)
    h, w = luma.shape
    table = tag_rows(tags)
    fit = A.board_fit(table, cols, rows, (w, h), first_id=first_id, spacing_ratio=s, max_err_sq=max_err * max_err, max_drop=max_drop,
                      min_tags=min_tags, predict_missing=True)
    if fit["status"] not in (OK, LOOSE) or not len(fit["pred"]) or not len(saddles):
        return dict(tags), fit
    _slots, _dist, quads, index, sst = A.snap_points(saddles, fit["pred"], max_dist * max_dist, reverse=True)
    if sst != _ffi.AGX_SNAP_OK or not len(quads):
        return dict(tags), fit
    pts = np.stack([saddles["x"][quads], saddles["y"][quads]], axis=-1)
    qtags, qstatus = A.decode_quads_tail(family, luma, pts)
    want = fit["pred"]["id"][index]
    qstatus = np.where((qstatus == _ffi.AGX_QUAD_DECODED) & (qtags["id"] == want), qstatus, _ffi.AGX_QUAD_NO_MATCH).astype(np.uint32)
    cap = 587
    room = np.zeros(cap, TAG)
    room[:len(table)] = table
    out, n, status, _ = A.collect_tags(family, quads, _ffi.AGX_BOARD_FOUND, qtags, qstatus, len(saddles), None, room, len(table), _ffi.AGX_TAGS_OK, cap)
    assert status == _ffi.AGX_TAGS_OK
    return {int(t["id"]): np.array(t["xy"], np.float32).reshape(4, 2) for t in out[:n]}, fit
