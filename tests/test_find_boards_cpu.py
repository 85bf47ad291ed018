"""agx_find_board_tail -- the host form of try_find_best_board (reference src/detector.rs:588-639) for caller-given saddle
lists -- against the oracle's orc_try_find_best_board on the golden lists, detect rebuilt by hand from it and
agx_decode_quads_tail against agx_detect_tail, and the argument / status rules.  No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.util import ALL_IMAGES, GOLDEN, ROOT, bits_equal, load_image

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi


# what tests/test_gpu_find_boards.py runs on: synth.render_batch(GPU_FIRST, GPU_FRAMES, *GPU_SIZE), the 6 x 6 board
GPU_SIZE = (640, 400)
GPU_FRAMES = 8
GPU_FIRST = 0


def golden_list(name):
    """The committed saddle list of a fixture image as a SADDLE_DTYPE array."""
    with open(os.path.join(GOLDEN, "saddles_%s.json" % os.path.splitext(name)[0])) as f:
        s = json.load(f)["saddles"]
    out = np.zeros(len(s["x_bits"]), A.SADDLE_DTYPE)
    for field, key in (("x", "x_bits"), ("y", "y_bits"), ("k", "k_bits")):
        out[field] = np.array([int(h, 16) for h in s[key]], np.uint32).view(np.float32)
    out["theta"] = np.array(s["theta_deg"], np.float32)
    out["phi"] = np.array(s["phi_deg"], np.float32)
    return out


def yardstick(saddles, cap=1024):
    """orc_try_find_best_board -> (quads [n, 4] or None for -1)."""
    from oracle import oracle as O
    lib = O.lib()
    lib.orc_try_find_best_board.restype = C.c_int
    lib.orc_try_find_best_board.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    s = np.asarray(saddles)
    if s.dtype.names is None:  # an [n, 5] float32 array: the same 20-byte records
        s = np.ascontiguousarray(s, np.float32).reshape(-1, 5).view(O.SADDLE_DTYPE).reshape(-1)
    s = np.ascontiguousarray(s, O.SADDLE_DTYPE)
    q = np.zeros((cap, 4), np.int32)
    n = lib.orc_try_find_best_board(s.ctypes.data, len(s), q.ctypes.data, cap)
    assert n <= cap
    return None if n < 0 else q[:n].copy()


def check_against_yardstick(saddles, what):
    quads, status, n = A.find_board_tail(saddles, cap=1024)
    ref = yardstick(saddles)
    if ref is None:
        assert status == _ffi.AGX_BOARD_NONE and n == 0 and len(quads) == 0, what
    else:
        assert status == _ffi.AGX_BOARD_FOUND and n == len(ref), "%s: status %d, %d quads, yardstick %d" % (what, status, n, len(ref))
        assert np.array_equal(quads.astype(np.int64), ref.astype(np.int64)), what + ": quads or their order"
    return quads, status


@pytest.mark.parametrize("name", ALL_IMAGES)
def test_golden_lists_give_the_yardsticks_quads(name):
    s = golden_list(name)
    quads, status = check_against_yardstick(s, name)
    assert status == _ffi.AGX_BOARD_FOUND and len(quads) > 0, name  # (every fixture image shows a board)


@pytest.mark.parametrize("name", ALL_IMAGES)
def test_detect_by_hand_equals_detect_tail(name):
    """detect's loop (src/detector.rs:510-539) from the two public pieces: find a board, decode its quads, drop the saddles of
    the decoded ones, max_num_of_boards times."""
    s = golden_list(name)
    luma = A.TagDetector.luma8(load_image(name))
    prm = _ffi.Params()
    _ffi.lib().agx_default_params(C.byref(prm))
    tags = {}
    left = s.copy()
    for _ in range(prm.max_num_of_boards):
        quads, status, _n = A.find_board_tail(left, cap=1024)
        if status != _ffi.AGX_BOARD_FOUND:
            continue
        pts = np.stack([left["x"][quads], left["y"][quads]], axis=-1)  # [n, 4, 2]
        out, qst = A.decode_quads_tail("t36h11", luma, pts)
        used = np.zeros(len(left), bool)
        for i in range(len(quads)):
            if qst[i] != _ffi.AGX_QUAD_DECODED:
                continue
            tags[int(out["id"][i])] = np.array(out["xy"][i], np.float32).reshape(4, 2)  # (a repeated id keeps its place, new corners)
            used[quads[i]] = True
        left = left[~used]
    ref = A.TagDetector.detect_tail("t36h11", s, luma)
    assert list(tags) == list(ref), name + ": ids or their order"
    for t in ref:
        assert bits_equal(tags[t], ref[t]), "%s: corners of tag %d" % (name, t)
    assert len(ref) > 0


def test_the_gpu_tests_frames_show_a_board_the_host_form_finds():
    """The oracle's saddle lists of the GPU tests' frames: a board in every one, the score-36 stop in at least half of them,
    the yardstick's quads."""
    from oracle import oracle as O
    from aprilgrid_rs_amd import synth
    frames, _ = synth.render_batch(GPU_FIRST, GPU_FRAMES, *GPU_SIZE)
    full = 0
    for f in range(GPU_FRAMES):
        s = O.refined_saddle_points(frames[f].numpy())
        assert 100 < len(s) <= 1024
        quads, status = check_against_yardstick(s, "synthetic frame %d" % f)
        assert status == _ffi.AGX_BOARD_FOUND and len(quads) >= 30, f
        full += len(quads) == 36
    assert full >= GPU_FRAMES // 2


def raw_call(saddles, n, quads, cap, n_quads=True, status=True):
    nq, st = C.c_uint32(77), C.c_uint32(77)
    rc = _ffi.lib().agx_find_board_tail(saddles, n, quads, cap, C.byref(nq) if n_quads else None, C.byref(st) if status else None)
    return rc, nq.value, st.value


def test_argument_rules():
    s = golden_list("EuRoC.png")
    q = np.zeros((1024, 4), np.uint32)
    assert raw_call(s.ctypes.data, len(s), q.ctypes.data, 1024, n_quads=False)[0] == _ffi.AGX_ERR_ARG
    assert raw_call(s.ctypes.data, len(s), q.ctypes.data, 1024, status=False)[0] == _ffi.AGX_ERR_ARG
    assert raw_call(None, len(s), q.ctypes.data, 1024)[0] == _ffi.AGX_ERR_ARG
    assert raw_call(s.ctypes.data, len(s), None, 1024)[0] == _ffi.AGX_ERR_ARG
    # an empty list: None (:589-591), whatever the pointers
    assert raw_call(None, 0, None, 0) == (_ffi.AGX_OK, 0, _ffi.AGX_BOARD_NONE)
    assert raw_call(s.ctypes.data, 0, q.ctypes.data, 1024) == (_ffi.AGX_OK, 0, _ffi.AGX_BOARD_NONE)


@pytest.mark.parametrize("field", ["x", "y", "theta"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_value_that_is_not_finite_is_board_input(field, value):
    s = golden_list("EuRoC.png")
    s[field][len(s) // 2] = value
    quads, status, n = A.find_board_tail(s, cap=1024)
    assert (status, n, len(quads)) == (_ffi.AGX_BOARD_INPUT, 0, 0)


@pytest.mark.parametrize("field", ["k", "phi"])
def test_k_and_phi_are_never_read(field):
    s = golden_list("EuRoC.png")
    want = A.find_board_tail(s, cap=1024)[0]
    s[field][:] = np.nan
    quads, status, _ = A.find_board_tail(s, cap=1024)
    assert status == _ffi.AGX_BOARD_FOUND and np.array_equal(quads, want)


def test_cap_one_short_is_capacity_with_the_true_count_and_untouched_rows():
    s = golden_list("EuRoC.png")
    want, status, n = A.find_board_tail(s, cap=1024)
    assert status == _ffi.AGX_BOARD_FOUND and n > 1
    q = np.full((n, 4), 0xDEADBEEF, np.uint32)
    assert raw_call(s.ctypes.data, len(s), q.ctypes.data, n - 1) == (_ffi.AGX_OK, n, _ffi.AGX_BOARD_CAPACITY)
    assert (q == 0xDEADBEEF).all()
    assert raw_call(s.ctypes.data, len(s), q.ctypes.data, n) == (_ffi.AGX_OK, n, _ffi.AGX_BOARD_FOUND)
    assert np.array_equal(q, want)


def test_lists_beyond_the_kernels_limits_are_answered_on_the_host():
    """More than 1024 saddles, and thetas outside [-180, 180] (the histogram takes a map): still the yardstick's quads where
    the yardstick's own histogram (keys clamped to [-256, 255]) holds them."""
    s = golden_list("EuRoC.png")
    rng = np.random.default_rng(5)
    pad = np.zeros(1100, A.SADDLE_DTYPE)
    pad["x"] = rng.uniform(2000, 3000, len(pad)).astype(np.float32)  # far from the board, sparse, every theta its own bin
    pad["y"] = rng.uniform(2000, 3000, len(pad)).astype(np.float32)
    pad["theta"] = (np.arange(len(pad)) % 170 - 85).astype(np.float32) + 0.25
    check_against_yardstick(np.concatenate([s, pad]), "EuRoC + 1100 far saddles")
    s2 = s.copy()
    s2["theta"][::7] += 120.0  # (some beyond 180: the host's map path; all within the yardstick's keys)
    assert s2["theta"].max() > 180.0
    check_against_yardstick(s2, "EuRoC with thetas beyond [-180, 180]")


def test_constants_agree_in_header_python_and_rust():
    names = ["AGX_BOARD_FOUND", "AGX_BOARD_NONE", "AGX_BOARD_CAPACITY", "AGX_BOARD_INPUT", "AGX_BOARD_PENDING"]
    header = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for i, name in enumerate(names):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == i, name + " in the header"
        assert getattr(_ffi, name) == i, name + " in _ffi.py"
        m = re.search(r"pub const %s: c_int = (\d+);" % name, rust)
        assert m and int(m.group(1)) == i, name + " in ffi.rs"
    for fn in ("agx_find_boards_enqueue", "agx_find_boards_fetch", "agx_find_board", "agx_find_board_tail"):
        assert re.search(r"\bint %s\(" % fn, header) and ("pub fn %s(" % fn) in rust and fn in _ffi.SYMBOLS, fn
    assert "pub fn find_best_board(refined: &[Saddle]) -> Option<Vec<[usize; 4]>>" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
