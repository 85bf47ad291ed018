"""agx_collect_tags_tail -- one round of detect's loop behind its board search and decode (reference src/detector.rs:510-539):
the decoded quads into the tag table, AGX_POINT_USED into the words of their saddles -- against a Python dict insert loop on
synthetic rounds, and the rounds of find_board_tail -> decode_quads_tail -> collect_tags on the golden saddle lists against
agx_detect_tail.  No GPU.

The fourth cause of AGX_TAGS_INPUT, an AGX_BOARD_FOUND count above quads_per_frame, does not exist in the host form, which has no
quads_per_frame (its n_quads IS the length of its arrays): tests/test_gpu_collect_tags.py has it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_find_boards_cpu import golden_list
from tests.util import ALL_IMAGES, ROOT, bits_equal, load_image

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

TAG = A.TagDetector.TAG_DTYPE
FOUND, NONE, B_CAPACITY, B_INPUT, PENDING = 0, 1, 2, 3, 4
T_OK, T_CAPACITY, T_INPUT, T_PENDING = 0, 1, 2, 3
USED = 5
N_CODES = 587  # t36h11
SENT = 0x7E7E7E7E


# ---- the yardstick: detected_tags.insert and indexs_to_remove of :513-536 as a dict loop ------------------------------------
class Model:
    """A frame's state through the rounds: the dict, the status, the would-be count of a CAPACITY round, the words."""

    def __init__(self, n_slots, cap, words=None, n_codes=N_CODES):
        self.tags, self.status, self.count = {}, T_OK, 0
        self.n_slots, self.cap, self.n_codes = n_slots, cap, n_codes
        self.words = np.zeros(n_slots, np.uint32) if words is None else np.array(words, np.uint32)

    def round(self, board_status, quads, qtags, qstatus, n_quads=None, quads_per_frame=None, mark=True):
        if self.status != T_OK:
            return  # sticky
        if board_status == PENDING:
            self.status = T_PENDING
            return
        if board_status == NONE:
            return
        if board_status != FOUND:
            self.status = T_INPUT
            return
        nq = len(quads) if n_quads is None else n_quads
        if quads_per_frame is not None and nq > quads_per_frame:
            self.status = T_INPUT
            return
        dec = [q for q in range(nq) if qstatus[q] == 0]
        if any(qtags["id"][q] >= self.n_codes or (np.asarray(quads[q]) >= self.n_slots).any() for q in dec):
            self.status = T_INPUT
            return
        new = dict(self.tags)
        for q in dec:
            new[int(qtags["id"][q])] = qtags["xy"][q].copy()  # (a repeated id keeps its place, new corners)
        if len(new) > self.cap:
            self.status, self.count = T_CAPACITY, len(new)
            return
        self.tags, self.count = new, len(new)
        if mark:
            for q in dec:
                self.words[np.asarray(quads[q])] = USED

    def rows(self):
        out = np.zeros(len(self.tags), TAG)
        for i, (t, xy) in enumerate(self.tags.items()):
            out["id"][i], out["xy"][i] = t, xy
        return out


def make_round(rng, ids, statuses=None, n_slots=600, slots=None):
    """quads [n, 4], tags [n] (zero unless decoded, as the decode leaves them), statuses [n] of a synthetic round."""
    n = len(ids)
    st = np.zeros(n, np.uint32) if statuses is None else np.array(statuses, np.uint32)
    quads = rng.integers(0, n_slots, (n, 4)).astype(np.uint32) if slots is None else np.array(slots, np.uint32).reshape(n, 4)
    tags = np.zeros(n, TAG)
    for q in range(n):
        if st[q] == 0:
            tags["id"][q] = ids[q]
            tags["xy"][q] = rng.uniform(0, 1000, 8).astype(np.float32)
    return quads, tags, st


class Host:
    """The same state through agx_collect_tags_tail; the table starts as sentinels, so that a row beyond the count that is
    written shows."""

    def __init__(self, n_slots, cap, words=None):
        self.rows_ = np.zeros(cap, TAG)
        self.rows_.view(np.uint32)[:] = SENT
        self.n, self.status, self.cap, self.n_slots = 0, T_OK, cap, n_slots
        self.words = np.zeros(n_slots, np.uint32) if words is None else np.array(words, np.uint32)

    def round(self, board_status, quads, qtags, qstatus, mark=True):
        self.rows_, self.n, self.status, w = A.collect_tags("t36h11", quads, board_status, qtags, qstatus, self.n_slots,
                                                            self.words if mark else None, self.rows_, self.n, self.status, self.cap)
        if mark:
            self.words = w


def same(model, host, what=""):
    assert host.status == model.status, "%s: status %d, the dict loop %d" % (what, host.status, model.status)
    if model.status in (T_OK, T_CAPACITY):
        assert host.n == model.count, "%s: count %d, the dict loop %d" % (what, host.n, model.count)
    want = model.rows()
    assert host.rows_[:len(want)].tobytes() == want.tobytes(), what + ": rows or their order"
    assert (host.rows_[len(want):].view(np.uint32) == SENT).all(), what + ": a row beyond the table was written"
    assert np.array_equal(host.words, model.words), what + ": status words"


def both(n_slots=600, cap=40, words=None):
    return Model(n_slots, cap, words), Host(n_slots, cap, words)


def step(m, h, board_status, r, what="", mark=True):
    m.round(board_status, *r, mark=mark)
    h.round(board_status, *r, mark=mark)
    same(m, h, what)


# ---- 1. synthetic rounds ---------------------------------------------------------------------------------------------------
def test_an_id_repeated_inside_a_round_keeps_the_first_row_and_takes_the_last_corners():
    rng = np.random.default_rng(1)
    m, h = both()
    r = make_round(rng, [7, 3, 7, 9, 3, 7])
    step(m, h, FOUND, r)
    assert list(h.rows_["id"][:h.n]) == [7, 3, 9]
    assert bits_equal(h.rows_["xy"][0], r[1]["xy"][5]) and bits_equal(h.rows_["xy"][1], r[1]["xy"][4])


def test_an_id_repeated_across_rounds_keeps_its_row():
    rng = np.random.default_rng(2)
    m, h = both()
    step(m, h, FOUND, make_round(rng, [5, 6, 7]), "round 1")
    r2 = make_round(rng, [8, 6, 9, 5])
    step(m, h, FOUND, r2, "round 2")
    assert list(h.rows_["id"][:h.n]) == [5, 6, 7, 8, 9]
    assert bits_equal(h.rows_["xy"][0], r2[1]["xy"][3]) and bits_equal(h.rows_["xy"][1], r2[1]["xy"][1])


def test_a_quad_that_only_repeats_an_id_still_marks_its_slots():
    rng = np.random.default_rng(3)
    m, h = both()
    step(m, h, FOUND, make_round(rng, [11, 11], slots=[[0, 1, 2, 3], [10, 11, 12, 13]]))
    assert h.n == 1 and sorted(np.flatnonzero(h.words == USED)) == [0, 1, 2, 3, 10, 11, 12, 13]
    step(m, h, FOUND, make_round(rng, [11], slots=[[20, 21, 22, 599]]), "round 2")
    assert h.n == 1 and (h.words[[20, 21, 22, 599]] == USED).all() and (h.words == USED).sum() == 12


def test_quads_that_were_not_decoded_are_ignored_and_other_words_stay():
    rng = np.random.default_rng(4)
    words = rng.integers(0, 5, 600).astype(np.uint32)  # REFINED .. FILTERED
    m, h = both(words=words)
    ids = [1, 2, 3, 4, 5, 6, 7]
    r = make_round(rng, ids, statuses=[1, 0, 2, 3, 0, 4, 5])
    r[1]["id"][[0, 2, 3, 5, 6]] = [600, 700, 800, 900, 1000]  # what a slot that was not decoded holds is never looked at
    r[0][0] = [9999, 0, 0, 0]
    step(m, h, FOUND, r)
    assert list(h.rows_["id"][:h.n]) == [2, 5]
    untouched = np.setdiff1d(np.arange(600), np.concatenate([r[0][1], r[0][4]]))
    assert np.array_equal(h.words[untouched], words[untouched])
    # a round that decodes nothing changes nothing
    step(m, h, FOUND, make_round(rng, [1, 2], statuses=[4, 2]), "nothing decoded")
    assert h.n == 2


def test_tag_cap_reached_is_ok_one_over_is_capacity_and_sticky():
    rng = np.random.default_rng(5)
    m, h = both(cap=40)
    step(m, h, FOUND, make_round(rng, list(range(100, 130)) + [100, 101]), "round 1")
    step(m, h, FOUND, make_round(rng, list(range(125, 135)) + [200, 201, 202, 203, 204]), "round 2: row 40 exactly")
    assert (h.status, h.n) == (T_OK, 40)
    rows, words = h.rows_.copy(), h.words.copy()
    step(m, h, FOUND, make_round(rng, [300, 100, 301, 300]), "one over")
    assert (h.status, h.n) == (T_CAPACITY, 42)  # the would-be count
    assert h.rows_.tobytes() == rows.tobytes() and np.array_equal(h.words, words)
    step(m, h, FOUND, make_round(rng, [100]), "sticky")
    step(m, h, PENDING, make_round(rng, []), "sticky")
    assert (h.status, h.n) == (T_CAPACITY, 42) and h.rows_.tobytes() == rows.tobytes() and np.array_equal(h.words, words)
    # needing row 41 from an empty table
    m, h = both(cap=40)
    step(m, h, FOUND, make_round(rng, list(range(41))), "41 ids")
    assert (h.status, h.n) == (T_CAPACITY, 41) and not (h.words == USED).any()


@pytest.mark.parametrize("cause", ["board capacity", "board input", "no board status", "id", "slot"])
def test_every_cause_of_tags_input_is_decided_before_anything_is_written(cause):
    rng = np.random.default_rng(6)
    m, h = both()
    step(m, h, FOUND, make_round(rng, [1, 2, 3]), "round 1")
    rows, words = h.rows_.copy(), h.words.copy()
    ids, slots, bs = [4, 5, 586], rng.integers(0, 600, (3, 4)), FOUND
    slots[1, 2] = 599
    if cause == "id":
        step(m, h, FOUND, make_round(rng, ids, slots=slots), "586 and 599 are accepted")
        assert h.status == T_OK and h.n == 6
        rows, words = h.rows_.copy(), h.words.copy()
        ids = [7, 8, 587]
    elif cause == "slot":
        slots[2, 3] = 600
    else:
        bs = {"board capacity": B_CAPACITY, "board input": B_INPUT, "no board status": 9}[cause]
    step(m, h, bs, make_round(rng, ids, slots=slots), cause)
    assert h.status == T_INPUT and h.rows_.tobytes() == rows.tobytes() and np.array_equal(h.words, words)
    step(m, h, FOUND, make_round(rng, [20, 21]), "sticky")
    assert h.status == T_INPUT and h.rows_.tobytes() == rows.tobytes() and np.array_equal(h.words, words)


def test_pending_none_and_no_quads():
    rng = np.random.default_rng(7)
    m, h = both()
    step(m, h, NONE, make_round(rng, [1, 2]), "NONE first")  # (the quads of a frame without a board are never looked at)
    step(m, h, FOUND, make_round(rng, []), "n_quads == 0")
    assert (h.status, h.n) == (T_OK, 0)
    step(m, h, FOUND, make_round(rng, [1, 2]), "a board")
    step(m, h, NONE, make_round(rng, [3]), "NONE: the loop runs on")
    step(m, h, FOUND, make_round(rng, [3]), "and on")
    assert (h.status, list(h.rows_["id"][:h.n])) == (T_OK, [1, 2, 3])
    rows, words = h.rows_.copy(), h.words.copy()
    step(m, h, PENDING, make_round(rng, [4]), "PENDING")
    assert h.status == T_PENDING and h.n == 3 and h.rows_.tobytes() == rows.tobytes() and np.array_equal(h.words, words)
    step(m, h, FOUND, make_round(rng, [4]), "sticky")
    assert h.status == T_PENDING and h.n == 3


def test_without_point_status_nothing_is_marked_but_slots_are_still_bounded():
    rng = np.random.default_rng(8)
    m, h = both()
    step(m, h, FOUND, make_round(rng, [1, 2, 3]), mark=False)
    assert h.n == 3 and not h.words.any()
    step(m, h, FOUND, make_round(rng, [4], slots=[[0, 1, 2, 600]]), mark=False)
    assert h.status == T_INPUT


def test_random_rounds_equal_the_dict_loop():
    rng = np.random.default_rng(9)
    for trial in range(200):
        cap = int(rng.integers(1, 50))
        m, h = both(n_slots=300, cap=cap)
        for r in range(4):
            n = int(rng.integers(0, 140))
            ids = rng.integers(0, int(rng.choice([8, 60, 587])), n)
            st = rng.choice([0, 0, 0, 1, 2, 3, 4, 5], n)
            bs = int(rng.choice([FOUND] * 8 + [NONE, PENDING]))
            step(m, h, bs, make_round(rng, ids, st, n_slots=300), "trial %d round %d" % (trial, r), mark=bool(rng.integers(0, 4)))


# ---- 2. the rounds on the golden lists against agx_detect_tail ---------------------------------------------------------------
def host_rounds(records, words, luma, rounds, family="t36h11", tag_cap=N_CODES):
    """detect's loop (src/detector.rs:510-539) from the three public host pieces over a saddle list that is never compacted: only
    the status words change.  records: SADDLE_DTYPE [n]; words: uint32 [n] (0 = listed).  find_board_tail has no words of its
    own, so it gets the listed records and its indices are mapped back.  -> (rows TAG_DTYPE, tag status, the words)."""
    records = np.asarray(records)
    if records.dtype != A.SADDLE_DTYPE:
        records = np.ascontiguousarray(records, np.float32).reshape(-1, 5).view(A.SADDLE_DTYPE).reshape(-1)
    words = np.array(words, np.uint32)
    tags, n_tags, status = None, 0, T_OK
    for _ in range(rounds):
        listed = np.flatnonzero(words == 0)
        quads, bstatus, _n = A.find_board_tail(records[listed], cap=1024)
        quads = listed[quads.astype(np.int64)].astype(np.uint32).reshape(-1, 4)
        if len(quads):
            pts = np.stack([records["x"][quads], records["y"][quads]], axis=-1)
            qtags, qstatus = A.decode_quads_tail(family, luma, pts)
        else:
            qtags, qstatus = np.zeros(0, TAG), np.zeros(0, np.uint32)
        tags, n_tags, status, words = A.collect_tags(family, quads, bstatus, qtags, qstatus, len(words), words, tags, n_tags, status, tag_cap)
    return (tags[:n_tags] if tags is not None else np.zeros(0, TAG)), status, words


@pytest.mark.parametrize("name", ALL_IMAGES)
def test_the_rounds_on_a_golden_list_equal_detect_tail(name):
    s = golden_list(name)
    luma = A.TagDetector.luma8(load_image(name))
    for boards in (1, 2, 3):
        prm = A.DetectorParams.default_params()
        prm.max_num_of_boards = boards
        ref = A.TagDetector.detect_tail("t36h11", s, luma, prm)
        rows, status, _ = host_rounds(s, np.zeros(len(s), np.uint32), luma, boards)
        assert status == T_OK
        assert [int(t) for t in rows["id"]] == list(ref), "%s, %d boards: ids or their order" % (name, boards)
        for i, t in enumerate(ref):
            assert bits_equal(rows["xy"][i].reshape(4, 2), ref[t]), "%s, %d boards: corners of tag %d" % (name, boards, t)
        if name == "two_boards.png":
            assert len(rows) == {1: 36, 2: 72, 3: 72}[boards]
        assert len(rows) > 0


# ---- 3. arguments of the host form, constants and declarations ----------------------------------------------------------------
def raw(family=3, n_quads=2, quads=True, board_status=FOUND, quad_tags=True, quad_status=True, n_slots=600, point_status=True,
        tag_cap=8, tags=True, n_tags=True, tag_status=True):
    rng = np.random.default_rng(10)
    q, t, s = make_round(rng, [1, 2])
    words, rows = np.zeros(600, np.uint32), np.zeros(8, TAG)
    n, st = C.c_uint32(0), C.c_uint32(0)
    p = lambda a, on: a.ctypes.data if on else None
    rc = _ffi.lib().agx_collect_tags_tail(family, n_quads, p(q, quads), board_status, p(t, quad_tags), p(s, quad_status), n_slots,
                                          p(words, point_status), tag_cap, p(rows, tags), C.byref(n) if n_tags else None,
                                          C.byref(st) if tag_status else None)
    return rc, n.value, st.value


def test_argument_rules_of_the_host_form():
    assert raw() == (_ffi.AGX_OK, 2, T_OK)
    assert raw(point_status=False) == (_ffi.AGX_OK, 2, T_OK)
    for bad in ("quads", "quad_tags", "quad_status", "tags", "n_tags", "tag_status"):
        assert raw(**{bad: False})[0] == _ffi.AGX_ERR_ARG, bad
    assert raw(tag_cap=0)[0] == _ffi.AGX_ERR_ARG
    assert raw(family=17)[0] == _ffi.AGX_ERR_FAMILY
    # nothing of the quads is read where there are none, or no board
    assert raw(n_quads=0, quads=False, quad_tags=False, quad_status=False) == (_ffi.AGX_OK, 0, T_OK)
    assert raw(board_status=NONE, quads=False, quad_tags=False, quad_status=False) == (_ffi.AGX_OK, 0, T_OK)
    assert raw(board_status=PENDING, quads=False, quad_tags=False, quad_status=False) == (_ffi.AGX_OK, 0, T_PENDING)
    # a smaller family bounds the ids: t16h5 has 30 codes
    rng = np.random.default_rng(11)
    r = make_round(rng, [29])
    assert A.collect_tags("t16h5", r[0], FOUND, r[1], r[2], 600)[1:3] == (1, T_OK)
    r = make_round(rng, [30])
    assert A.collect_tags("t16h5", r[0], FOUND, r[1], r[2], 600)[1:3] == (0, T_INPUT)


def test_constants_and_declarations_agree_in_header_python_and_rust():
    header = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name, value in (("AGX_TAGS_OK", 0), ("AGX_TAGS_CAPACITY", 1), ("AGX_TAGS_INPUT", 2), ("AGX_TAGS_PENDING", 3), ("AGX_POINT_USED", 5)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name + " in the header"
        assert getattr(_ffi, name) == value, name + " in _ffi.py"
        m = re.search(r"pub const %s: c_int = (\d+);" % name, rust)
        assert m and int(m.group(1)) == value, name + " in ffi.rs"
    for fn, n_args in (("agx_collect_tags_enqueue", 16), ("agx_collect_tags_tail", 12)):
        assert re.search(r"\bint %s\(" % fn, header) and ("pub fn %s(" % fn) in rust, fn
        assert len(_ffi.SYMBOLS[fn][1]) == n_args, fn
    assert "pub fn collect_tags_tail(" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"#define AGX_ABI_VERSION 1\b", header)
    assert "agx_collect_tags_enqueue" in header.split("int agx_find_boards_enqueue(")[0].rsplit("d_point_status NULL, or one word per slot", 1)[1]
