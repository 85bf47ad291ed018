"""Which batch is in flight on a handle, pinned as the statuses a fixed sequence of calls returns.

A scenario is a list of steps -- enqueues of the six kinds (saddles, detect, refine, decode, find_boards, planes) and the five
fetches + agx_debug_fetch -- on 2 zero frames of 64 x 48 L8 (4 points, 1 quad, 8 saddles per frame); its result is the list of
statuses.  Every ordered pair of kinds and every kind alone is followed by all six fetches in a fixed order; further scenarios
fetch twice, fetch saddles behind a detect fetch, refuse an enqueue or a fetch in between, refine on the blurred image and on
the plane, use the caller-owned-buffer forms and a group's batch.  The expected lists (tests/golden/batch_state.json) were
recorded once from the build before the handle got its single batch state (`python -m tests.test_gpu_batch_state FILE` writes
them) and are never regenerated from a later build.

Not from the golden file: whenever a fetch refuses (AGX_ERR_STATE) because the batch in flight is another kind's,
agx_last_error names the fetch that resolves that batch."""
import json
import os
import sys

import pytest

from tests import entry_harness as E
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "batch_state.json")
W, H, N = 64, 48, 2
ALL_FETCHES = [("fetch", f) for f in E.FETCHES]


def scenarios():
    """name -> steps; a step is ("enq", kind[, options]) | ("fetch", which[, options])."""
    s = {"nothing enqueued": list(ALL_FETCHES)}  # first: on the fresh handle
    for a in E.KINDS:
        s["%s alone" % a] = [("enq", a)] + ALL_FETCHES
        for b in E.KINDS:
            s["%s then %s" % (a, b)] = [("enq", a), ("enq", b)] + ALL_FETCHES
    for a in E.KINDS[:5]:
        s["%s fetched twice" % a] = [("enq", a), ("fetch", a), ("fetch", a)] + ALL_FETCHES
        s["%s then a refused enqueue" % a] = [("enq", a), ("enq", a, {"format": 99})] + ALL_FETCHES
        s["%s fetch without outputs, then with" % a] = [("enq", a), ("fetch", a, {"null": True}), ("fetch", a)] + ALL_FETCHES
        s["%s to caller-owned buffers" % a] = [("enq", a, {"to": True})] + ALL_FETCHES
        s["%s to caller-owned buffers, fetch without outputs" % a] = [("enq", a, {"to": True}), ("fetch", a, {"null": True})] + ALL_FETCHES
    s["saddles then a refused planes enqueue"] = [("enq", "saddles"), ("enq", "planes", {"format": 99})] + ALL_FETCHES
    s["detect fetch then saddles fetch"] = [("enq", "detect"), ("fetch", "detect"), ("fetch", "saddles"), ("fetch", "debug"), ("fetch", "detect")]
    s["refine on the blurred image"] = [("enq", "saddles"), ("enq", "refine", {"image": 0})] + ALL_FETCHES
    s["refine on the plane"] = [("enq", "saddles"), ("enq", "refine", {"image": 1, "format": E.LF32})] + ALL_FETCHES
    s["refine on the blurred image of a frame without a 9 x 9 window"] = [("enq", "saddles"), ("enq", "refine", {"image": 0, "w": 8})] + ALL_FETCHES
    # a group's batch on the rank's detector: only the group's fetch resolves it
    s["group batch"] = [("enq", "group")] + [("fetch", f, {"rank0": True}) for f in E.FETCHES] + [("group_fetch",)] + \
                       [("fetch", f, {"rank0": True}) for f in E.FETCHES]
    s["group batch then saddles"] = [("enq", "group"), ("enq", "saddles", {"rank0": True})] + \
                                    [("fetch", f, {"rank0": True}) for f in E.FETCHES] + [("group_fetch",)]
    return s


def run(hx, steps):
    """-> (statuses, [(step, in-flight kind, message) of refusals that do not name the in-flight batch's fetch])"""
    statuses, unnamed = [], []
    inflight = {}  # handle -> kind of the unresolved batch
    for step in steps:
        opt = step[2] if len(step) > 2 else {}
        h = hx.rank0 if opt.get("rank0") else hx.h
        key = "rank0" if opt.get("rank0") else "det"
        if step[0] == "enq":
            kind = step[1]
            px = 4 if opt.get("format") == E.LF32 else 1
            w = opt.get("w", W)
            n = 0 if kind == "find" and "format" in opt else N  # (no frames, no format: its refused enqueue is n_frames 0)
            f = (hx.frames, n, w, H, w * px, w * px * H, opt.get("format", E.L8))
            st = hx.enqueue(kind, f, to=opt.get("to", False), image=opt.get("image", 0), h=h)
            if st == E.OK:
                inflight["rank0" if kind == "group" else key] = None if kind in ("planes", "group") else kind
        elif step[0] == "group_fetch":
            st = hx.group_fetch()
        else:
            which = step[1]
            st = hx.fetch(which, null=opt.get("null", False), h=h)
            cur = inflight.get(key)
            if which == cur:
                if st != E.ERR_ARG:  # resolved by its fetch; a saddle batch stays fetchable
                    inflight[key] = cur if cur == "saddles" else None
            elif which != "debug" and st == E.ERR_STATE and cur is not None and E.FETCH_OF[cur] not in hx.last_error(h):
                unnamed.append((step, cur, hx.last_error(h)))
        statuses.append(st)
    return statuses, unnamed


@pytest.fixture(scope="module")
def hx():
    x = E.Harness()
    yield x
    x.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_golden_file_is_complete(golden):
    assert sorted(golden["statuses"]) == sorted(scenarios())
    assert all("%s then %s" % (a, b) in golden["statuses"] for a in E.KINDS for b in E.KINDS) and all("%s alone" % a in golden["statuses"] for a in E.KINDS)


def test_statuses_and_refusal_messages(hx, golden):
    wrong, unnamed = {}, {}
    for name, steps in scenarios().items():
        got, un = run(hx, steps)
        print(name, got)
        if got != golden["statuses"][name]:
            wrong[name] = (got, golden["statuses"][name])
        if un:
            unnamed[name] = un
    assert not wrong, wrong
    assert not unnamed, unnamed


if __name__ == "__main__":  # the recorder: python -m tests.test_gpu_batch_state OUT.json
    x = E.Harness()
    rec, n_unnamed = {"statuses": {}}, 0
    for name, steps in scenarios().items():
        rec["statuses"][name], un = run(x, steps)
        n_unnamed += len(un)
        for step, kind, msg in un:
            print("%s: %s with a %s batch in flight: %r" % (name, step, kind, msg))
    x.close()
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
    print("recorded %d scenarios; %d refusals do not name the fetch" % (len(rec["statuses"]), n_unnamed))
