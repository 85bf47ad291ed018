"""The three per-frame list limits of agx_detector_set_limits AT their bounds: a limit equal to a frame's true count changes
nothing, a limit one below voids exactly that frame (AGX_ERR_CAPACITY, no record anywhere) and leaves the rest of the batch
byte-identical -- on the three sparse paths and the generic path alike, through every entry that reads the limits, on a handle
whose workspace is reused at smaller strides, and with guard bytes around every list.

Where the bounds come from (tests/limit_cases.py, tests/test_limit_cases_cpu.py): n_saddles, n_clusters, n_candidates are the
oracle's; the device counters of an unlimited run must agree with them before any limit is set.  max_clusters bounds TWO lists,
the cluster list and the flood seed list in front of it, and the seed list is the longer one (at least one seed per cluster):
B_clusters(frame) = the `seeds` counter of the unlimited run, on every path -- the seeds are listed on the generic path too.
A seed list one short sets AGX_FRAME_CANDIDATE_OVERFLOW (SEED_OVERFLOW_BIT below: the bit the seed appends raise today).

Which max_saddles leg reaches which emission form (asserted from last_sparse_path, flag 16 and flag 64):
  mixed batch, sparse_path 1           emit_wide (k_rare, at most 1024 refined records)            frames without flag 16 / 64
  mixed batch, sparse_path 2 / 3       emit_wide_lds (records in LDS), the tail of k_sparse_frame   frames without flag 16 / 64
  the generic-path frame, every path   rare_frame behind generic_frame                              flag 16
  the large-list frame, sparse_path 1  emit_large_split (eight workgroups)                          flag 64, refined > 1024
  the large-list frame, sparse_path 2  filter_sort_emit inside k_sparse_frame                       flag 64, refined > 1024"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import limit_cases as L
from tests import patch_oracle, sigma_oracle
from tests.util import bits_equal, check_frame, check_saddles

pytestmark = pytest.mark.gpu

AGX_ERR_CAPACITY = -3
CAND, CLUSTER, SADDLE, GENERIC, LARGE = 1, 2, 4, 16, 64  # AGX_FRAME_*
OVERFLOW = CAND | CLUSTER | SADDLE
SEED_OVERFLOW_BIT = CAND  # what a flood seed list beyond max_clusters sets (include/aprilgrid_amd.h, DESIGN.md "List capacities")
SENT = 0xFFC0FFEE  # every word of an output buffer before a fetch
CONFIGS = {"path1": (1, 0), "path2": (2, 0), "path3": (3, 0), "generic": (1, 1)}  # sparse_path, force_generic
GENERIC_CONFIGS = {"generic1": (1, 1), "generic2": (2, 1), "generic3": (3, 1)}
ALL_CONFIGS = dict(CONFIGS, **GENERIC_CONFIGS)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


def A():
    import aprilgrid_rs_amd
    return aprilgrid_rs_amd


def make(cfg, guarded=False, **kw):
    path, generic = ALL_CONFIGS[cfg]
    if guarded:
        os.environ["AGX_REDZONE_BYTES"] = str(1 << 16)
    try:
        d = A().TagDetector("t36h11", None, device=0, **kw)
    finally:
        os.environ.pop("AGX_REDZONE_BYTES", None)
    d.set_option("sparse_path", path)
    d.set_option("force_generic", generic)
    return d


def cuda(frames):
    import torch
    return torch.from_numpy(np.array(frames)).cuda()


class Run:
    """One batch fetched into a buffer full of SENT: status, counts, the rows as words [n, cap, 5], the device counters."""

    def __init__(self, d, frames, cap):
        n = len(frames)
        d.saddles_batch_enqueue(frames)
        out = np.empty((n, cap), A().SADDLE_DTYPE)
        self.rows = out.view(np.uint32).reshape(n, cap, 5)
        self.rows[...] = SENT
        self.counts, self.status = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        self.rc = d.saddles_batch_fetch_into(out, self.counts, self.status)
        self.ctr = [d.debug_fetch(i, "counters") for i in range(n)]
        self.path = d.get_option("last_sparse_path")
        self.out = out

    def records(self, i):
        return self.out[i, : self.counts[i]] if self.status[i] == 0 else self.out[i, :0]

    def flags(self, i):
        return self.ctr[i]["flags"]


def assert_ok_as(r, base, i, what, counters=True):
    """Frame i of r is OK and byte-identical to frame i of the unlimited run; nothing is written behind its list."""
    assert r.status[i] == 0 and not (r.flags(i) & OVERFLOW), "%s: status %d flags %#x" % (what, r.status[i], r.flags(i))
    assert r.counts[i] == base.counts[i] and r.records(i).tobytes() == base.records(i).tobytes(), "%s: records differ from the unlimited run" % what
    assert (r.rows[i, r.counts[i]:] == SENT).all(), "%s: a row behind the list was written" % what
    if counters:
        assert r.ctr[i] == base.ctr[i], "%s: counters %s, unlimited %s" % (what, r.ctr[i], base.ctr[i])


def assert_void(r, i, what, exactly=None):
    """Frame i reads AGX_ERR_CAPACITY with no record anywhere in its rows, and an overflow bit (`exactly`: that bit alone)."""
    assert r.status[i] == AGX_ERR_CAPACITY, "%s: status %d, flags %#x, counters %s" % (what, r.status[i], r.flags(i), r.ctr[i])
    assert (r.rows[i] == SENT).all(), "%s: a record of the void frame was written" % what
    assert r.flags(i) & OVERFLOW, "%s: no overflow bit in %#x" % (what, r.flags(i))
    if exactly is not None:
        assert r.flags(i) & OVERFLOW == exactly, "%s: overflow bits %#x, expected %#x alone" % (what, r.flags(i) & OVERFLOW, exactly)


def signature(r):
    """What must agree between the paths: status, overflow and informational flag bits, records."""
    return [(int(r.status[i]), r.flags(i) & (OVERFLOW | LARGE), r.records(i).tobytes()) for i in range(len(r.status))]


def limit_kw(which, value):
    return {"saddles": dict(max_saddles=value), "clusters": dict(max_clusters=value), "candidates": dict(max_candidates=value)}[which]


def bounds(which, counts, base):
    """Per frame, the smallest limit at which the frame succeeds."""
    if which == "saddles":
        return [c["n_saddles"] for c in counts]
    if which == "candidates":
        return [c["n_candidates"] for c in counts]
    return [c["seeds"] for c in base.ctr]  # (seeds >= clusters: asserted with the other premises)


def at_and_below(d, frames, base, which, counts, what, exactly=None, check=None):
    """Legs 1 and 2 of one limit on one detector: limit = B reproduces the unlimited run, limit = B - 1 voids frame F alone.
    -> (F, B, signature at B, signature at B - 1)."""
    b = bounds(which, counts, base)
    f = L.unique_argmax(b, "bound of %s (%s)" % (which, what))
    B = b[f]
    assert B >= 2, "premise: the bound %d of %s leaves no explicit limit below it" % (B, which)
    cap = base.rows.shape[1]
    d.set_limits(**limit_kw(which, B))
    at = Run(d, frames, cap)
    for i in range(len(counts)):
        assert_ok_as(at, base, i, "%s, %s = %d (its bound), frame %d" % (what, which, B, i))
        if check is not None:
            check(d, at, i)
    d.set_limits(**limit_kw(which, B - 1))
    below = Run(d, frames, cap)
    for i in range(len(counts)):
        w = "%s, %s = %d (one below the bound of frame %d), frame %d" % (what, which, B - 1, f, i)
        if i == f:
            assert_void(below, i, w, exactly)
        else:
            # (the byte-identity of F's neighbours is also the evidence that F wrote nothing into their lists)
            assert_ok_as(below, base, i, w)
    d.set_limits(0, 0, 0)
    return f, B, signature(at), signature(below)


# ---- the frames, their oracle counts and the unlimited runs -----------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    frames = L.batch()
    return frames, cuda(frames), [L.oracle_counts(f) for f in frames]


@pytest.fixture(scope="module")
def large():
    f = L.large_frame()[None]
    return f, cuda(f), [L.oracle_counts(f[0])]


@pytest.fixture(scope="module")
def unlimited(mixed):
    """cfg -> the mixed batch with no limit set (computed once per configuration)."""
    runs = {}

    def get(cfg):
        if cfg not in runs:
            d = make(cfg)
            runs[cfg] = Run(d, mixed[1], max(c["n_saddles"] for c in mixed[2]) + 2)
            d.close()
        return runs[cfg]
    return get


def oracle_check(oracle, host):
    def check(d, r, i):
        ref = check_frame(d, oracle, host[i], i, "frame %d" % i)
        check_saddles(r.records(i), ref, "frame %d" % i)
    return check


# ---- 0. premises ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(ALL_CONFIGS))
def test_counters_of_an_unlimited_run_are_the_oracles_counts(oracle, mixed, unlimited, cfg):
    host, dev, counts = mixed
    path, generic = ALL_CONFIGS[cfg]
    d = make(cfg)
    r = Run(d, dev, unlimited(cfg).rows.shape[1])
    assert r.path == path, "premise: sparse_path %d ran as %d" % (path, r.path)
    for i, c in enumerate(counts):
        what = "premise (%s, %s)" % (cfg, L.NAMES[i])
        ctr = r.ctr[i]
        print(what, ctr, c)
        assert r.status[i] == 0 and not (ctr["flags"] & OVERFLOW), what
        assert ctr["saddles"] == c["n_saddles"] == r.counts[i], "%s: saddles counter" % what
        assert ctr["clusters"] == c["n_clusters"], "%s: clusters counter" % what
        assert ctr["seeds"] >= c["n_clusters"], "%s: fewer seeds than clusters" % what
        assert ctr["refined"] == c["n_refined"] <= 1024 and not (ctr["flags"] & LARGE), "%s: refined counter" % what
        if generic:
            assert ctr["generic_candidates"] == c["n_candidates"], "%s: generic_candidates counter" % what
            assert ctr["generic_roots"] == c["n_clusters"], "%s: generic_roots counter" % what
        # flag 16: the generic-path frame takes that path by itself, no other frame does (under force_generic no flood runs and
        # nothing raises the flag: the generic_candidates counter above shows that the generic kernels ran)
        assert bool(ctr["flags"] & GENERIC) == (i == L.I_BIG and not generic), "%s: AGX_FRAME_GENERIC_PATH in %#x" % (what, ctr["flags"])
        oracle_check(oracle, host)(d, r, i)
        assert_ok_as(r, unlimited(cfg), i, what + ", second unlimited run")
        assert ctr["seeds"] == unlimited("path1").ctr[i]["seeds"], "%s: the seed list differs between the paths" % what
    d.close()


# ---- 1-3. each limit at its bound and one below, on every path ---------------------------------------------------------------
@pytest.mark.parametrize("which,cfgs,exactly", [("saddles", list(CONFIGS), SADDLE), ("clusters", list(CONFIGS), SEED_OVERFLOW_BIT),
                                                ("candidates", list(GENERIC_CONFIGS), CAND)])
def test_limit_at_its_bound_and_one_below_on_every_path(oracle, mixed, unlimited, which, cfgs, exactly):
    """max_candidates binds only where the generic path runs: its legs run under force_generic on the three sparse paths."""
    host, dev, counts = mixed
    sigs = {}
    for cfg in cfgs:
        d = make(cfg)
        sigs[cfg] = at_and_below(d, dev, unlimited(cfg), which, counts, cfg, exactly, oracle_check(oracle, host))
        d.close()
    first = sigs[cfgs[0]]
    assert first[0] == (L.I_BIG if which == "candidates" else L.I_NOISE)
    for cfg in cfgs[1:]:
        assert sigs[cfg][:2] == first[:2], "the bound of %s differs between %s and %s" % (which, cfgs[0], cfg)
        for leg, name in ((2, "at the bound"), (3, "one below")):
            for i, (a, b) in enumerate(zip(sigs[cfg][leg], first[leg])):
                assert a == b, "%s %s: frame %d differs between %s and %s: %s / %s" % (which, name, i, cfg, cfgs[0], a[:2], b[:2])


@pytest.mark.parametrize("path", [1, 2, 3])
def test_max_candidates_on_the_frame_that_takes_the_generic_path_by_itself(oracle, mixed, path):
    host, dev, counts = mixed
    pick = [0, L.I_BIG, L.I_FLAT]
    sub, csub = cuda(host[pick]), [counts[i] for i in pick]
    d = make("path%d" % path)
    base = Run(d, sub, max(c["n_saddles"] for c in csub) + 2)
    assert base.flags(1) & GENERIC and not base.flags(0) & GENERIC, "premise: flag 16 of the generic-path frame alone"
    assert base.ctr[1]["generic_candidates"] == csub[1]["n_candidates"], "premise: generic_candidates counter"
    # (the board's candidates are fewer, and no list of a frame on the flood paths is bounded by max_candidates)
    f, B, _, _ = at_and_below(d, sub, base, "candidates", csub, "sparse_path %d" % path, CAND, oracle_check(oracle, host[pick]))
    assert f == 1 and B == counts[L.I_BIG]["n_candidates"]
    d.close()


# ---- emission forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2, 3])
def test_max_saddles_on_the_generic_path_frame(oracle, mixed, path):
    host, dev, counts = mixed
    one, c = cuda(host[L.I_BIG:L.I_BIG + 1]), [counts[L.I_BIG]]
    d = make("path%d" % path)
    base = Run(d, one, c[0]["n_saddles"] + 2)
    assert base.path == path and base.flags(0) & GENERIC, "premise: the frame takes the generic path on sparse_path %d" % path
    assert base.counts[0] == c[0]["n_saddles"]
    at_and_below(d, one, base, "saddles", c, "generic-path frame, sparse_path %d" % path, SADDLE, oracle_check(oracle, host[L.I_BIG:]))
    d.close()


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("which", ["saddles", "clusters"])
def test_limits_on_the_large_list_frame(oracle, large, path, which):
    """More than 1024 refined records: eight workgroups emit the frame on path 1, the frame's own workgroup on path 2.  With
    max_saddles at its bound (below 1024) the LDS list keeps 1024 entries and the records sort in global memory."""
    host, dev, counts = large
    d = make("path%d" % path)
    base = Run(d, dev, counts[0]["n_saddles"] + 2)
    c = base.ctr[0]
    assert base.path == path
    assert c["refined"] == counts[0]["n_refined"] > 1024, "premise: refined %d, oracle %d" % (c["refined"], counts[0]["n_refined"])
    assert c["flags"] & LARGE and not c["flags"] & GENERIC, "premise: AGX_FRAME_LARGE_RESULT in %#x" % c["flags"]
    assert c["saddles"] == counts[0]["n_saddles"] and c["clusters"] == counts[0]["n_clusters"] <= c["seeds"]
    at_and_below(d, dev, base, which, counts, "large list, sparse_path %d" % path, SADDLE if which == "saddles" else SEED_OVERFLOW_BIT,
                 oracle_check(oracle, host))
    d.close()


# ---- 4. one handle, in sequence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["path1", "path2", "generic"])
def test_one_handle_in_sequence(mixed, unlimited, cfg):
    """unlimited, B, B - 1, set_limits(0, 0, 0), unlimited -- on ONE detector, for each limit in turn: the lowered limits reuse
    the larger allocation at smaller per-frame strides, and the batch after a voided one starts from its leftovers."""
    host, dev, counts = mixed
    d = make(cfg)
    base = unlimited(cfg)
    cap = base.rows.shape[1]
    for which in ("saddles", "clusters") + (("candidates",) if ALL_CONFIGS[cfg][1] else ()):
        first = Run(d, dev, cap)
        at_and_below(d, dev, first, which, counts, "%s in sequence" % cfg)  # (ends with set_limits(0, 0, 0))
        last = Run(d, dev, cap)
        for i in range(len(counts)):
            assert_ok_as(first, base, i, "%s, before %s, frame %d" % (cfg, which, i))
            assert_ok_as(last, base, i, "%s, after %s, frame %d" % (cfg, which, i))
    d.close()


# ---- other entries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_packed_slab_of_exactly_the_batch_and_one_record_short(mixed, unlimited, path):
    import torch
    host, dev, counts = mixed
    base = unlimited("path%d" % path)
    n, total = len(counts), sum(c["n_saddles"] for c in counts)
    d = make("path%d" % path)
    for cap in (total, total - 1):
        slab = torch.full((total + 8, 5), float("nan"), dtype=torch.float32, device="cuda")
        slab.view(torch.int32)[...] = SENT - (1 << 32)
        table = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        d.saddles_batch_enqueue_to(dev, slab[:cap], table)
        d.sync()
        words, t = slab.cpu().numpy().view(np.uint32), table.cpu().numpy().view(np.uint32)
        ok = [i for i in range(n) if t[i, 2] & OVERFLOW == 0]
        spans = sorted((int(t[i, 1]), int(t[i, 1] + t[i, 0])) for i in ok if t[i, 0])
        for i in range(n):
            what = "slab of %d records, frame %d: row %s" % (cap, i, t[i])
            if i in ok:
                assert t[i, 0] == counts[i]["n_saddles"] and t[i, 1] + t[i, 0] <= cap, what
                assert words[t[i, 1]: t[i, 1] + t[i, 0]].tobytes() == base.records(i).tobytes(), what + ": list"
            else:
                assert t[i, 2] & OVERFLOW == SADDLE and t[i, 0] == 0, what
            assert t[i, 3] == counts[i]["n_clusters"], what
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "slab of %d: lists overlap: %s" % (cap, spans)
        assert (words[cap:] == SENT).all(), "slab of %d records: written at or beyond its capacity" % cap
        if cap == total:
            assert len(ok) == n and spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans
        else:
            assert len(ok) < n, "a slab one record short held every list"
            used = np.zeros(total + 8, bool)
            for a, b in spans:
                used[a:b] = True
            assert (words[~used] == SENT).all(), "a record outside every OK frame's list was written"
    d.close()


def test_fetch_with_cap_per_frame_at_the_longest_list_and_one_below(mixed, unlimited):
    host, dev, counts = mixed
    base = unlimited("path1")
    f = L.unique_argmax([c["n_saddles"] for c in counts], "n_saddles")
    B = counts[f]["n_saddles"]
    d = make("path1")
    at = Run(d, dev, B)
    assert at.rc == 0
    for i in range(len(counts)):
        assert_ok_as(at, base, i, "cap_per_frame %d, frame %d" % (B, i))
    below = Run(d, dev, B - 1)
    assert below.rc == AGX_ERR_CAPACITY
    for i in range(len(counts)):
        if i == f:
            assert below.status[i] == AGX_ERR_CAPACITY and below.counts[i] == B, (below.status[i], below.counts[i])  # the true count
            assert (below.rows[i] == SENT).all(), "a row of the frame that does not fit was written"
            assert not below.flags(i) & OVERFLOW  # (the caller's buffer is short, not a list of the detector)
        else:
            assert_ok_as(below, base, i, "cap_per_frame %d, frame %d" % (B - 1, i))
    d.close()


@pytest.mark.parametrize("path", [1, 2])
def test_single_host_frame_at_cap_and_max_saddles(oracle, mixed, path):
    """agx_refined_saddle_points: one frame, the list in the pinned mirror."""
    host, dev, counts = mixed
    img, n = np.ascontiguousarray(host[1]), counts[1]["n_saddles"]
    ref = oracle.refined_saddle_points(img)
    d = make("path%d" % path)

    def call(cap):
        buf = np.empty((cap + 1, 5), np.uint32)
        buf[...] = SENT
        got = C.c_uint32(12345)
        st = d._lib.agx_refined_saddle_points(d._h, img.ctypes.data, L.W, L.H, L.W, 0, buf.ctypes.data, cap, C.byref(got))
        return st, got.value, buf

    st, got, buf = call(n)
    assert (st, got) == (0, n) and (buf[n] == SENT).all()
    check_saddles(buf[:n].view(np.float32).copy().view(A().SADDLE_DTYPE).reshape(-1), ref, "cap = n")
    st, got, buf = call(n - 1)
    assert (st, got) == (AGX_ERR_CAPACITY, n), (st, got)
    assert (buf == SENT).all(), "a list that does not fit was written in part"
    d.set_limits(max_saddles=n)
    st, got, buf = call(n)
    assert (st, got) == (0, n)
    check_saddles(buf[:n].view(np.float32).copy().view(A().SADDLE_DTYPE).reshape(-1), ref, "max_saddles = n")
    d.set_limits(max_saddles=n - 1)
    st, got, buf = call(n)
    assert st == AGX_ERR_CAPACITY and (buf == SENT).all(), (st, got)
    assert d.debug_fetch(0, "counters")["flags"] & OVERFLOW == SADDLE
    d.set_limits(0, 0, 0)
    check_saddles(d.refined_saddle_points(img, as_array=True), ref, "after the reset")
    d.close()


@pytest.mark.parametrize("device_tail", [1, 0])
def test_detect_batch_with_max_saddles_one_below(mixed, device_tail):
    host, dev, counts = mixed
    pick = [0, 1, 2, L.I_FLAT]
    sub, csub = cuda(host[pick]), [counts[i] for i in pick]
    f = L.unique_argmax([c["n_saddles"] for c in csub], "n_saddles of the boards")
    B = csub[f]["n_saddles"]
    d = make("path1")
    try:
        d.set_option("device_tail", device_tail)
    except A().AgxError as e:  # this process's atan2f is not the routine the kernel restates: the device tail is refused
        d.close()
        if device_tail == 1 and e.status == A()._ffi.AGX_ERR_STATE:
            pytest.skip("device tail refused on this host (AGX_ERR_STATE)")
        raise

    def detect():
        d.detect_batch_enqueue(sub, cap=64)
        rc, out, cnt, st = d.detect_batch_fetch_raw(0)
        return rc, out, cnt, st

    rc0, out0, cnt0, st0 = detect()
    assert rc0 == 0 and (st0 == 0).all() and (cnt0[:3] >= 20).all() and cnt0[3] == 0, (rc0, st0, cnt0)
    d.set_limits(max_saddles=B)
    rc, out, cnt, st = detect()
    assert rc == 0 and np.array_equal(cnt, cnt0) and out.tobytes() == out0.tobytes(), "max_saddles at its bound changes the tags"
    d.set_limits(max_saddles=B - 1)
    rc, out, cnt, st = detect()
    assert rc == AGX_ERR_CAPACITY
    for i in range(len(pick)):
        if i == f:
            assert st[i] == AGX_ERR_CAPACITY and cnt[i] == 0 and not out[i].tobytes().strip(b"\0"), (i, st[i], cnt[i])
        else:
            assert st[i] == 0 and cnt[i] == cnt0[i] and out[i].tobytes() == out0[i].tobytes(), "frame %d beside the void frame" % i
    d.close()


@pytest.mark.parametrize("mode", ["half_size_patch_3", "blur_sigma_2", "chain_refine_general"])
def test_deferred_refinement_and_any_sigma_front(mixed, mode):
    """half_size_patch 3: k_refine_clusters behind flood stages that only cluster; sigma 2: the any-sigma response front;
    chain_refine_general: the deferred plan at the reference's half 2 -- k_refine_clusters appends through the same append_refined
    as the fused kernels, and the seed list one short must void the frame there too."""
    host, dev, counts = mixed
    pick = [0, 1, 2, L.I_NOISE, L.I_FLAT]
    sub = cuda(host[pick])
    if mode == "half_size_patch_3":
        kw, orc = dict(half_size_patch=3), (lambda img: patch_oracle.refined_saddle_points(img, 1.5, 3))
    elif mode == "blur_sigma_2":
        kw, orc = dict(blur_sigma=2.0), (lambda img: sigma_oracle.refined_saddle_points(img, 2.0))
    else:
        kw, orc = dict(), (lambda img: patch_oracle.refined_saddle_points(img, 1.5, 2))
    refs = [orc(np.ascontiguousarray(host[i])) for i in pick]
    csub = [L.counts_of(*r) for r in refs]
    d = make("path1", **kw)
    if mode == "chain_refine_general":
        d.set_option("chain_refine_general", 1)
    base = Run(d, sub, max(c["n_saddles"] for c in csub) + 2)
    assert d.get_option("last_chain_refine") == (0 if mode == "blur_sigma_2" else 1), "premise: the plan that ran"
    for i, (c, (ref, dbg)) in enumerate(zip(csub, refs)):
        what = "premise (%s, frame %d)" % (mode, i)
        print(what, base.ctr[i], c)
        assert base.status[i] == 0 and base.ctr[i]["saddles"] == c["n_saddles"] and base.ctr[i]["clusters"] == c["n_clusters"] <= base.ctr[i]["seeds"], what
        check_saddles(base.records(i), ref, what)
    for which, exactly in (("saddles", SADDLE), ("clusters", SEED_OVERFLOW_BIT)):
        at_and_below(d, sub, base, which, csub, mode, exactly)
    d.close()


def test_clusters_of_caller_given_response_planes(oracle, mixed, unlimited):
    """agx_clusters_enqueue on agx_planes_enqueue's response planes of the same frames: max_clusters at its bound and one below
    (AGX_CLUSTERS_OVERFLOW, count 0, no row, for that frame alone); clusters_per_frame at the count and one below.  The planes are
    the chain's own response bit for bit (tests/test_gpu_planes.py), so the seed lists are those of the chain's unlimited run."""
    import torch
    host, dev, counts = mixed
    n = len(counts)
    d = make("path1")
    resp = torch.empty((n, L.H, L.W), dtype=torch.float32, device="cuda")
    d.planes_enqueue(dev, 1.5, response=resp)

    def clusters(cpf):
        d.clusters_enqueue(resp, clusters_per_frame=cpf)
        rows, pts, cnt, st = d.clusters_fetch()
        return rows, cnt, st

    OK, CAPACITY, BORDER, OVER = 0, 1, 2, 3
    cpf = max(c["n_clusters"] for c in counts) + 2
    rows0, cnt0, st0 = clusters(cpf)
    ctr0 = unlimited("path1").ctr
    print("clusters premise", cnt0, st0, [c["seeds"] for c in ctr0])
    good = [i for i in range(n) if st0[i] & 0xFF == OK]
    assert len(good) >= 4, "premise: frames whose outermost ring is clean: %s" % st0
    for i in good:
        _, dbg = oracle.refined_saddle_points(np.ascontiguousarray(host[i]), debug=True)
        assert cnt0[i] == counts[i]["n_clusters"], "premise: clusters of frame %d" % i
        r = rows0[i, : cnt0[i]]
        assert np.array_equal(r["first_index"], dbg["first_index"]) and np.array_equal(r["size"], dbg["sizes"])
        assert bits_equal(r["cx"], dbg["centers"][:, 0]) and bits_equal(r["cy"], dbg["centers"][:, 1])
        assert (rows0[i, cnt0[i]:].view(np.uint32) == 0xFFFFFFFF).all()
        assert ctr0[i]["seeds"] >= cnt0[i]
    b = [ctr0[i]["seeds"] if i in good else 0 for i in range(n)]
    f = L.unique_argmax(b, "seed list of the clusters batch")
    for limit, void in ((b[f], None), (b[f] - 1, f)):
        d.set_limits(max_clusters=limit)
        rows, cnt, st = clusters(cpf)
        for i in range(n):
            what = "max_clusters %d, frame %d: status %#x count %d" % (limit, i, st[i], cnt[i])
            if i == void:
                assert st[i] == OVER and cnt[i] == 0 and (rows[i].view(np.uint32) == 0xFFFFFFFF).all(), what
            else:
                assert st[i] == st0[i] and cnt[i] == cnt0[i] and rows[i].tobytes() == rows0[i].tobytes(), what
    d.set_limits(0, 0, 0)
    g = L.unique_argmax([cnt0[i] if i in good else 0 for i in range(n)], "cluster count")
    for per_frame, short in ((int(cnt0[g]), None), (int(cnt0[g]) - 1, g)):
        rows, cnt, st = clusters(per_frame)
        for i in good:
            what = "clusters_per_frame %d, frame %d: status %#x count %d" % (per_frame, i, st[i], cnt[i])
            if i == short:
                assert st[i] & 0xFF == CAPACITY and cnt[i] == cnt0[i] and (rows[i].view(np.uint32) == 0xFFFFFFFF).all(), what
            else:
                assert st[i] == st0[i] and cnt[i] == cnt0[i] and rows[i, : cnt[i]].tobytes() == rows0[i, : cnt[i]].tobytes(), what
    d.close()


# ---- guard bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["last", "middle"])
@pytest.mark.parametrize("path", [1, 2])
def test_guard_bytes_with_the_overflowing_frame_last_and_in_the_middle(mixed, path, place):
    """The B - 1 legs of the three limits on a handle with guard bytes around every workspace buffer.  The overflowing frame as
    the LAST frame: one element past its lists is past the buffers, in the guards.  As a middle frame the element would land in
    the next frame's list: there the neighbours' byte-identity (at_and_below) is the evidence, the guards only confirm."""
    host, dev, counts = mixed
    others = [0, 1, L.I_FLAT]
    for which, f, generic in (("saddles", L.I_NOISE, 0), ("clusters", L.I_NOISE, 0), ("candidates", L.I_BIG, 1)):
        order = others + [f] if place == "last" else others[:2] + [f] + others[2:]
        sub, csub = cuda(host[order]), [counts[i] for i in order]
        d = make("generic%d" % path if generic else "path%d" % path, guarded=True)
        base = Run(d, sub, max(c["n_saddles"] for c in csub) + 2)
        got, _, _, _ = at_and_below(d, sub, base, which, csub, "guarded, %s frame" % place)
        assert order[got] == f
        r = d.debug_fetch(0, "redzones")
        assert r["buffers"] >= 20 and r["damaged_bytes"] == 0, "%s, %s frame: %s" % (which, place, r)
        d.close()
