"""The status every entry point that takes frames returns for a table of argument cases, cell for cell.

Entry points: the nine device entry points (agx_saddles_batch_enqueue / _to, agx_detect_batch_enqueue / _to,
agx_refine_points_enqueue, agx_decode_quads_enqueue, agx_planes_enqueue, the group's detect enqueue on one rank) and the
host-image ones that stage a frame (agx_refined_saddle_points, agx_detect, agx_rochade_refine, agx_decode_quads,
agx_gaussian_blur_f32, agx_hessian_response).  Cases: null frames, frame counts, every format value, sides 0 / 1 / 2, the
size limits, strides one byte short and at the 2^31 bound, every alignment rule, the front-end row limit, and two-fault cases
that pin which refusal comes first.  Frames are zeros; an accepted case has a tiny geometry, so acceptance costs nothing.

A cell is null where the case does not exist for the entry point (a host image has no frame count, no frame stride and no
bound on its row stride), and for one accepted case whose acceptance needs gigabytes: a frame of 2^30 - W pixels is a
workspace of several GiB on the chain's entry points and a 4 GiB plane on agx_planes_enqueue.  It runs, as one frame 8 wide,
on agx_refine_points_enqueue (no 9 x 9 window: the frame is never read) and on agx_decode_quads_enqueue (which reads the
quads' corners only); tests/test_gpu_large_offsets.py covers what the kernels do with large extents.  Its refused neighbour,
2^30 pixels, runs everywhere, and so do 65535 frames (2 x 2 each) and a second row 0x7fffffff bytes behind the first.

The expected matrix (tests/golden/entry_arg_matrix.json) was recorded once from the build before the entry points shared one
frame-batch check (`python -m tests.test_gpu_entry_arg_matrix FILE` writes it) and is never regenerated from a later build."""
import json
import os
import sys

import pytest

from tests import entry_harness as E
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "entry_arg_matrix.json")
DEVICE_ENTRIES = ("agx_saddles_batch_enqueue", "agx_saddles_batch_enqueue_to", "agx_detect_batch_enqueue", "agx_detect_batch_enqueue_to",
                  "agx_refine_points_enqueue", "agx_decode_quads_enqueue", "agx_planes_enqueue", "agx_group_detect_enqueue")
HOST_ENTRIES = ("agx_refined_saddle_points", "agx_detect", "agx_rochade_refine", "agx_decode_quads", "agx_gaussian_blur_f32",
                "agx_hessian_response")
ENQUEUE_OF = {"agx_saddles_batch_enqueue": ("saddles", False), "agx_saddles_batch_enqueue_to": ("saddles", True),
              "agx_detect_batch_enqueue": ("detect", False), "agx_detect_batch_enqueue_to": ("detect", True),
              "agx_refine_points_enqueue": ("refine", False), "agx_decode_quads_enqueue": ("decode", False),
              "agx_planes_enqueue": ("planes", False), "agx_group_detect_enqueue": ("group", False)}
NO_FRAME_READ = ("agx_refine_points_enqueue", "agx_decode_quads_enqueue")  # where 2^30 - W pixels cost nothing (docstring)
PX = {0: 1, 1: 2, 2: 3, 3: 4, 4: 2, 5: 4, 6: 3, 7: 4, 8: 1, 9: 4, 10: 6, 11: 8}
W, H = 16, 12


def case(fmt=E.L8, n=2, w=W, h=H, ptr=0, null=False, rs=None, fs=None, drs=0, dfs=0, host=True, only=None):
    """One row of the table: frames of `fmt` at pool + ptr (null: NULL), tight strides + drs / dfs unless given."""
    px = PX.get(fmt, 1)
    rs = max(w, 0) * px + drs if rs is None else rs
    fs = rs * max(h, 0) * (3 if fmt == 8 else 1) + dfs if fs is None else fs
    return {"fmt": fmt, "n": n, "w": w, "h": h, "ptr": None if null else ptr, "rs": rs, "fs": fs, "host": host, "only": only}


def cases():
    c = {"null frames": case(null=True), "tiny and valid": case()}
    for n in (0, -1, 65536):
        c["n_frames %d" % n] = case(n=n, w=2, h=2, host=False)
    c["n_frames 65535"] = case(n=65535, w=2, h=2, host=False)
    for fmt in range(-1, 13):
        c["format %d" % fmt] = case(fmt=fmt, rs=W * 8, fs=W * 8 * H * 3)
    for v in (0, 1, 2):
        c["width %d" % v] = case(w=v, rs=16)
        c["height %d" % v] = case(h=v, fs=16 * 16)
    c["width 65001"] = case(w=65001, h=2, n=1)
    c["2^30 pixels"] = case(w=32768, h=32768, n=1, host=False)
    c["2^30 - W pixels"] = case(w=8, h=(1 << 27) - 1, n=1, host=False, only=NO_FRAME_READ)
    c["row stride one byte short"] = case(drs=-1, fs=W * H)
    c["row stride exact"] = case()
    c["row stride 0x7fffffff"] = case(w=8, h=2, n=1, rs=0x7fffffff, fs=1 << 32, host=False)
    c["row stride 0x80000000"] = case(w=8, h=2, n=1, rs=0x80000000, fs=1 << 33, host=False)
    for n in (1, 2):
        c["frame stride one byte short, %d frame(s)" % n] = case(n=n, dfs=-1, host=False)
        for what, kw in (("pointer", {"ptr": 1}), ("row stride", {"drs": 1}), ("frame stride", {"dfs": 1})):
            c["L16, odd %s, %d frame(s)" % (what, n)] = case(fmt=E.L16, n=n, host=what != "frame stride", **kw)
    for r in (1, 2):
        c["LF32, pointer = %d mod 4" % r] = case(fmt=E.LF32, ptr=r)
        c["LF32, row stride = %d mod 4" % r] = case(fmt=E.LF32, drs=r)
        c["LF32, frame stride = %d mod 4, 2 frames" % r] = case(fmt=E.LF32, dfs=r, host=False)
        c["LF32, frame stride = %d mod 4, 1 frame" % r] = case(fmt=E.LF32, n=1, dfs=r, host=False)
    c["LA8, 16 * 65535 + 1 rows"] = case(fmt=E.LA8, w=2, h=16 * 65535 + 1, n=1)
    # two faults at once: which refusal comes first
    c["bad format + width 0"] = case(fmt=-1, w=0, rs=16)
    c["null frames + bad format"] = case(fmt=12, null=True)
    c["null frames + LF32"] = case(fmt=E.LF32, null=True)
    c["null frames + n_frames 0"] = case(null=True, n=0, host=False)
    c["n_frames 0 + bad format"] = case(fmt=-1, n=0, host=False)
    c["n_frames 65536 + bad format"] = case(fmt=99, n=65536, w=2, h=2, host=False)
    c["LF32 + width 1"] = case(fmt=E.LF32, w=1)
    c["LF32 + odd pointer + n_frames 0"] = case(fmt=E.LF32, ptr=1, n=0, host=False)
    c["bad format + row stride 0"] = case(fmt=-1, rs=0, fs=0)
    c["L16 odd pointer + width 0"] = case(fmt=E.L16, ptr=1, w=0, rs=32)
    c["bad format + width 65001"] = case(fmt=12, w=65001, h=2, n=1)
    c["LF32 + 2^30 pixels"] = case(fmt=E.LF32, w=32768, h=32768, n=1, host=False)
    c["LA8 too tall + row stride short"] = case(fmt=E.LA8, w=2, h=16 * 65535 + 1, n=1, drs=-1, fs=1 << 23)
    c["LF32 + row stride 0x80000000"] = case(fmt=E.LF32, w=8, h=2, n=1, rs=0x80000000, fs=1 << 33, host=False)
    return c


def cell(hx, entry, k):
    """The status of `entry` for case k, or None where the case is not run on it."""
    if k["only"] is not None and entry not in k["only"]:
        return None
    if entry in HOST_ENTRIES:
        if not k["host"]:
            return None
        p = 0 if k["ptr"] is None else hx.host.ctypes.data + E.LEAD + k["ptr"]
        return hx.host_call(entry, (p, k["w"], k["h"], k["rs"], k["fmt"]))
    kind, to = ENQUEUE_OF[entry]
    p = 0 if k["ptr"] is None else hx.frames + k["ptr"]
    st = hx.enqueue(kind, (p, k["n"], k["w"], k["h"], k["rs"], k["fs"], k["fmt"]), to=to)
    if kind == "group" and st == E.OK:
        hx.group_fetch()  # (nothing of it stays in flight)
    return st


def matrix(hx):
    out = {}
    for name, k in cases().items():  # case-major: a workspace geometry serves every entry point before it changes
        out[name] = {e: cell(hx, e, k) for e in DEVICE_ENTRIES + HOST_ENTRIES}
        hx.det.sync()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_golden_file_is_complete(golden):
    table = cases()
    assert sorted(golden) == sorted(table)
    for name, k in table.items():
        assert sorted(golden[name]) == sorted(DEVICE_ENTRIES + HOST_ENTRIES), name
        for e, st in golden[name].items():
            run_here = (k["only"] is None or e in k["only"]) and (k["host"] or e not in HOST_ENTRIES)
            assert (st is not None) == run_here, (name, e)


def test_status_matrix(golden):
    hx = E.Harness()
    try:
        got = matrix(hx)
    finally:
        hx.close()
    wrong = {(c, e): (got[c][e], golden[c][e]) for c in got for e in got[c] if got[c][e] != golden[c][e]}
    for c in got:
        print(c, [got[c][e] for e in DEVICE_ENTRIES + HOST_ENTRIES])
    assert not wrong, wrong


if __name__ == "__main__":  # the recorder: python -m tests.test_gpu_entry_arg_matrix OUT.json
    x = E.Harness()
    rec = matrix(x)
    x.close()
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
    print("recorded %d cases x %d entry points" % (len(rec), len(DEVICE_ENTRIES + HOST_ENTRIES)))
