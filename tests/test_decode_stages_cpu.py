"""The decode in three stages -- decode_positions (reference src/detector.rs:42-72), bit_code (:74-122), best_tag (:142-169) --
as far as it can be checked without a device: the host forms agx_decode_positions_tail, agx_bit_code_tail and
agx_best_tag_tail against the oracle's orc_decode_positions, orc_bit_code and orc_best_tag, their composition against
agx_decode_quads_tail, the declarations, and the gfx950 code object's metadata of the three kernels.

The inputs are built once here; tests/test_gpu_decode_stages.py sends the same ones through the kernels.

Two rules are the project's and not the oracle's, and are tested as such: a quad corner and a sample coordinate that is not
finite is AGX_QUAD_OUTSIDE (the oracle's `as u32` takes NaN and -inf for 0).  The sample POINTS are compared with the oracle's
under the project's coordinate tolerance of 1e-3 px: the two affines are each a binary64 solve rounded once to binary32 and may
differ in the last bit of a coefficient; the measured difference goes to profiles/decode_stages.json."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import tag_cases as T
from tests.test_decode_quads_cpu import FAMILIES, TAG_DTYPE, as_u32, family, jittered_quads, orc
from tests.util import ROOT

HDR = os.path.join(ROOT, "include", "aprilgrid_amd.h")
PROFILE = os.path.join(ROOT, "profiles", "decode_stages.json")
DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS, NO_MATCH, SKIPPED = range(6)
AGX_ERR_ARG, AGX_ERR_FAMILY = -1, -6
ENTRY_POINTS = {
    "agx_decode_positions_enqueue": (["det", "d_quads", "point_stride_bytes", "n_frames", "quads_per_frame", "d_counts", "d_point_status", "img_w",
                                      "img_h", "border_bits", "edge_bits", "margin", "d_points", "d_status"], "src/detector.rs:42-72"),
    "agx_decode_positions_tail": (["quads", "n_quads", "img_w", "img_h", "border_bits", "edge_bits", "margin", "points", "status"],
                                  "src/detector.rs:42-72"),
    "agx_bit_code_enqueue": (["det", "d_frames", "n_frames", "width", "height", "row_stride_bytes", "frame_stride_bytes", "format", "d_points",
                              "points_per_slot", "quads_per_frame", "d_counts", "d_status_in", "valid_brightness_threshold", "max_invalid_bit",
                              "d_bits", "d_status"], "src/detector.rs:74-122"),
    "agx_bit_code_tail": (["luma8", "width", "height", "row_stride_bytes", "points", "points_per_slot", "n_slots", "status_in",
                           "valid_brightness_threshold", "max_invalid_bit", "bits", "status"], "src/detector.rs:74-122"),
    "agx_best_tag_enqueue": (["det", "d_bits", "n_slots", "quads_per_frame", "d_counts", "d_status_in", "thres", "d_codes", "n_codes", "edge_bits",
                              "d_quads", "point_stride_bytes", "d_ids", "d_rotations", "d_status", "d_tags"], "src/detector.rs:142-169"),
    "agx_best_tag_tail": (["bits", "n_slots", "status_in", "thres", "family", "codes", "n_codes", "edge_bits", "quads", "ids", "rotations",
                           "status", "tags"], "src/detector.rs:142-169"),
}
PW, PH = 64, 48  # the bit_code planes (and the GPU file's frames)


# ---- best_tag: inputs and the oracle ----------------------------------------------------------------------------------------
def rot(bits, edge, times=1):
    for _ in range(times):
        bits = int(orc().orc_rotate_bits(C.c_uint64(bits), edge))
    return bits


def flip(word, positions):
    for p in positions:
        word ^= 1 << int(p)
    return word


@functools.lru_cache(None)
def best_tag_sets():
    """-> list of (name, codes uint64 [n], edge_bits, thres, bits uint64 [m])"""
    rng = np.random.default_rng(2024)
    sets = []

    def probes(codes, edge, thres, picks):
        nb = edge * edge
        out = []
        for i in picks:
            c = int(codes[i])
            for r in range(4):  # bits that equal the code after 0, 3, 2, 1 rotations
                out.append(rot(c, edge, r))
            if thres >= 1:  # a code at distance exactly thres - 1 and thres, at rotation 0 and one rotation away
                for d in (thres - 1, thres):
                    if d <= nb:
                        pos = rng.choice(nb, size=d, replace=False)
                        out.append(flip(c, pos))
                        out.append(rot(flip(c, pos), edge, 3))
        out += [int(v) for v in rng.integers(0, 1 << nb, 8, dtype=np.uint64)]
        return np.array(out, np.uint64)

    for fam in FAMILIES:
        edge, _, hamming, codes = family(fam)
        n = len(codes)
        picks = sorted({0, 15 % n, 16 % n, 17 % n, n - 1, (n // 16) * 16 % n, n // 2})
        sets.append((fam, codes, edge, hamming, probes(codes, edge, hamming, picks)))
        sets.append((fam + " thres 0", codes, edge, 0, probes(codes, edge, 0, picks[:2])))
    for n in (1, 15, 16, 17, 640, 641, 4096):
        codes = rng.integers(0, 1 << 36, n, dtype=np.uint64)
        picks = sorted({0, n - 1, n // 2, min(n - 1, 639), min(n - 1, 640)})
        sets.append(("random %d" % n, codes, 6, 4, probes(codes, 6, 4, picks)))  # (thres 4: no chance match among 4096 random codes)
    for edge, n in ((1, 2), (7, 40), (8, 100)):
        nb = edge * edge
        codes = rng.integers(0, 1 << nb, n, dtype=np.uint64) if nb < 64 else rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        sets.append(("edge %d" % edge, codes, edge, min(nb, 9), probes(codes, edge, min(nb, 9), sorted({0, n - 1, n // 2}))))
    # two codes at the same smallest distance: the lower index wins (a ^ 1 and a ^ 2 are one bit from a ^ 3 at index 2 and from a at 4;
    # a itself is at 4 and 6)
    a = 0x5A5A5A5A5
    codes = np.array([0xFFFFFFFFF, 0x0, a ^ 0b11, 0x123456789, a, a ^ 0b11, a], np.uint64)
    sets.append(("ties", codes, 6, 11, np.array([a ^ 0b01, a, a ^ 0b10, rot(a ^ 0b01, 6, 2)], np.uint64)))
    # bits above edge^2: they count at rotation 0 only
    edge, _, hamming, codes = family("T16H5")
    c = int(codes[7])
    hi = [c | 1 << 40, c | 0xFFF << 20, rot(c, 4, 3) | 1 << 63, rot(c, 4, 2) | 0xFFFF << 16, c | 1 << 16]
    sets.append(("high bits", codes, edge, hamming, np.array(hi, np.uint64)))
    sets.append(("high bits, thres 3", codes, edge, 3, np.array(hi, np.uint64)))
    return sets


def oracle_best_tag(bits, thres, codes, edge):
    """-> (ids, rotations, status) of orc_best_tag, zero where it gives None"""
    lib = orc()
    ids, rots, st = np.zeros(len(bits), np.uint32), np.zeros(len(bits), np.uint32), np.zeros(len(bits), np.uint32)
    codes = np.ascontiguousarray(codes, np.uint64)
    for i, b in enumerate(bits):
        idx, r = C.c_int(0), C.c_int(0)
        if lib.orc_best_tag(C.c_uint64(int(b)), thres, codes.ctypes.data, len(codes), edge, C.byref(idx), C.byref(r)):
            ids[i], rots[i] = idx.value, r.value
        else:
            st[i] = NO_MATCH
    return ids, rots, st


# ---- bit_code: inputs, a model of the statuses, the oracle ------------------------------------------------------------------
def grid_points(n, x0=3.0, y0=2.0, step=1.0, cols=8):
    """n points on distinct pixels: (x0 + step * (i % cols), y0 + step * (i // cols))"""
    i = np.arange(n)
    return np.stack([x0 + step * (i % cols), y0 + step * (i // cols)], axis=1).astype(np.float32)


def painted(points, values, ground=7):
    """A PW x PH plane of `ground` with values[i] at the pixel points[i] rounds to."""
    plane = np.full((PH, PW), ground, np.uint8)
    ix, iy = as_u32(points[:, 0]).astype(int), as_u32(points[:, 1]).astype(int)
    plane[iy, ix] = values
    return plane


@functools.lru_cache(None)
def bit_code_cases():
    """-> list of (name, plane [PH, PW] u8, points [P, 2] f32, valid_brightness_threshold, max_invalid_bit, intended status or None)"""
    rng = np.random.default_rng(77)
    cases = []
    noise = rng.integers(0, 256, (PH, PW), dtype=np.uint8)
    for p in (1, 7, 8, 9, 36, 49, 64):
        for k in range(3):
            pts = np.stack([rng.uniform(-0.4, PW - 0.6, p), rng.uniform(-0.4, PH - 0.6, p)], axis=1).astype(np.float32)
            cases.append(("noise P=%d #%d" % (p, k), noise, pts, 10, 3 + 20 * k, None))
        pts = grid_points(p)
        vals = np.where(np.arange(p) % 3 == 0, 200, 20)
        if p == 1:
            cases.append(("one point", painted(pts, vals), pts, 10, 3, LOW_CONTRAST))
        else:
            cases.append(("two levels P=%d" % p, painted(pts, vals), pts, 10, 3, DECODED))
    pts = grid_points(36)
    two = np.where(np.arange(36) % 2 == 0, 0, 1)
    cases.append(("contrast 49", painted(pts, 60 + 49 * two), pts, 0, 3, LOW_CONTRAST))
    cases.append(("contrast 50", painted(pts, 60 + 50 * two), pts, 0, 3, DECODED))
    for max_inv in (3, 0):
        for extra in (0, 1):
            vals = np.where(np.arange(36) % 2 == 0, 0, 200)  # mid 100
            vals[:max_inv + extra] = 95  # |100 - 95| < 10
            cases.append(("invalid %d of max %d" % (max_inv + extra, max_inv), painted(pts, vals), pts, 10, max_inv, AMBIGUOUS if extra else DECODED))
    vals = np.where(np.arange(36) % 2 == 0, 0, 200)
    vals[5] = 100  # exactly the mid brightness
    cases.append(("threshold 0", painted(pts, vals), pts, 0, 0, DECODED))
    cases.append(("threshold 255", painted(pts, vals), pts, 255, 35, AMBIGUOUS))
    cases.append(("threshold 255, max 36", painted(pts, vals), pts, 255, 36, DECODED))
    vals = np.where(np.arange(36) % 2 == 0, 0, 201)  # mid = round(100.5) = 101
    vals[3], vals[4], vals[5], vals[6] = 100, 101, 102, 92
    cases.append(("odd min + max", painted(pts, vals), pts, 10, 36, DECODED))
    vals = np.where(np.arange(36) % 2 == 0, 0, 200)
    edge_in = pts.copy()
    edge_in[0], edge_in[1] = (PW - 1 + 0.4, 3.0), (5.0, PH - 1 + 0.4)
    cases.append(("samples at w-1 and h-1", painted(edge_in, vals), edge_in, 10, 3, DECODED))
    for name, xy in (("w", (PW - 0.5, 3.0)), ("h", (5.0, PH - 0.5)), ("far", (3.0e9, 5.0)), ("huge", (3.0e38, 5.0))):
        out = pts.copy()
        out[35] = xy
        cases.append(("sample at " + name, painted(pts, vals), out, 10, 3, OUTSIDE))
    neg = pts.copy()
    neg[0] = (-7.0, -0.6)  # saturates to pixel (0, 0): inside
    cases.append(("negative sample", painted(neg, vals), neg, 10, 3, DECODED))
    for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):  # the project's rule; the oracle is not asked
        bad = pts.copy()
        bad[17, 1] = v
        cases.append(("sample " + name, painted(pts, vals), bad, 10, 3, OUTSIDE))
    return cases


def model_bit_code(plane, pts, thr, max_inv):
    """bit_code's status in the reference's order, and its bits (the project's rule for coordinates that are not finite)"""
    h, w = plane.shape
    if not np.isfinite(pts).all():
        return OUTSIDE, 0
    ix, iy = as_u32(pts[:, 0]), as_u32(pts[:, 1])
    if ((ix >= w) | (iy >= h)).any():
        return OUTSIDE, 0
    v = plane[iy.astype(int), ix.astype(int)].astype(int)
    lo, hi = int(v.min()), int(v.max())
    if hi - lo < 50:
        return LOW_CONTRAST, 0
    mid = (lo + hi + 1) // 2  # round half away from zero of a non-negative half-integer
    if int((np.abs(mid - v) < thr).sum()) > max_inv:
        return AMBIGUOUS, 0
    bits = 0
    for b in v:
        bits = bits << 1 | int(b > mid)
    return DECODED, bits


def oracle_bit_code(plane, pts, thr, max_inv):
    plane = np.ascontiguousarray(plane, np.uint8)
    pts = np.ascontiguousarray(pts, np.float32)
    bits = C.c_uint64(0)
    hit = orc().orc_bit_code(plane.ctypes.data, plane.shape[1], plane.shape[0], pts.ctypes.data, len(pts), thr, max_inv, C.byref(bits))
    return bool(hit), bits.value if hit else 0


# ---- decode_positions: inputs and the oracle --------------------------------------------------------------------------------
SETTINGS = tuple(sorted({(family(f)[1], family(f)[0]) for f in FAMILIES})) + ((0, 1), (0, 8), (3, 7))  # (border_bits, edge_bits)
MARGINS = (0.0, 0.25, 0.5, 1.0, -0.25)


def degenerate(border, edge, margin):
    s = np.float32(np.float32(2 * border + edge) - np.float32(1.0)) + np.float32(margin)
    return bool(s == -np.float32(margin))


def random_quads(rng, n, w, h, lo=8.0, hi=400.0):
    """n convex-ish quads inside w x h: a square of side lo .. hi (capped by the frame), turned, jittered, kept inside."""
    side = rng.uniform(min(lo, 0.3 * min(w, h)), min(hi, 0.8 * min(w, h)), n)
    cx, cy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    base = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64) * 0.5
    c, s = np.cos(ang), np.sin(ang)
    x = cx[:, None] + side[:, None] * (base[None, :, 0] * c[:, None] - base[None, :, 1] * s[:, None]) + rng.uniform(-0.1, 0.1, (n, 4)) * side[:, None]
    y = cy[:, None] + side[:, None] * (base[None, :, 0] * s[:, None] + base[None, :, 1] * c[:, None]) + rng.uniform(-0.1, 0.1, (n, 4)) * side[:, None]
    q = np.stack([np.clip(x, 0, w - 1.0), np.clip(y, 0, h - 1.0)], axis=2)
    return q.reshape(n, 8).astype(np.float32)


@functools.lru_cache(None)
def decision_quads(w, h):
    """Quads for the Some / None decision at a w x h image: random ones around and across the frame's edges, and the named ones."""
    rng = np.random.default_rng(1000 * w + h)
    q = rng.uniform(-3.0, max(w, h) + 3.0, (60, 8)).astype(np.float32)
    inside = np.array([0.2, 0.2, w - 1.2, 0.3, w - 1.3, h - 1.2, 0.3, h - 1.3], np.float32)
    named = []
    for i, v in ((2, w - 1 - 0.49), (2, w - 1 + 0.49), (2, w - 0.5), (5, h - 1 + 0.49), (5, h - 0.5), (0, -0.6), (0, -1e30), (1, -4.0), (4, np.inf),
                 (6, 3.0e9), (6, 4294967296.0)):
        one = inside.copy()
        one[i] = v
        named.append(one)
    return np.concatenate([q, np.array(named, np.float32), inside[None]])


def oracle_positions(quads, w, h, border, edge, margin):
    """-> (points [n, edge^2, 2] (zero where None), status [n])"""
    lib = orc()
    quads = np.ascontiguousarray(quads, np.float32).reshape(-1, 8)
    pts = np.zeros((len(quads), edge * edge, 2), np.float32)
    st = np.zeros(len(quads), np.uint32)
    for i in range(len(quads)):
        if not lib.orc_decode_positions(w, h, quads[i].ctypes.data, border, edge, margin, pts[i].ctypes.data):
            st[i] = OUTSIDE
            pts[i] = 0
    return pts, st


# ---- the composition's inputs ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def composition_sets():
    """-> list of (name, family, plane [h, w] u8, quads [n, 8]): seeded random quads on a noise plane, jittered ground-truth quads
    on synthetic frames (these decode), and every painted case of tests/tag_cases.py"""
    rng = np.random.default_rng(5)
    sets = []
    noise = rng.integers(0, 256, (200, 320), dtype=np.uint8)
    quads = random_quads(rng, 2000, 320, 200, lo=8.0, hi=120.0)
    quads[::50] += rng.uniform(-40, 40, quads[::50].shape).astype(np.float32)  # (some leave the frame)
    for fam in ("T36H11", "T16H5", "T36H11B1"):
        sets.append(("noise " + fam, fam, noise, quads))
    frames, jq = jittered_quads(3, 400, 31)
    for f in range(3):
        sets.append(("synthetic frame %d" % f, "T36H11", frames[f], jq[f]))
    for fam in T.FAMILIES:
        for c in T.family_cases(fam):
            sets.append((fam + " " + c.name, fam, c.plane, c.quad[None]))
    return sets


def compose(fam, plane, quads, margin=0.5, thr=10, max_inv=3):
    """agx_decode_positions_tail -> agx_bit_code_tail -> agx_best_tag_tail with one status array handed on -> (tags, status, bits, points)"""
    import aprilgrid_rs_amd as A
    edge, border, hamming, _ = family(fam)
    h, w = plane.shape
    pts, st = A.decode_positions(quads, w, h, border, edge, margin)
    bits, st = A.bit_code(plane, pts, thr, max_inv, status_in=st)
    _, _, st, tags = A.best_tag(bits, hamming, tag_family=fam, status_in=st, quads=quads)
    return tags, st, bits, pts


# ---- declarations -------------------------------------------------------------------------------------------------------------
def test_header_library_ctypes_and_rust_declare_the_six_entry_points():
    from aprilgrid_rs_amd import _ffi
    import aprilgrid_rs_amd as A
    raw = open(HDR).read()
    h = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"^int (agx_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.M | re.S)}
    lib = _ffi.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    for name, (args, cite) in ENTRY_POINTS.items():
        assert name in protos, name
        assert [a.strip().split()[-1].lstrip("*") for a in protos[name].split(",")] == args, name
        at = raw.index("int " + name + "(")
        assert cite in raw[raw.rindex("/*", 0, at):at], name
        assert re.search(r"\bT %s\b" % name, nm), name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes == _ffi.SYMBOLS[name][1] and len(_ffi.SYMBOLS[name][1]) == len(args)
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, rust, flags=re.S)
        assert m and [a.split(":")[0].strip() for a in m.group(1).split(",") if a.strip()] == args, name
    assert re.search(r"#define AGX_ABI_VERSION 1\b", raw) and lib.agx_abi_version() == 1
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for sig in (r"pub fn decode_positions\(img_w: u32, img_h: u32, quad_pts: &\[\(f32, f32\)\], border_bits: u8, edge_bits: u8, margin: f32\) -> Option<Vec<\(f32, f32\)>>",
                r"pub fn bit_code\(img: &image::GrayImage, decode_pts: &\[\(f32, f32\)\], valid_brightness_threshold: u8, max_invalid_bit: u32\) -> Option<u64>",
                r"pub fn best_tag\(bits: u64, thres: u8, tag_family: &\[u64\], edge_bits: u8\) -> Option<\(usize, usize\)>"):
        assert re.search(sig, lib_rs), sig
    assert all(callable(getattr(A, n)) for n in ("decode_positions", "bit_code", "best_tag"))
    assert all(hasattr(A.TagDetector, n) for n in ("decode_positions_enqueue", "bit_code_enqueue", "best_tag_enqueue", "decode_quads_staged"))
    # NULL handles are argument errors, not crashes (no device is needed for that)
    assert lib.agx_decode_positions_enqueue(None, None, 8, 1, 1, None, None, 64, 48, 2, 6, 0.5, None, None) == AGX_ERR_ARG
    assert lib.agx_bit_code_enqueue(None, None, 1, 64, 48, 64, 64 * 48, 0, None, 36, 1, None, None, 10, 3, None, None) == AGX_ERR_ARG
    assert lib.agx_best_tag_enqueue(None, None, 1, 1, None, None, 11, None, 0, 6, None, 0, None, None, None, None) == AGX_ERR_ARG


def test_host_forms_refuse_bad_arguments():
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    lib = _ffi.lib()
    q = np.array([[10, 10, 40, 10, 40, 40, 10, 40]], np.float32)
    # the degenerate source square: side 1, margin 0 (S = 0 = -margin); and S == -margin at another size
    for border, edge, margin in ((0, 1, 0.0), (0, 2, -0.5), (0, 9, 0.5), (0, 0, 0.5), (17, 6, 0.5), (-1, 6, 0.5), (2, 6, np.nan), (2, 6, np.inf)):
        with pytest.raises(A.AgxError) as e:
            A.decode_positions(q, 64, 48, border, edge, margin)
        assert e.value.status == AGX_ERR_ARG, (border, edge, margin)
    assert degenerate(0, 1, 0.0) and degenerate(0, 2, -0.5) and not degenerate(0, 1, -0.25)
    pts, st = A.decode_positions(q, 64, 48, 0, 1, -0.25)  # the smallest square that is one
    assert st[0] == DECODED and np.isfinite(pts).all()
    plane = np.zeros((PH, PW), np.uint8)
    pts = grid_points(4)[None]
    for thr, p in ((-1, pts), (256, pts), (10, np.zeros((1, 65, 2), np.float32)), (10, np.zeros((1, 0, 2), np.float32))):
        with pytest.raises(A.AgxError) as e:
            A.bit_code(plane, p, thr, 3)
        assert e.value.status == AGX_ERR_ARG
    bits, st, out = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    assert lib.agx_bit_code_tail(plane.ctypes.data, PW, PH, PW - 1, pts.ctypes.data, 4, 1, None, 10, 3, bits.ctypes.data, st.ctypes.data) == AGX_ERR_ARG
    assert lib.agx_bit_code_tail(None, PW, PH, PW, pts.ctypes.data, 4, 1, None, 10, 3, bits.ctypes.data, st.ctypes.data) == AGX_ERR_ARG
    codes = np.arange(3, dtype=np.uint64)
    for thres, c, edge in ((-1, codes, 6), (256, codes, 6), (11, codes, 0), (11, codes, 9), (11, np.zeros(0, np.uint64), 6), (11, np.zeros(65536, np.uint64), 6)):
        with pytest.raises(A.AgxError) as e:
            A.best_tag(bits, thres, codes=c, edge_bits=edge)
        assert e.value.status == AGX_ERR_ARG, (thres, len(c), edge)
    assert len(A.best_tag(bits, 11, codes=np.zeros(65535, np.uint64), edge_bits=6)[0]) == 1
    ids = np.zeros(1, np.uint32)
    call = lambda fam, c, n, quads, tags: lib.agx_best_tag_tail(bits.ctypes.data, 1, None, 11, fam, c, n, 6, quads, ids.ctypes.data, out.ctypes.data,
                                                               st.ctypes.data, tags)
    assert call(99, None, 0, None, None) == AGX_ERR_FAMILY
    assert call(3, None, 5, None, None) == AGX_ERR_ARG  # n_codes without codes
    assert call(3, None, 0, q.ctypes.data, None) == AGX_ERR_ARG  # quads without tags
    assert call(3, None, 0, None, None) == 0


# ---- best_tag -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(best_tag_sets())), ids=[s[0] for s in best_tag_sets()])
def test_best_tag_equals_the_oracle(i):
    import aprilgrid_rs_amd as A
    name, codes, edge, thres, bits = best_tag_sets()[i]
    ids, rots, st = A.best_tag(bits, thres, codes=codes, edge_bits=edge)
    rid, rrot, rst = oracle_best_tag(bits, thres, codes, edge)
    assert np.array_equal(st, rst) and np.array_equal(ids, rid) and np.array_equal(rots, rrot), name
    if thres == 0:
        assert (st == NO_MATCH).all()
    elif name in FAMILIES or name.startswith("random") or name in ("edge 7", "edge 8"):
        assert (st == DECODED).any() and len(set(rots[st == DECODED])) == 4, name
    if name in FAMILIES:  # NULL codes = the family's list
        again = A.best_tag(bits, thres, tag_family=name)
        assert all(np.array_equal(a, b) for a, b in zip(again, (ids, rots, st)))


def test_best_tag_ties_high_bits_and_status_pass_through():
    import aprilgrid_rs_amd as A
    sets = {s[0]: s for s in best_tag_sets()}
    _, codes, edge, thres, bits = sets["ties"]
    ids, rots, st = A.best_tag(bits, thres, codes=codes, edge_bits=edge)
    assert list(st) == [DECODED] * 4 and list(ids) == [2, 4, 2, 2] and list(rots[:3]) == [0, 0, 0] and rots[3] != 0
    _, codes, edge, thres, bits = sets["high bits"]
    ids, rots, st = A.best_tag(bits, thres, codes=codes, edge_bits=edge)
    assert st[0] == NO_MATCH and st[1] == NO_MATCH  # rotation 0 counts the bits above edge^2, and the rotated words are not the code
    assert (st[2], ids[2], rots[2]) == (DECODED, 7, 1) and (st[3], ids[3], rots[3]) == (DECODED, 7, 2)  # they are dropped by the first rotation
    _, codes, edge, thres, bits = sets["high bits, thres 3"]
    ids, rots, st = A.best_tag(bits, thres, codes=codes, edge_bits=edge)
    assert (st[0], ids[0], rots[0]) == (DECODED, 7, 0) and st[1] == NO_MATCH
    # status_in: a non-zero word is passed through, ids / rotations / tags are zero
    quads = np.arange(40, dtype=np.float32).reshape(5, 8)
    s_in = np.array([0, SKIPPED, 0, OUTSIDE, 0xDEAD], np.uint32)
    ids, rots, st, tags = A.best_tag(bits, 3, codes=codes, edge_bits=edge, status_in=s_in, quads=quads)
    assert list(st) == [DECODED, SKIPPED, DECODED, OUTSIDE, 0xDEAD] and not ids[[1, 3, 4]].any() and not rots[[1, 3, 4]].any()
    assert not np.frombuffer(tags[[1, 3, 4]].tobytes(), np.uint8).any()
    assert tags[0]["id"] == 7 and np.array_equal(tags[0]["xy"], quads[0].reshape(4, 2)[::-1].reshape(8))  # rotation 0: reversed
    assert tags[2]["id"] == 7 and np.array_equal(tags[2]["xy"], np.roll(quads[2].reshape(4, 2), -1, axis=0)[::-1].reshape(8))


# ---- bit_code -------------------------------------------------------------------------------------------------------------------
def test_bit_code_equals_the_oracle_and_the_reference_order_of_statuses():
    import aprilgrid_rs_amd as A
    cases = bit_code_cases()
    seen = set()
    for name, plane, pts, thr, max_inv, intent in cases:
        bits, st = A.bit_code(plane, pts[None], thr, max_inv)
        want, wbits = model_bit_code(plane, pts, thr, max_inv)
        assert (int(st[0]), int(bits[0])) == (want, wbits), (name, int(st[0]), want, hex(int(bits[0])), hex(wbits))
        if np.isfinite(pts).all():
            hit, obits = oracle_bit_code(plane, pts, thr, max_inv)
            assert hit == (st[0] == DECODED) and obits == int(bits[0]), name
        assert intent is None or st[0] == intent, (name, int(st[0]), intent)
        seen.add(int(st[0]))
    assert seen == {DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS}
    assert sorted(set(len(c[2]) for c in cases)) == [1, 7, 8, 9, 36, 49, 64]


def test_bit_code_row_stride_slots_and_status_pass_through():
    import aprilgrid_rs_amd as A
    cases = [c for c in bit_code_cases() if len(c[2]) == 36 and c[3] == 10 and c[4] == 3]
    assert len(cases) >= 8
    for name, plane, pts, thr, max_inv, _ in cases[:4]:
        wide = np.full((PH, PW + 19), 255, np.uint8)
        wide[:, :PW] = plane
        a, b = A.bit_code(wide[:, :PW], pts[None], thr, max_inv), A.bit_code(plane, pts[None], thr, max_inv)  # row stride PW + 19
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
    # several slots on one plane, every second with a word to pass through
    plane = cases[0][1]
    pts = np.stack([c[2] for c in cases[:8]])
    alone = [A.bit_code(plane, p[None], 10, 3) for p in pts]
    s_in = np.array([0, SKIPPED, 0, OUTSIDE, 0, 0xDEAD, 0, NO_MATCH], np.uint32)
    bits, st = A.bit_code(plane, pts, 10, 3, status_in=s_in)
    for i in range(8):
        if s_in[i]:
            assert st[i] == s_in[i] and bits[i] == 0
        else:
            assert st[i] == alone[i][1][0] and bits[i] == alone[i][0][0]
    nan = pts.copy()
    nan[1, 0, 0] = np.nan  # a slot that is passed through reads nothing: its NaN does not turn it OUTSIDE
    bits2, st2 = A.bit_code(plane, nan, 10, 3, status_in=s_in)
    assert np.array_equal(st2, st) and np.array_equal(bits2, bits)


# ---- decode_positions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1280, 800), (64, 48), (9, 9), (8, 8), (8, 3), (1, 1), (3, 7)])
def test_decode_positions_decision_equals_the_oracle(size):
    import aprilgrid_rs_amd as A
    w, h = size
    quads = decision_quads(w, h)
    for border, edge in ((2, 6), (1, 6), (0, 1)):
        _, st = A.decode_positions(quads, w, h, border, edge, 0.5)
        _, rst = oracle_positions(quads, w, h, border, edge, 0.5)
        assert np.array_equal(st, rst), (size, border, edge, np.flatnonzero(st != rst))
        assert set(st) == {DECODED, OUTSIDE}
    # the project's rule, where the oracle's `as u32` takes the value for 0: NaN and -inf are OUTSIDE before anything else
    for v in (np.nan, -np.inf, np.inf):
        for i in range(8):
            q = quads[-1:].copy()
            assert A.decode_positions(q, w, h, 2, 6, 0.5)[1][0] == DECODED
            q[0, i] = v
            pts, st = A.decode_positions(q, w, h, 2, 6, 0.5)
            assert st[0] == OUTSIDE and not pts.any()


def test_decode_positions_points_within_the_coordinate_tolerance_of_the_oracle():
    """Largest |difference| of a sample coordinate between the closed-form affine and the oracle's Gauss-Jordan solve, per
    (border_bits, edge_bits) and margin, over 300 seeded quads inside 1280 x 800 each: in pixels, and in units of the f32 ulp of
    the quad's largest coordinate.  The tolerance is the project's for coordinates, 1e-3 px (README).  The order
    of the points (x outer, y inner) is held by the same comparison."""
    import aprilgrid_rs_amd as A
    w, h = 1280, 800
    rng = np.random.default_rng(42)
    quads = random_quads(rng, 300, w, h)
    ulp = np.spacing(np.abs(quads).max(axis=1).astype(np.float32)).astype(np.float64)
    report, worst = {}, 0.0
    for border, edge in SETTINGS:
        for margin in MARGINS:
            if degenerate(border, edge, margin):
                continue
            pts, st = A.decode_positions(quads, w, h, border, edge, margin)
            rpts, rst = oracle_positions(quads, w, h, border, edge, margin)
            assert np.array_equal(st, rst) and (st == DECODED).sum() >= 250
            d = np.abs(pts.astype(np.float64) - rpts.astype(np.float64)).reshape(len(quads), -1).max(axis=1)
            differ = float((d > 0).mean())
            report["border %d edge %d margin %g" % (border, edge, margin)] = {
                "max_abs_px": float(d.max()), "max_ulp_of_largest_coordinate": float((d / ulp).max()), "share_of_quads_that_differ": round(differ, 4)}
            worst = max(worst, float(d.max()))
    print(json.dumps(report, indent=1))
    assert len(report) == len(SETTINGS) * len(MARGINS) - 1  # (0, 1) at margin 0 is the degenerate square
    try:
        doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        doc["points_against_oracle"] = {"test": "tests/test_decode_stages_cpu.py", "quads": len(quads), "image": [w, h], "settings": report}
        with open(PROFILE, "w") as f:
            f.write(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    except OSError as e:  # a read-only checkout: the figures are above
        print("profiles/decode_stages.json not written:", e)
    assert worst <= 1e-3, worst


# ---- the composition ----------------------------------------------------------------------------------------------------------
def test_three_host_stages_compose_to_decode_quads_tail_byte_for_byte():
    import aprilgrid_rs_amd as A
    n, seen = 0, set()
    for name, fam, plane, quads in composition_sets():
        tags, st, bits, _ = compose(fam, plane, quads)
        rtags, rst, rbits = A.decode_quads_tail(fam, plane, quads, with_bits=True)
        assert st.tobytes() == rst.tobytes() and bits.tobytes() == rbits.tobytes() and tags.tobytes() == rtags.tobytes(), name
        n += len(quads)
        seen |= set(int(s) for s in st)
    assert n >= 2000 + sum(len(T.family_cases(f)) for f in T.FAMILIES) and seen == {DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS, NO_MATCH}


def test_open_arguments_change_the_answer_as_the_oracle_says():
    """Away from try_decode_quad's constants: another margin, looser brightness rules, a sub-family as the code list -- each stage
    against the oracle on the synthetic frames."""
    import aprilgrid_rs_amd as A
    frames, jq = jittered_quads(1, 200, 9)
    plane, quads = frames[0], jq[0]
    h, w = plane.shape
    edge, border, hamming, codes = family("T36H11")
    sub = np.ascontiguousarray(codes[::2])
    for margin, thr, max_inv, thres in ((0.5, 10, 3, hamming), (0.25, 25, 8, 5), (0.0, 0, 0, 1)):
        pts, st = A.decode_positions(quads, w, h, border, edge, margin)
        rpts, rst = oracle_positions(quads, w, h, border, edge, margin)
        assert np.array_equal(st, rst)
        bits, st2 = A.bit_code(plane, pts, thr, max_inv, status_in=st)
        for i in np.flatnonzero(st == DECODED):
            hit, obits = oracle_bit_code(plane, pts[i], thr, max_inv)
            assert hit == (st2[i] == DECODED) and obits == int(bits[i])
        ids, rots, st3 = A.best_tag(bits, thres, codes=sub, edge_bits=edge, status_in=st2)
        ok = np.flatnonzero(st2 == DECODED)
        rid, rrot, rst3 = oracle_best_tag(bits[ok], thres, sub, edge)
        assert np.array_equal(ids[ok], rid) and np.array_equal(rots[ok], rrot) and np.array_equal(st3[ok], rst3)
        assert np.array_equal(st3[st2 != DECODED], st2[st2 != DECODED])
    assert (st3 == DECODED).sum() >= 1


# ---- the code object --------------------------------------------------------------------------------------------------------
def test_compiled_stage_kernels_metadata():
    """The gfx950 code objects inside the built library (metadata notes only): k_decode_positions, k_bit_code and both forms of
    k_best_tag (the list in LDS, the list read in place) are there, with no private segment (no scratch), no spilled register, at
    most 128 VGPRs, workgroups of 256; LDS only in k_best_tag's staged form, 640 codes of 8 bytes."""
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so")
    notes = ""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused")],
                       check=True, capture_output=True)
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        assert len(starts) >= 3
        for i, at in enumerate(starts):
            one, co = os.path.join(tmp, "fat%d.bin" % i), os.path.join(tmp, "dev%d.co" % i)
            open(one, "wb").write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + one,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
            notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in ("k_decode_positions", "k_bit_code", "k_best_tag"):
            if k in name:
                kernels.setdefault(k, []).append({f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1))
                                                 for f in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count",
                                                           "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size")})
    assert {k: len(v) for k, v in kernels.items()} == {"k_decode_positions": 1, "k_bit_code": 1, "k_best_tag": 2}, kernels
    for name, forms in kernels.items():
        for k in forms:
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
            assert k["vgpr_count"] <= 128 and k["max_flat_workgroup_size"] == 256, (name, k)
    assert sorted(k["group_segment_fixed_size"] for k in kernels["k_best_tag"]) == [0, 640 * 8]
    assert kernels["k_decode_positions"][0]["group_segment_fixed_size"] == 0 and kernels["k_bit_code"][0]["group_segment_fixed_size"] == 0
