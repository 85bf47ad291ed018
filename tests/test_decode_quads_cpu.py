"""Decode of caller-given quads (agx_decode_quads_enqueue / _fetch, agx_decode_quads, agx_decode_quads_tail; reference
src/detector.rs:448-476) as far as it can be checked without a device: the declarations in header, library, ctypes table and
Rust binding; the host's agx_decode_quads_tail against a yardstick composed from the oracle's orc_decode_positions,
orc_bit_code, orc_best_tag and orc_rotate_bits; every AGX_QUAD_* reason reached by construction; the gfx950 code object's
metadata of k_decode_quads.

The yardstick and the library evaluate tag_affine differently (Gauss-Jordan against a diagonalised solve, both in binary64 and
rounded once): a coefficient can differ by one f32 ulp and a sample coordinate by about 4e-5 px at 320 px.  A quad is
KNIFE-EDGE when, under the oracle alone, a corner or sample coordinate lies within 2e-4 px of a half-integer: its rounding
could flip, and the pixel read with it.  Nothing else can differ: with every rounded coordinate equal the two read the same
pixels, and everything behind the samples is integer arithmetic.  (A sample can be swapped for its 4-neighbour -- and move
min, max or a .5 mid brightness with it -- only by such a flip, so that case is inside this set; taken on its own, "the mid
brightness is a .5 case and some neighbouring pixel would move min or max" holds for about half of all quads of a noisy
image and would exclude them for no reason.)  Knife-edge quads are left out of the library-versus-yardstick comparison and
nowhere else; at most 10 % of the quads of any one input set may be knife-edge (expected: 36 samples * 2 coordinates * 4e-4 =
3 %), asserted from the oracle alone for every seeded set."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.util import ALL_IMAGES, ROOT, load_image, synth_module

HDR = os.path.join(ROOT, "include", "aprilgrid_amd.h")
CITE = "src/detector.rs:448-476"
ENTRY_POINTS = {
    "agx_decode_quads_enqueue": ["det", "d_frames", "n_frames", "width", "height", "row_stride_bytes", "frame_stride_bytes", "format",
                                 "d_quads", "point_stride_bytes", "quads_per_frame", "d_counts", "d_point_status", "d_tags", "d_status",
                                 "d_bits"],
    "agx_decode_quads_fetch": ["det", "out", "status", "bits"],
    "agx_decode_quads": ["det", "pixels", "width", "height", "row_stride_bytes", "format", "quads", "n_quads", "out", "status", "bits",
                         "n_decoded"],
    "agx_decode_quads_tail": ["family", "luma8", "width", "height", "row_stride_bytes", "quads", "n_quads", "out", "status", "bits",
                              "n_decoded"],
}
DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS, NO_MATCH, SKIPPED = range(6)
CONSTANTS = {"AGX_QUAD_DECODED": 0, "AGX_QUAD_OUTSIDE": 1, "AGX_QUAD_LOW_CONTRAST": 2, "AGX_QUAD_AMBIGUOUS": 3, "AGX_QUAD_NO_MATCH": 4,
             "AGX_QUAD_SKIPPED": 5}
FAMILIES = ("T16H5", "T25H7", "T25H9", "T36H11", "T36H11B1")
KNIFE_PX = 2e-4
KNIFE_CAP = 0.10
TAG_DTYPE = np.dtype([("id", "u4"), ("xy", "f4", (8,))])


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def orc():
    """liborc.so's decode stages with this file's own prototypes (oracle/agx_oracle.c: orc_decode_positions, orc_bit_code,
    orc_best_tag, orc_rotate_bits)."""
    from oracle import oracle as O
    lib = C.CDLL(str(O.build()))
    lib.orc_decode_positions.restype = C.c_int
    lib.orc_decode_positions.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    lib.orc_bit_code.restype = C.c_int
    lib.orc_bit_code.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.orc_best_tag.restype = C.c_int
    lib.orc_best_tag.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.orc_rotate_bits.restype = C.c_uint64
    lib.orc_rotate_bits.argtypes = [C.c_uint64, C.c_int]
    return lib


@functools.lru_cache(None)
def family(name):
    from oracle import oracle as O
    edge, border, hamming, _ = O.FAMILIES[name]
    return edge, border, hamming, np.ascontiguousarray(O.family_codes(name), np.uint64)


def as_u32(v):
    """Rust's `f32::round() as u32` of float32 values: half away from zero, saturating, NaN -> 0 (in binary64: exact)."""
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    return np.where(r > 0, np.minimum(r, 4294967295.0), 0.0)  # (NaN > 0 is False)


def near_half(v):
    v = np.asarray(v, np.float64)
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= KNIFE_PX


def yardstick(luma, quad, fam):
    """try_decode_quad (src/detector.rs:448-476: margin 0.5, threshold 10, max-invalid 3, then rotate_left(rotation); reverse())
    of one quad on a CONTIGUOUS u8 plane -> (status, id, xy[8], bits, knife_edge).  Non-finite corners: OUTSIDE by the header's
    rule, and the oracle is not asked."""
    lib = orc()
    luma = np.ascontiguousarray(luma, np.uint8)
    h, w = luma.shape
    q = np.ascontiguousarray(quad, np.float32).reshape(8)
    zero = np.zeros(8, np.float32)
    if not np.isfinite(q).all():
        return OUTSIDE, 0, zero, 0, False
    edge, border, hamming, codes = family(fam)
    n = edge * edge
    knife = bool(near_half(q).any())
    pts = np.zeros(2 * n, np.float32)
    if not lib.orc_decode_positions(w, h, q.ctypes.data, border, edge, 0.5, pts.ctypes.data):
        return OUTSIDE, 0, zero, 0, knife
    knife = knife or bool(near_half(pts).any())
    ix, iy = as_u32(pts[0::2]), as_u32(pts[1::2])
    bits = C.c_uint64(0)
    have = lib.orc_bit_code(luma.ctypes.data, w, h, pts.ctypes.data, n, 10, 3, C.byref(bits))
    if ((ix >= w) | (iy >= h)).any():
        assert not have
        return OUTSIDE, 0, zero, 0, knife
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    v = luma[iy, ix].astype(np.int64)
    lo, hi = int(v.min()), int(v.max())
    if hi - lo < 50:
        assert not have
        return LOW_CONTRAST, 0, zero, 0, knife
    if not have:
        mid = int(as_u32(np.float32((np.float32(lo) + np.float32(hi)) / np.float32(2.0)))) & 0xFF
        assert int((np.abs(mid - v) < 10).sum()) > 3
        return AMBIGUOUS, 0, zero, 0, knife
    idx, rot = C.c_int(0), C.c_int(0)
    if not lib.orc_best_tag(bits.value, hamming, codes.ctypes.data, len(codes), edge, C.byref(idx), C.byref(rot)):
        return NO_MATCH, 0, zero, int(bits.value), knife
    c = q.reshape(4, 2)
    c = np.roll(c, -rot.value, axis=0)[::-1]  # rotate_left(rot); reverse()  (:467-470)
    return DECODED, idx.value, np.ascontiguousarray(c).reshape(8), int(bits.value), knife


def yardstick_many(luma, quads, fam):
    """-> (status [n], tags [n] TAG_DTYPE, bits [n] uint64, knife [n] bool)"""
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    st = np.zeros(len(quads), np.uint32)
    tags = np.zeros(len(quads), TAG_DTYPE)
    bits = np.zeros(len(quads), np.uint64)
    knife = np.zeros(len(quads), bool)
    for i, q in enumerate(quads):
        s, tid, xy, b, k = yardstick(luma, q, fam)
        st[i], bits[i], knife[i] = s, b, k
        if s == DECODED:
            tags[i]["id"], tags[i]["xy"] = tid, xy
    return st, tags, bits, knife


def check_against_yardstick(got, ref, what):
    """(tags, status, bits) of the library against yardstick_many's result, outside the knife-edge set; zero records and zero
    bits everywhere they are due, knife-edge or not."""
    tags, st, bits = got
    rst, rtags, rbits, knife = ref
    assert knife.mean() <= KNIFE_CAP, "%s: %d of %d quads knife-edge: change the input's seed" % (what, knife.sum(), len(knife))
    keep = ~knife
    assert np.array_equal(st[keep], rst[keep]), "%s: status differs at %s" % (what, np.flatnonzero(keep & (st != rst))[:8])
    assert np.array_equal(tags["id"][keep], rtags["id"][keep]), what + ": ids"
    assert np.array_equal(tags["xy"][keep].view(np.uint32), rtags["xy"][keep].view(np.uint32)), what + ": corner order"
    assert np.array_equal(bits[keep], rbits[keep]), what + ": bits"
    check_zero_records(tags, st, bits, what)


def check_zero_records(tags, st, bits, what):
    assert np.isin(st, list(range(6))).all(), what
    assert not np.frombuffer(tags[st != DECODED].tobytes(), np.uint8).any(), what + ": a slot that is not DECODED holds a non-zero agx_tag"
    assert not bits[~np.isin(st, (DECODED, NO_MATCH))].any(), what + ": bits of a slot that is neither DECODED nor NO_MATCH"


def orderings(corners):
    """A detected tag's 4x2 corners in the returned order, its three other cyclic rotations, and the same with reversed winding."""
    c = np.asarray(corners, np.float32).reshape(4, 2)
    return [np.roll(w, -r, axis=0).reshape(8) for w in (c, c[::-1]) for r in range(4)]


# ---- inputs, each computed once ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fixture_case(name):
    """-> (luma8, quads [n, 8], yardstick result): every tag the oracle's detect finds in the fixture image, in 8 orderings."""
    from oracle import oracle as O
    import aprilgrid_rs_amd as A
    img = load_image(name)
    luma = A.TagDetector.luma8(img)
    assert np.array_equal(luma, O.luma_u8(img))
    found = O.detect(img)
    quads = np.array([o for t in sorted(found) for o in orderings(found[t])], np.float32)
    return luma, quads, yardstick_many(luma, quads, "T36H11")


SYNTH_SPEC = {"T16H5": (5, 6), "T25H7": (6, 6), "T25H9": (5, 6), "T36H11": (6, 6), "T36H11B1": (6, 6)}  # (30 and 35 codes: 30 tags)


@functools.lru_cache(None)
def synth_case(fam, seed=21, w=800, h=600):
    """-> (luma8, quads [n, 8], yardstick result, ground-truth id of every quad)"""
    from oracle import oracle as O
    synth = synth_module()
    rows, cols = SYNTH_SPEC[fam]
    img, gt = synth.render_frame(seed, w, h, spec=synth.BoardSpec(rows=rows, cols=cols), family=fam)
    luma = img.numpy()
    found = O.detect(luma, family=fam)
    assert len(found) >= rows * cols // 2, (fam, len(found))
    quads, truth = [], []
    for t in sorted(found):
        centre = found[t].mean(axis=0)
        nearest = min(gt, key=lambda g: np.hypot(*(gt[g].mean(axis=0) - centre)))
        for o in orderings(found[t]):
            quads.append(o)
            truth.append(nearest)
    quads = np.array(quads, np.float32)
    return luma, quads, yardstick_many(luma, quads, fam), np.array(truth)


@functools.lru_cache(None)
def gt_case(fam="T36H11", first=0, n_frames=3, w=320, h=200):
    """The GPU file's frames: n_frames synthetic frames and, per frame, the ground-truth quads (TL, TR, BR, BL: the order that
    decodes with rotation 0) whose corners lie inside the frame.  -> (frames [n, h, w] u8, list of quads [n_f, 8], list of ids)"""
    synth = synth_module()
    rows, cols = SYNTH_SPEC[fam]
    frames, quads, ids = [], [], []
    for f in range(n_frames):
        img, gt = synth.render_frame(first + f, w, h, spec=synth.BoardSpec(rows=rows, cols=cols), family=fam)
        keep = [t for t in sorted(gt) if (gt[t][:, 0] > 2).all() and (gt[t][:, 0] < w - 3).all() and (gt[t][:, 1] > 2).all() and (gt[t][:, 1] < h - 3).all()]
        frames.append(img.numpy())
        quads.append(np.array([gt[t] for t in keep], np.float32).reshape(-1, 8))
        ids.append(np.array(keep))
    return np.stack(frames), quads, ids


GPU_SIZE = (320, 200)  # tests/test_gpu_decode_quads.py's frames (test_oracle_decodes_half_of_the_ground_truth_quads_at_the_gpu_size)


def jittered_quads(n_frames, qpf, seed, fam="T36H11"):
    """[n_frames, qpf, 8]: the frames' ground-truth quads, cycled, every third exact, the others with up to 0.6 px of jitter per
    coordinate; one quad in 40 far off (most of those leave the image or decode to nothing)."""
    frames, quads, _ = gt_case(fam, 0, 3, *GPU_SIZE)
    rng = np.random.default_rng(seed)
    out = np.zeros((n_frames, qpf, 8), np.float32)
    for f in range(n_frames):
        base = quads[f % 3][np.arange(qpf) % len(quads[f % 3])]
        j = rng.uniform(-0.6, 0.6, base.shape).astype(np.float32)
        j[::3] = 0
        far = rng.uniform(-60, 60, base.shape).astype(np.float32)
        out[f] = base + np.where((np.arange(qpf) % 40 == 39)[:, None], far, j)
    return frames[np.arange(n_frames) % 3], out


def constructed_cases():
    """Each AGX_QUAD_* reason by construction, on a 320 x 200 plane: a synthetic frame (its first ground-truth tag is the valid
    quad), with a flat patch and a smooth gradient painted where the board is not.
    -> (luma8, {name: (quad, intended status, family)})"""
    frames, quads, _ = gt_case("T36H11", 0, 1, 320, 200)
    luma = frames[0].copy()
    w, h = 320, 200
    luma[0:40, 0:40] = 128                                                                    # flat
    luma[160:200, 0:64] = (np.arange(64, dtype=np.float32) * 4.0)[None, :].astype(np.uint8)  # 0 .. 252 over 64 columns
    valid = quads[0][len(quads[0]) // 2].copy()
    assert not (valid.reshape(4, 2)[:, 0] < 70).all()
    rng = np.random.default_rng(7)
    side = float(np.hypot(*(valid[2:4] - valid[0:2])))
    jitter = (valid + rng.uniform(-1.0, 1.0, 8).astype(np.float32) * np.float32(side * 0.4)).astype(np.float32)
    sq = lambda x0, y0, s: np.array([x0, y0, x0 + s, y0, x0 + s, y0 + s, x0, y0 + s], np.float32)
    nan_q, inf_q = valid.copy(), valid.copy()
    nan_q[3] = np.nan
    inf_q[4] = -np.inf
    cases = {
        "valid": (valid, DECODED),
        "corner_at_width": (np.array([300, 90, float(w), 90, float(w), 110, 300, 110], np.float32), OUTSIDE),
        # corners inside, outer samples not.  A sample is a weighted mean of the four corners; with a border of two cells every
        # weight is >= 0 and no sample leaves the corners' hull, so this case exists only for T36H11B1 (border 1: the outermost
        # sample has the weights -1/16, 1/4, 9/16, 1/4): three corners on the right edge put it at x = 338
        "samples_outside": (np.array([1.3, 100.2, 318.8, 60.3, 318.7, 100.1, 318.9, 140.2], np.float32), OUTSIDE, "T36H11B1"),
        "negative_corner": (np.array([-3.0, -3.0, 37.47, 0.2, 37.27, 37.57, 0.3, 37.37], np.float32), LOW_CONTRAST),  # inside by saturation; flat
        "nan": (nan_q, OUTSIDE),
        "inf": (inf_q, OUTSIDE),
        "flat": (sq(4, 4, 31), LOW_CONTRAST),
        "gradient": (sq(2, 162, 36), AMBIGUOUS),
        "jittered": (jitter, NO_MATCH),
    }
    return luma, {n: (c[0], c[1], c[2] if len(c) > 2 else "T36H11") for n, c in cases.items()}


# ---- declarations -----------------------------------------------------------------------------------------------------------
def header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_constants():
    h = header()
    protos = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"^int (agx_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.M | re.S)}
    for name, args in ENTRY_POINTS.items():
        assert name in protos, name
        assert [a.strip().split()[-1].lstrip("*") for a in protos[name].split(",")] == args, name
    in_header = {n: int(v) for body in re.findall(r"enum\s*\w*\s*\{(.*?)\}", h, flags=re.S) for n, v in re.findall(r"\b(AGX_\w+)\s*=\s*(-?\d+)", body)}
    for name, value in CONSTANTS.items():
        assert in_header.get(name) == value, name
    raw = open(HDR).read()
    for name in ENTRY_POINTS:
        at = raw.index("int " + name + "(")
        assert CITE in raw[raw.rindex("/*", 0, at):at], name
    at = raw.index("enum { AGX_QUAD_DECODED")
    assert CITE in raw[raw.rindex("/*", 0, at):at] or CITE in raw[at:raw.index("};", at)]
    assert re.search(r"#define AGX_ABI_VERSION 1\b", raw)


def test_library_exports_and_bindings_bind_them():
    from aprilgrid_rs_amd import _ffi
    import aprilgrid_rs_amd as A
    lib = _ffi.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    for name, args in ENTRY_POINTS.items():
        assert re.search(r"\bT %s\b" % name, nm), name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes == _ffi.SYMBOLS[name][1] and len(_ffi.SYMBOLS[name][1]) == len(args)
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, rust, flags=re.S)
        assert m and [a.split(":")[0].strip() for a in m.group(1).split(",") if a.strip()] == args, name
    for name, value in CONSTANTS.items():
        assert getattr(_ffi, name) == value, name
        assert re.search(r"pub const %s: c_int = %d;" % (name, value), rust), name
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"pub fn decode_quads\(&self, img: &image::DynamicImage, quads: &\[\[\(f32, f32\); 4\]\]\)\s*->\s*Vec<Option<\(u32, \[\(f32, f32\); 4\]\)>>", lib_rs)
    assert callable(A.decode_quads_tail) and all(hasattr(A.TagDetector, n) for n in ("decode_quads", "decode_quads_enqueue", "decode_quads_fetch"))
    # NULL handles and NULL arrays are argument errors, not crashes (no device is needed for that)
    assert lib.agx_decode_quads_fetch(None, None, None, None) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads_enqueue(None, None, 1, 16, 16, 16, 256, 0, None, 8, 1, None, None, None, None, None) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads(None, None, 16, 16, 16, 0, None, 0, None, None, None, None) == _ffi.AGX_ERR_ARG
    luma = np.zeros((16, 16), np.uint8)
    n = C.c_uint32(7)
    q = np.zeros(8, np.float32)
    tag, st = np.zeros(1, TAG_DTYPE), np.zeros(1, np.uint32)
    assert lib.agx_decode_quads_tail(3, None, 16, 16, 16, q.ctypes.data, 1, tag.ctypes.data, st.ctypes.data, None, C.byref(n)) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads_tail(3, luma.ctypes.data, 16, 16, 16, None, 1, tag.ctypes.data, st.ctypes.data, None, C.byref(n)) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads_tail(3, luma.ctypes.data, 16, 16, 16, q.ctypes.data, 1, None, st.ctypes.data, None, C.byref(n)) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads_tail(3, luma.ctypes.data, 16, 16, 16, q.ctypes.data, 1, tag.ctypes.data, None, None, C.byref(n)) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads_tail(3, luma.ctypes.data, 16, 16, 16, q.ctypes.data, 1, tag.ctypes.data, st.ctypes.data, None, None) == _ffi.AGX_ERR_ARG
    assert lib.agx_decode_quads_tail(99, luma.ctypes.data, 16, 16, 16, q.ctypes.data, 1, tag.ctypes.data, st.ctypes.data, None, C.byref(n)) == _ffi.AGX_ERR_FAMILY


# ---- agx_decode_quads_tail against the yardstick -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_IMAGES)
def test_tail_equals_the_yardstick_on_the_fixture_images(name):
    import aprilgrid_rs_amd as A
    luma, quads, ref = fixture_case(name)
    got = A.decode_quads_tail("t36h11", luma, quads, with_bits=True)
    check_against_yardstick(got, ref, name)
    st = got[1]
    assert (st == DECODED).sum() >= len(quads) // 8, name  # (a detected tag decodes again in at least one of its orderings)
    assert len(quads) >= 8 * 30


@pytest.mark.parametrize("fam", [f for f in FAMILIES if f != "T36H11"])
def test_tail_equals_the_yardstick_and_the_ground_truth_on_every_family(fam):
    import aprilgrid_rs_amd as A
    luma, quads, ref, truth = synth_case(fam)
    tags, st, bits = A.decode_quads_tail(fam, luma, quads, with_bits=True)
    check_against_yardstick((tags, st, bits), ref, fam)
    dec = st == DECODED
    assert dec.sum() >= len(quads) // 8, fam
    assert np.array_equal(tags["id"][dec], truth[dec]), fam  # a decoded id is the id of the tag the quad was drawn from


def test_knife_edge_share_of_every_seeded_input_set_is_within_the_cap():
    """From the oracle alone: no library call."""
    shares = {}
    for name in ALL_IMAGES:
        shares[name] = fixture_case(name)[2][3].mean()
    for fam in FAMILIES:
        if fam != "T36H11":
            shares[fam] = synth_case(fam)[2][3].mean()
        frames, quads, _ = gt_case(fam, 0, 3, *GPU_SIZE)
        shares[fam + " gpu frames"] = np.concatenate([yardstick_many(frames[f], quads[f], fam)[3] for f in range(len(frames))]).mean()
    frames, quads = jittered_quads(3, 64, 11)  # tests/test_gpu_decode_quads.py's base set
    shares["gpu base set"] = np.concatenate([yardstick_many(frames[f], quads[f], "T36H11")[3] for f in range(3)]).mean()
    print(shares)
    assert max(shares.values()) <= KNIFE_CAP, shares


def test_oracle_decodes_half_of_the_ground_truth_quads_at_the_gpu_size():
    """The GPU file's frame size, 320 x 200 (a code cell is little more than a pixel wide there): the oracle decodes at least half
    of the ground-truth quads of every family, and what it decodes is the tag that was drawn."""
    for fam in FAMILIES:
        frames, quads, ids = gt_case(fam, 0, 3, *GPU_SIZE)
        n = sum(len(q) for q in quads)
        dec = 0
        for f in range(len(frames)):
            st, tags, _, _ = yardstick_many(frames[f], quads[f], fam)
            dec += int((st == DECODED).sum())
            assert np.array_equal(tags["id"][st == DECODED], ids[f][st == DECODED]), fam
        assert n >= 60 and 2 * dec >= n, (fam, dec, n)


# ---- each reason, by construction ------------------------------------------------------------------------------------------------
def test_constructed_inputs_land_where_intended_under_the_oracle_alone():
    luma, cases = constructed_cases()
    h, w = luma.shape
    for name, (quad, want, fam) in cases.items():
        st, _, _, bits, knife = yardstick(luma, quad, fam)
        assert st == want and not knife, (name, st, want, knife)
    # the OUTSIDE cases for the reason their names give
    q = cases["corner_at_width"][0]
    assert (as_u32(q[0::2]) >= w).any()
    q = cases["samples_outside"][0]
    assert (as_u32(q[0::2]) < w).all() and (as_u32(q[1::2]) < h).all()
    q = cases["negative_corner"][0]
    assert (q < 0).any() and (as_u32(q[0::2]) < w).all() and (as_u32(q[1::2]) < h).all()
    assert set(c[1] for c in cases.values()) == {DECODED, OUTSIDE, LOW_CONTRAST, AMBIGUOUS, NO_MATCH}


def test_tail_reaches_each_reason():
    import aprilgrid_rs_amd as A
    luma, cases = constructed_cases()
    for fam in sorted(set(c[2] for c in cases.values())):
        names = sorted(n for n in cases if cases[n][2] == fam)
        quads = np.array([cases[n][0] for n in names], np.float32)
        tags, st, bits = A.decode_quads_tail(fam, luma, quads, with_bits=True)
        assert [int(s) for s in st] == [cases[n][1] for n in names], dict(zip(names, st))
        ref = yardstick_many(luma, quads, fam)
        check_against_yardstick((tags, st, bits), ref, "constructed")
        if "jittered" in names:
            assert bits[names.index("jittered")] == ref[2][names.index("jittered")] != 0
        # without the bits
        tags2, st2 = A.decode_quads_tail(fam, luma, quads)
        assert tags2.tobytes() == tags.tobytes() and np.array_equal(st2, st)


def test_row_stride_larger_than_the_width_and_no_quads():
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    luma, quads, ref = fixture_case("EuRoC.png")
    h, w = luma.shape
    wide = np.full((h, w + 37), 255, np.uint8)
    wide[:, :w] = luma
    got = A.decode_quads_tail("t36h11", wide[:, :w], quads, with_bits=True)  # a strided view: row stride w + 37
    tight = A.decode_quads_tail("t36h11", luma, quads, with_bits=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, tight))
    # n_quads == 0
    tags, st = A.decode_quads_tail("t36h11", luma, np.zeros((0, 8), np.float32))
    assert len(tags) == 0 and len(st) == 0
    n = C.c_uint32(5)
    assert _ffi.lib().agx_decode_quads_tail(3, luma.ctypes.data, w, h, w, None, 0, None, None, None, C.byref(n)) == _ffi.AGX_OK and n.value == 0


def test_detect_is_unchanged_by_the_reasons():
    """decode_quad now reports why: what detect returns from it is the oracle's, as before."""
    import aprilgrid_rs_amd as A
    from oracle import oracle as O
    img = load_image("two_boards.png")
    s = O.refined_saddle_points(img)
    got = A.TagDetector.detect_tail("t36h11", s, A.TagDetector.luma8(img))
    ref = O.detect(img)
    assert sorted(got) == sorted(ref) and all(np.array_equal(got[t], ref[t]) for t in ref)


# ---- the code object --------------------------------------------------------------------------------------------------------
def test_compiled_decode_kernel_metadata():
    """The gfx950 code object inside the built library (metadata notes only): k_decode_quads is there, with no private segment
    (no scratch), no spilled register, the code list as its only LDS (640 entries of 8 bytes: the table k_board_tail keeps,
    587 used by the largest family) and the workgroup of 256 its comment states; at most 128 VGPRs (four waves per SIMD)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so")
    notes = ""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused")],
                       check=True, capture_output=True)
        # one bundle per .hip file of the library, back to back in the section
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        assert len(starts) >= 2
        for i, at in enumerate(starts):
            one, co = os.path.join(tmp, "fat%d.bin" % i), os.path.join(tmp, "dev%d.co" % i)
            open(one, "wb").write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + one,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
            notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_decode_quads" in name:
            kernels[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                             for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "vgpr_spill_count",
                                       "sgpr_spill_count", "max_flat_workgroup_size")}
    assert len(kernels) == 1, sorted(kernels)
    (name, k), = kernels.items()
    assert "k_refine_points" not in name and "k_front_luma" not in name  # (existing tests count kernels by those names)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == 640 * 8, k
    assert max(len(family(f)[3]) for f in FAMILIES) == 587 <= 640
    assert k["vgpr_count"] <= 128, k
    assert k["max_flat_workgroup_size"] == 256, k
    src = open(os.path.join(ROOT, "aprilgrid-rs_amd", "csrc", "tail_kernels.hip")).read()
    assert "constexpr int DQ_THREADS = 256;" in src and "workgroup of 256 threads" in src
