"""agx_decimate_tail (csrc/decimate.hip + csrc/decimate_math.h) without a GPU: against a numpy integer restatement byte for byte,
guard bytes included; every refused argument; and the point mapping agx_refine_windows_enqueue's `factor` relies on."""
import numpy as np
import pytest

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

SIZES = ((2, 2), (3, 2), (5, 3), (8, 8), (9, 7), (67, 45), (130, 4))  # (W, H)
FACTORS = (2, 3, 4)
GUARD = 0xA5


def numpy_decimate(a, f):
    """(sum of the f x f block + f f // 2) // (f f) in uint32; trailing columns and rows dropped.  a: [N, H, W]."""
    n, h, w = a.shape
    oh, ow = h // f, w // f
    blocks = a[:, :oh * f, :ow * f].astype(np.uint32).reshape(n, oh, f, ow, f)
    return ((blocks.sum(axis=(2, 4), dtype=np.uint32) + np.uint32(f * f // 2)) // np.uint32(f * f)).astype(a.dtype)


def padded(n, h, w, dtype, row_pad, frame_pad, seed):
    """-> (buffer, view [n, h, w] into it with row_pad pixels behind every row and frame_pad rows behind every frame)"""
    buf = np.full((n, h + frame_pad, w + row_pad), GUARD * (0x0101 if dtype == np.uint16 else 1), dtype)
    view = buf[:, :h, :w]
    rng = np.random.default_rng(seed)
    view[...] = rng.integers(0, np.iinfo(dtype).max + 1, size=(n, h, w), dtype=np.uint32).astype(dtype)
    return buf, view


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
@pytest.mark.parametrize("f", FACTORS)
def test_host_form_equals_the_numpy_restatement(f, dtype):
    for k, (w, h) in enumerate(SIZES):
        if w < f or h < f:
            continue
        for n, row_pad, frame_pad in ((1, 0, 0), (3, 5, 2)):
            _, src = padded(n, h, w, dtype, row_pad, frame_pad, seed=10 * k + f)
            ref = numpy_decimate(src, f)
            assert A.decimate(src, f).tobytes() == ref.tobytes(), (w, h, f, n)
            out_buf, out = padded(n, h // f, w // f, dtype, 3, 1, seed=99)
            before = out_buf.copy()
            A.decimate(src, f, out=out)
            assert np.array_equal(out, ref), (w, h, f, n)
            out_buf[:, :h // f, :w // f] = before[:, :h // f, :w // f]
            assert np.array_equal(out_buf, before), "a guard byte was written"
    lone = padded(1, 9, 7, dtype, 0, 0, seed=5)[1][0]
    assert A.decimate(lone, f).shape == (9 // f, 7 // f)  # [H, W] in, [H // f, W // f] out


@pytest.mark.parametrize("f", FACTORS)
def test_saturated_frames_do_not_overflow(f):
    for dtype in (np.uint8, np.uint16):
        top = np.iinfo(dtype).max
        out = A.decimate(np.full((2, 13, 17), top, dtype), f)
        assert out.shape == (2, 13 // f, 17 // f) and (out == top).all()


def _tail(w=8, h=8, f=2, fmt=_ffi.AGX_L8, n=1, row=None, dst_row=None, src=True, dst=True):
    px = 2 if fmt == _ffi.AGX_L16 else 3 if fmt == _ffi.AGX_RGB8 else 1
    a = np.zeros(4096, np.uint8)
    b = np.zeros(4096, np.uint8)
    row = w * px if row is None else row
    ow, oh = max(w // max(f, 1), 1), max(h // max(f, 1), 1)
    dst_row = ow * px if dst_row is None else dst_row
    return _ffi.lib().agx_decimate_tail(a.ctypes.data if src else None, n, w, h, row, row * h, fmt, f, b.ctypes.data if dst else None, dst_row,
                                        dst_row * oh)


def test_every_refused_argument():
    ARG, FORMAT = _ffi.AGX_ERR_ARG, _ffi.AGX_ERR_FORMAT
    assert _tail() == _ffi.AGX_OK and _tail(fmt=_ffi.AGX_L16, f=4) == _ffi.AGX_OK
    for over in (dict(w=1, f=2), dict(h=1, f=2), dict(w=3, f=4), dict(h=2, f=3), dict(f=1), dict(f=5), dict(f=0), dict(n=0), dict(n=65536),
                 dict(row=7), dict(dst_row=3), dict(src=False), dict(dst=False), dict(fmt=_ffi.AGX_L16, row=17),
                 dict(fmt=_ffi.AGX_L16, dst_row=9)):
        assert _tail(**over) == ARG, over
    for fmt in (_ffi.AGX_RGB8, _ffi.AGX_LF32, 99):
        assert _tail(fmt=fmt) == FORMAT, fmt
    with pytest.raises(A.AgxError) as e:
        A.decimate(np.zeros((3, 8), np.uint8), 4)
    assert e.value.status == ARG


@pytest.mark.parametrize("f", FACTORS)
def test_a_bright_block_lands_on_its_pixel_and_maps_back_to_its_centre(f):
    """One bright f x f block at (f X, f Y): the maximum of the decimated frame is at (X, Y), and X * f + 0.5 * (f - 1), the
    mapping of agx_refine_windows_enqueue's factor, is the block's centre."""
    w, h = 41, 29
    for X, Y in ((0, 0), (3, 2), (w // f - 1, h // f - 1)):
        img = np.full((h, w), 10, np.uint8)
        img[f * Y:f * Y + f, f * X:f * X + f] = 250
        out = A.decimate(img, f)
        assert np.unravel_index(np.argmax(out), out.shape) == (Y, X) and out[Y, X] == 250 and (out == 250).sum() == 1
        ys, xs = np.nonzero(img == 250)
        cx = np.float32(X) * np.float32(f) + np.float32(0.5) * np.float32(f - 1)
        cy = np.float32(Y) * np.float32(f) + np.float32(0.5) * np.float32(f - 1)
        assert cx == xs.mean() and cy == ys.mean()


def test_header_python_and_rust_name_the_new_entries():
    import os
    import re
    from tests.util import ROOT
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("agx_decimate_enqueue", "agx_decimate_tail", "agx_refine_windows_enqueue"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and ("pub fn %s(" % name) in rust, name
    assert "pub fn decimate_tail(" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
