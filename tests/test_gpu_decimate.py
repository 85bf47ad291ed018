"""k_decimate (agx_decimate_enqueue) against the host form (agx_decimate_tail, itself held to a numpy restatement by
tests/test_decimate_cpu.py): every byte of the destination buffer, guard bytes included.  The layouts walk every path of the
kernel: source loads of 16, 8 and 4 bytes and pixel by pixel (pointers off by 1 and 3 bytes; 16-bit: by 1 and 3 pixels), whole
dword stores and pixel stores, the short last quad of a row, rows and frames with padding, batches of 1 and 5."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = ((2, 2), (3, 2), (5, 3), (8, 8), (9, 7), (67, 45), (130, 4)) + tuple((w, 6) for w in range(1, 10))  # (W, H)
GUARD = 0xA5
# (source offset in pixels, source row stride: None tight / else padded to 16 bytes plus this many bytes, destination offset,
#  destination row padding in pixels)
LAYOUTS = ((0, None, 0, 0), (0, 0, 0, 0), (0, 8, 0, 4), (0, 4, 0, 3), (1, None, 0, 0), (3, 0, 1, 5), (1, 4, 3, 8))


@pytest.fixture(scope="module")
def det():
    import aprilgrid_rs_amd as A
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def view(buf, off, n, h, w, row, frame):
    """[n, h, w] of a flat buffer (numpy or torch) from element `off`, rows `row` and frames `frame` elements apart"""
    if isinstance(buf, np.ndarray):
        return np.lib.stride_tricks.as_strided(buf[off:], (n, h, w), (frame * buf.itemsize, row * buf.itemsize, buf.itemsize))
    return buf.as_strided((n, h, w), (frame, row, 1), off)


@pytest.mark.parametrize("dtype", ("uint8", "uint16"))
@pytest.mark.parametrize("f", (2, 3, 4))
def test_every_destination_byte_equals_the_host_forms(det, f, dtype):
    import torch
    import aprilgrid_rs_amd as A
    np_dtype = np.dtype(dtype)
    px = np_dtype.itemsize
    t_dtype = torch.uint8 if px == 1 else torch.int16
    rng = np.random.default_rng(7 * f + px)
    ran = 0
    for w, h in SIZES:
        if w < f or h < f:
            with pytest.raises(A.AgxError) as e:
                det.decimate_enqueue(torch.zeros((1, h, w), dtype=t_dtype, device="cuda:0"), f)
            assert e.value.status == A._ffi.AGX_ERR_ARG
            continue
        ow, oh = w // f, h // f
        for n in (1, 5):
            for s_off, s_pad, d_off, d_pad in LAYOUTS:
                s_row = w if s_pad is None else ((w * px + 15) // 16 * 16 + s_pad) // px
                s_frame = s_row * (h + (0 if s_pad is None else 2))
                d_row, d_frame = ow + d_pad, (ow + d_pad) * (oh + (1 if d_pad else 0))
                src = rng.integers(0, np.iinfo(np_dtype).max + 1, size=s_off + n * s_frame + 8, dtype=np.uint32).astype(np_dtype)
                dst = np.full(d_off + n * d_frame + 8, GUARD * (0x0101 if px == 2 else 1), np_dtype)
                d_src = torch.from_numpy(src.view(np.int16) if px == 2 else src).to("cuda:0")
                d_dst = torch.from_numpy(dst.view(np.int16) if px == 2 else dst).to("cuda:0")
                A.decimate(view(src, s_off, n, h, w, s_row, s_frame), f, out=view(dst, d_off, n, oh, ow, d_row, d_frame))
                got = det.decimate_enqueue(view(d_src, s_off, n, h, w, s_row, s_frame), f, out=view(d_dst, d_off, n, oh, ow, d_row, d_frame))
                det.sync()
                assert got.shape == (n, oh, ow)
                assert d_dst.cpu().numpy().tobytes() == dst.tobytes(), (w, h, n, s_off, s_pad, d_off, d_pad)
                ran += 1
    assert ran >= 100


def test_made_output_and_refusals(det):
    import torch
    import aprilgrid_rs_amd as A
    frames = torch.randint(0, 256, (2, 45, 67), dtype=torch.uint8, device="cuda:0")
    out = det.decimate_enqueue(frames, 3)
    det.sync()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 15, 22)
    assert out.cpu().numpy().tobytes() == A.decimate(frames.cpu().numpy(), 3).tobytes()
    for factor in (1, 5):
        with pytest.raises(A.AgxError) as e:
            det.decimate_enqueue(frames, factor)
        assert e.value.status == A._ffi.AGX_ERR_ARG
    rgb = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda:0")
    lib, h = A._ffi.lib(), det._h
    assert lib.agx_decimate_enqueue(h, rgb.data_ptr(), 1, 8, 8, 24, 192, A._ffi.AGX_RGB8, 2, out.data_ptr(), 4, 16) == A._ffi.AGX_ERR_FORMAT
