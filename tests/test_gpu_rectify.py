"""k_rectify_map, k_remap and k_rectified_points on the GPU against their host forms, byte for byte, guard bytes between rows and
frames included (tests/test_rectify_cpu.py holds the host forms to numpy and scipy); remap -> detect on the device against
detect_batch of the host form's rectified frames; the batch-in-flight rule of the three calls."""
import numpy as np
import pytest

from tests import board_pose_cases as PC
from tests import rectify_cases as RC
from tests.rectify_cases import CAMERAS, DST, NEW_CAMERA, NONE, ROTATION, SRC

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi

pytestmark = pytest.mark.gpu

GROUP = 16  # csrc/rectify.h: REMAP_FRAMES_PER_GROUP


@pytest.fixture(scope="module")
def det():
    d = A.TagDetector("t36h11", None, device=0)
    yield d
    d.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def dev_padded(a, row_pad, frame_pad):
    """rectify_cases.padded on both sides -> (host view, host buffer, device view, device buffer)."""
    import torch
    view, buf = RC.padded(a, row_pad, frame_pad)
    px = a.itemsize
    t = torch.from_numpy(buf.copy()).cuda()
    typed = t if px == 1 else t.view(torch.int16)
    dview = typed.as_strided(a.shape, tuple(s // px for s in view.strides))
    return view, buf, dview, t


def synced(det):
    import torch
    det.sync()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dst", [(97, 61), (1, 1), (5, 3), (256, 4), (130, 7)])
@pytest.mark.parametrize("lens", ["radtan", "equi"])
def test_map_kernel_gives_the_host_forms_bytes(det, lens, dst):
    """Both lenses, with a rotation, into a map whose rows are padded: the padding keeps its pattern."""
    import torch
    cam = CAMERAS[lens]
    stride = 8 * dst[0] + 24
    want = A.rectify_map(cam, SRC, dst, NEW_CAMERA, ROTATION, row_stride=stride)
    buf = torch.full((dst[1], stride // 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
    out = buf[:, :2 * dst[0]].unflatten(1, (dst[0], 2))
    got = det.rectify_map_enqueue(cam, SRC, dst, NEW_CAMERA, ROTATION, out=out)
    synced(det)
    assert got is out
    assert buf.cpu().numpy().tobytes() == want.base.tobytes()
    if dst == (97, 61):
        assert 0 < (want[..., 0] == NONE).sum() < want[..., 0].size
        packed = det.rectify_map_enqueue(cam, SRC, dst, NEW_CAMERA, ROTATION)
        plain = det.rectify_map_enqueue(cam, SRC, dst, NEW_CAMERA)
        synced(det)
        assert np.array_equal(packed.cpu().numpy(), want)
        assert np.array_equal(plain.cpu().numpy(), A.rectify_map(cam, SRC, dst, NEW_CAMERA))


def _map(which):
    if which == "camera":
        return A.rectify_map(CAMERAS["equi"], SRC, DST, NEW_CAMERA, ROTATION)
    if which == "none":
        return np.full((7, 130, 2), NONE, np.int32)
    return RC.callers_map(SRC, {"callers": (130, 7), "wide": (256, 4), "one": (1, 1), "narrow": (5, 3)}[which])


# (map, row padding and frame padding of the destination in pixels).  97 and 130 are no multiples of the four pixels of a lane or
# of 64; a packed 97-pixel row and a row padded by 3 take the byte stores, 130 + 6 and the packed 256 the whole-dword stores.
LAYOUTS = [("camera", 0, 0), ("camera", 3, 8), ("callers", 6, 8), ("callers", 3, 5), ("wide", 0, 0), ("none", 6, 8), ("one", 0, 0), ("narrow", 1, 2)]


@pytest.mark.parametrize("n_frames", [1, 3, 5, GROUP + 1])
@pytest.mark.parametrize("which,row_pad,frame_pad", LAYOUTS)
@pytest.mark.parametrize("dtype,border", [(np.uint8, 201), (np.uint16, 51234)])
def test_remap_kernel_gives_the_host_forms_bytes(det, dtype, border, which, row_pad, frame_pad, n_frames):
    """L8 and L16, 1 / 3 / 5 frames and one more than a workgroup's frame group, padded source and destination strides with their
    guard bytes intact between rows and frames, a border above 255 for L16, the all-none map and the caller's out-of-range map."""
    px = np.dtype(dtype).itemsize
    m = _map(which)
    img = RC.image(n_frames, SRC, dtype)
    src_h, _, src_d, _ = dev_padded(img, 5 * px, 12 * px)
    zero = np.zeros((n_frames, m.shape[0], m.shape[1]), dtype)
    out_h, buf_h, out_d, buf_d = dev_padded(zero, row_pad * px, frame_pad * px)
    A.remap(src_h, m, border, out=out_h)
    got = det.remap_enqueue(src_d, dev(m), out=out_d, border=border)
    synced(det)
    assert got is out_d
    assert buf_d.cpu().numpy().tobytes() == buf_h.tobytes()
    assert np.array_equal(out_h, RC.numpy_remap(img, m, border))
    if which == "none":
        assert (out_h == border).all()


def test_remap_makes_its_own_output(det):
    m = _map("camera")
    for dtype in (np.uint8, np.uint16):
        img = RC.image(2, SRC, dtype)
        got = det.remap_enqueue(dev(img), dev(m))
        synced(det)
        assert got.cpu().numpy().tobytes() == A.remap(img, m).tobytes()


@pytest.mark.parametrize("lens", ["radtan", "equi"])
def test_points_kernel_gives_the_host_forms_bytes(det, lens):
    """On a tag table in place (the ids stay), and on a packed list with NaN, infinite and behind-camera points."""
    cam = CAMERAS[lens]
    rng = np.random.RandomState(11)
    table = np.zeros((3, 5), A.TagDetector.TAG_DTYPE)
    table["id"] = rng.randint(0, 587, (3, 5))
    table["xy"] = (rng.rand(3, 5, 8) * 120 - 10).astype(np.float32)
    want = table.copy()
    want["xy"] = A.rectified_points(table["xy"].reshape(3, 5, 4, 2), cam, NEW_CAMERA, ROTATION).reshape(3, 5, 8)
    t = dev(table.view(np.int32).reshape(3, 5, 9))
    assert det.rectified_points_enqueue(t, cam, NEW_CAMERA, ROTATION) is t
    synced(det)
    assert t.cpu().numpy().tobytes() == want.tobytes()
    R = PC.rotation(0.0, 75.0, 0.0)
    pts = (rng.rand(700, 2) * [DST[0] * 3, DST[1]]).astype(np.float32)
    pts[5] = (np.nan, 3.0)
    pts[6] = (2.0, np.inf)
    want = A.rectified_points(pts, cam, NEW_CAMERA, R)
    assert 20 < np.isnan(want[:, 0]).sum() < 680
    p = dev(pts)
    got = det.rectified_points_enqueue(p, cam, NEW_CAMERA, R)
    synced(det)
    assert got.cpu().numpy().tobytes() == want.tobytes() and p.cpu().numpy().tobytes() == pts.tobytes()
    assert det.rectified_points_enqueue(p, cam, NEW_CAMERA, R, out=p) is p  # in place
    synced(det)
    assert p.cpu().numpy().tobytes() == want.tobytes()


def _fisheye_batch():
    luma, cam, _, (w, h) = RC.fisheye_frame(0.35)
    return np.stack([luma, np.roll(luma, 3, axis=1), np.roll(luma, -2, axis=0)]), cam, (w, h)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for t in x:
            assert np.asarray(x[t]).tobytes() == np.asarray(y[t]).tobytes()


def test_remap_then_detect_on_the_device(det):
    """Three frames behind the 0.35 fisheye: the device's map is the host form's, remap_enqueue followed by detect_batch_enqueue on
    its output equals detect_batch of the host form's rectified frames, and detect_rectified(to_source=True) equals the composition
    of the host forms."""
    frames, cam, (w, h) = _fisheye_batch()
    m = A.rectify_map(cam, (w, h))
    rect = A.remap(frames, m)
    want = det.detect_batch(rect)
    assert min(len(f) for f in want) >= 15
    m_d = det.rectify_map_enqueue(cam, (w, h))
    rect_d = det.remap_enqueue(dev(frames), m_d)
    det.detect_batch_enqueue(rect_d)
    got = det.detect_batch_fetch()
    assert m_d.cpu().numpy().tobytes() == m.tobytes() and rect_d.cpu().numpy().tobytes() == rect.tobytes()
    _same(got, want)
    _same(det.detect_rectified(dev(frames), cam), want)
    back = [{t: A.rectified_points(xy, cam, None) for t, xy in f.items()} for f in want]
    _same(det.detect_rectified(dev(frames), cam, to_source=True), back)
    assert len(det._rectify_maps) == 1  # (one map for the three calls)


def test_the_calls_follow_the_batch_in_flight_rule(det):
    """Each of the three calls replaces the batch in flight (a pending fetch of another kind is AGX_ERR_STATE afterwards); refused,
    it leaves the batch where it was."""
    import torch
    lib, cam = _ffi.lib(), CAMERAS["equi"]
    frames = dev(RC.image(2, SRC, np.uint8))
    m = dev(_map("camera"))
    pts = dev(np.zeros((4, 2), np.float32))
    counts = np.zeros(2, np.uint32)
    fetch = lambda: lib.agx_saddles_batch_fetch(det._h, None, 0, counts.ctypes.data, None)
    calls = {
        "map": (lambda: det.rectify_map_enqueue(cam, SRC, DST, NEW_CAMERA), lambda: det.rectify_map_enqueue(cam, SRC, DST, (0.0, 50.0, 1.0, 1.0))),
        "remap": (lambda: det.remap_enqueue(frames, m), lambda: det.remap_enqueue(frames, m, border=256)),
        "points": (lambda: det.rectified_points_enqueue(pts, cam, NEW_CAMERA), lambda: det.rectified_points_enqueue(pts, cam, (0.0, 1.0, 1.0, 1.0))),
    }
    big = torch.zeros((2, 64, 96), dtype=torch.uint8, device="cuda:0")
    for name, (good, bad) in calls.items():
        det.saddles_batch_enqueue(big)
        with pytest.raises(A.AgxError) as e:
            bad()
        assert e.value.status == _ffi.AGX_ERR_ARG, name
        assert fetch() in (_ffi.AGX_OK, _ffi.AGX_ERR_CAPACITY), name  # the saddle batch is still in flight
        det.saddles_batch_enqueue(big)
        good()
        assert fetch() == _ffi.AGX_ERR_STATE, name
        with pytest.raises(A.AgxError) as e:
            det.saddles_batch_fetch()
        assert e.value.status == _ffi.AGX_ERR_STATE, name
    synced(det)
