"""Every per-frame outcome of "detect over a batch" in ONE call, through every entry point: agx_detect_batch with the device
tail, with the host tail and on device-resident frames, agx_detect_batch_enqueue + _fetch into host arrays and into the caller's
device arrays, in L8 and L16.  The entry points share one statement of the per-frame rules (csrc/detect_batch.cpp: FrameResults,
HostTail, read_tail_table, take_host_frames); the other tests exercise mostly one outcome per call.

The batch: 8 frames of 640 x 480 (synth.py), measured with a detector without limits:

  frame  what                         saddles  tags   outcome under cap 20, max_saddles 1000, tail_debug_band 50
  0      flat                               0     0   (a) count 0, AGX_OK
  1      board 3 x 3, pose 0               66     9   (b) 9 tags; the device tail keeps it
  2      board 3 x 3, pose 3               66     9   (b) + (e): handed back as uncertain, the host tail's 9 tags
  3      board 6 x 6, pose 1              177    36   (c) AGX_ERR_CAPACITY, count 36, no row written
  4      board 6 x 6, pose 0              189    36   (c) + (e)
  5      noise                           2102     0   (d) the chain's list overflows: count 0, AGX_ERR_CAPACITY
  6      board 4 x 4, pose 1              113    16   (b) the device tail keeps it
  7      board 4 x 4, pose 0              120    16   (b) + (e)

The expected results are not these figures but per-frame detect() and refined_saddle_points() of a detector without limits,
plus the rules; the figures are asserted as the test's preconditions (cap and max_saddles lie between them)."""
import numpy as np
import pytest

from tests.util import synth_module

pytestmark = pytest.mark.gpu

AGX_OK, AGX_ERR_CAPACITY, AGX_ERR_STATE = 0, -3, -7
W, H, CAP, MAX_SADDLES, BAND = 640, 480, 20, 1000, 50
THREADS = 2
FRAMES = [("flat",), (3, 3, 0), (3, 3, 3), (6, 6, 1), (6, 6, 0), ("noise", 100), (4, 4, 1), (4, 4, 0)]
FLAT, KEPT, BACK, OVER_CAP, NOISE = 0, (1, 6), (2, 7), (3, 4), 5
SENTINEL_BYTE = 0xA5
SENTINEL_I32 = -0x21524111  # 0xDEADBEEF


def A():
    import aprilgrid_rs_amd
    return aprilgrid_rs_amd


def expected(free, frames):
    """The rules, from a detector without limits: a chain list beyond max_saddles voids the frame; more tags than cap are
    reported with their count; either way no row is written.  The call: the lowest non-OK frame's status (here every such
    status is AGX_ERR_CAPACITY, so "the first recorded" of agx_detect_batch is the same)."""
    exp = []
    for img in frames:
        tags = free.detect(img)
        rows = np.zeros(len(tags), A().TagDetector.TAG_DTYPE)
        for k, (tid, xy) in enumerate(tags.items()):
            rows[k] = (tid, np.asarray(xy, np.float32).reshape(8))
        n_saddles = len(free.refined_saddle_points(img, as_array=True, cap=65536))
        if n_saddles > MAX_SADDLES:
            exp.append(dict(count=0, status=AGX_ERR_CAPACITY, rows=None, saddles=n_saddles, tags=len(tags)))
        elif len(tags) > CAP:
            exp.append(dict(count=len(tags), status=AGX_ERR_CAPACITY, rows=None, saddles=n_saddles, tags=len(tags)))
        else:
            exp.append(dict(count=len(tags), status=AGX_OK, rows=rows, saddles=n_saddles, tags=len(tags)))
    return exp


@pytest.fixture(scope="module")
def batch():
    """-> {format: (host frames, device tensor, expected)}"""
    import torch
    synth = synth_module()
    codes = synth.t36h11_codes()
    imgs = []
    for f in FRAMES:
        if f[0] == "flat":
            imgs.append(np.full((H, W), 128, np.uint8))
        elif f[0] == "noise":
            imgs.append(synth.render_frame(f[1], W, H, "cuda", None, codes, pure_noise=True)[0].cpu().numpy())
        else:
            imgs.append(synth.render_frame(f[2], W, H, "cuda", synth.BoardSpec(rows=f[0], cols=f[1]), codes)[0].cpu().numpy())
    l8 = np.stack(imgs)
    l16 = l8.astype(np.uint16) * 257
    free = A().TagDetector("t36h11", None, device=0)
    res = {}
    for name, fr in (("L8", l8), ("L16", l16)):
        exp = expected(free, fr)
        print(name, [(e["saddles"], e["tags"]) for e in exp])
        # the preconditions: each outcome is in the batch, and cap and max_saddles lie between the figures they separate
        assert exp[FLAT]["tags"] == 0 and exp[FLAT]["status"] == AGX_OK
        assert all(0 < exp[i]["tags"] <= CAP and exp[i]["status"] == AGX_OK for i in KEPT + BACK), exp
        assert all(exp[i]["tags"] > CAP and exp[i]["saddles"] <= MAX_SADDLES for i in OVER_CAP), exp
        assert exp[NOISE]["saddles"] > MAX_SADDLES and exp[NOISE]["count"] == 0
        dev = torch.from_numpy(fr.view(np.int16) if fr.dtype == np.uint16 else fr).cuda()
        res[name] = (fr, dev, exp)
    free.close()
    return res


@pytest.fixture(scope="module", params=[1, 0], ids=["device_tail", "host_tail"])
def det(request):
    d = A().TagDetector("t36h11", None, device=0)
    try:
        d.set_option("device_tail", request.param)
    except A().AgxError as e:  # this process's atan2f is not the routine the kernel restates: the device tail is refused
        d.close()
        if request.param == 1 and e.status == AGX_ERR_STATE:
            pytest.skip("device tail refused on this host (AGX_ERR_STATE)")
        raise
    d.set_limits(max_saddles=MAX_SADDLES)
    d.set_option("tail_debug_band", BAND)
    yield d, request.param
    d.close()


def check(got, exp, sentinel, d, device_tail, what):
    rc, out, cnt, st = got
    print(what, "rc", rc, "counts", list(cnt), "statuses", list(st), "handed back", d.get_option("last_device_tail_fallbacks"),
          "uncertain", d.get_option("last_device_tail_uncertain"))
    assert rc == AGX_ERR_CAPACITY, (what, rc)
    assert [int(c) for c in cnt] == [e["count"] for e in exp], (what, list(cnt))
    assert [int(s) for s in st] == [e["status"] for e in exp], (what, list(st))
    for f, e in enumerate(exp):
        if e["status"] == AGX_OK:
            assert out[f, : e["count"]].tobytes() == e["rows"].tobytes(), "%s: rows of frame %d" % (what, f)
        else:
            assert out[f].tobytes() == sentinel * (out[f].nbytes // len(sentinel)), "%s: frame %d is not OK, yet its rows were written" % (what, f)
    if device_tail:  # (e): some board frames were handed back as uncertain and some were kept; the noise frame is not counted
        back, unc = d.get_option("last_device_tail_fallbacks"), d.get_option("last_device_tail_uncertain")
        assert d.get_option("last_device_tail_frames") == len(exp)
        assert 1 <= unc <= back < len(KEPT + BACK + OVER_CAP), (what, back, unc)
        assert back >= len(OVER_CAP), (what, back)  # (the kernel's limit is cap: it hands frames beyond it back)
    else:
        assert d.get_option("last_device_tail_frames") == 0


def host_out(n):
    out = np.zeros((n, CAP), A().TagDetector.TAG_DTYPE)
    out.view(np.uint8)[:] = SENTINEL_BYTE
    return out


@pytest.mark.parametrize("fmt", ["L8", "L16"])
def test_blocking_call_on_host_frames(det, batch, fmt):
    d, device_tail = det
    fr, _, exp = batch[fmt]
    got = d.detect_batch_raw(fr, n_threads=THREADS, cap=CAP, out=host_out(len(fr)))
    check(got, exp, bytes([SENTINEL_BYTE]), d, device_tail, "agx_detect_batch %s" % fmt)


def test_blocking_call_on_device_frames(det, batch):
    d, device_tail = det
    fr, dev, exp = batch["L8"]
    got = d.detect_batch_raw(fr, n_threads=THREADS, cap=CAP, device_frames=dev, out=host_out(len(fr)))
    check(got, exp, bytes([SENTINEL_BYTE]), d, device_tail, "agx_detect_batch, device_frames")


@pytest.mark.parametrize("fmt", ["L8", "L16"])
def test_enqueue_and_fetch_into_host_arrays(det, batch, fmt):
    d, device_tail = det
    _, dev, exp = batch[fmt]
    d.detect_batch_enqueue(dev, cap=CAP)
    got = d.detect_batch_fetch_raw(THREADS)  # (its rows start as zeros)
    check(got, exp, b"\0", d, device_tail, "enqueue + fetch %s" % fmt)


def test_enqueue_to_device_arrays(det, batch):
    import torch
    d, device_tail = det
    _, dev, exp = batch["L8"]
    n = len(exp)
    out = (torch.full((n, CAP, 9), SENTINEL_I32, dtype=torch.int32, device="cuda"),
           torch.full((n,), SENTINEL_I32, dtype=torch.int32, device="cuda"),
           torch.full((n,), SENTINEL_I32, dtype=torch.int32, device="cuda"))
    d.detect_batch_enqueue(dev, cap=CAP, out=out)
    rc, tags, counts, status = d.detect_batch_fetch_raw(THREADS)
    host = np.ascontiguousarray(tags.cpu().numpy()).view(A().TagDetector.TAG_DTYPE).reshape(n, CAP)
    got = (rc, host, counts.cpu().numpy().astype(np.uint32), status.cpu().numpy())
    check(got, exp, np.int32(SENTINEL_I32).tobytes(), d, device_tail, "enqueue_to + fetch")
