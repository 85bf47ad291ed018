"""The decode stage at its limits on the device (reference src/detector.rs:42-169, 448-476).

k_decode_quads on the hand-painted tags of tests/tag_cases.py -- what every case claims is proven on the CPU in
tests/test_tag_cases_cpu.py --: one detector per family, all of the family's cases in one batch (a frame, a quad and a slot per
case; the slot is the case's position, shuffled so that every kind of limit falls on all four quad rows of a wave and on both
sides of a workgroup's 16-slot boundary), equal to the host form byte for byte, to the yardstick of
tests/test_decode_quads_cpu.py in every field with NO exclusions, and to the status each case intends.

k_board_tail's copy of the same functions (other lane layout) cannot be given painted planes: it decodes the quads of a board the
chain found.  It runs on rendered T36H11 and T25H7 boards whose tag p carries p % (thres + 1) flipped code bits, as rendered and
turned by one, two and three quarter turns, against the oracle's detect on the same pixels."""
import numpy as np
import pytest

from tests import tag_cases as T
from tests.test_decode_quads_cpu import DECODED, TAG_DTYPE, check_zero_records, yardstick_many
from tests.util import check_tags

pytestmark = pytest.mark.gpu

AGX_ERR_STATE = -7


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("fam", T.FAMILIES)
def test_painted_cases_through_k_decode_quads(fam):
    import aprilgrid_rs_amd as A
    cs = T.family_cases(fam)
    n = len(cs)
    planes = np.stack([c.plane for c in cs])
    quads = np.stack([c.quad for c in cs]).reshape(n, 1, 8)
    d = A.TagDetector(fam, None, device=0)
    try:
        d.decode_quads_enqueue(dev(planes), dev(quads))
        tags, st, bits = d.decode_quads_fetch()
    finally:
        d.close()
    tags, st, bits = tags[:, 0], st[:, 0], bits[:, 0]
    check_zero_records(tags, st, bits, fam)
    bad = []
    for i, c in enumerate(cs):
        # the host form, byte for byte
        ht, hs, hb = A.decode_quads_tail(fam, c.plane, c.quad[None], with_bits=True)
        if not (tags[i:i + 1].tobytes() == ht.tobytes() and st[i] == hs[0] and bits[i] == hb[0]):
            bad.append((c.name, "host form", int(st[i]), int(hs[0]), int(bits[i]), int(hb[0])))
        # the yardstick, every field, no exclusions
        ys, yt, yb, _ = yardstick_many(c.plane, c.quad[None], fam)
        if not (st[i] == ys[0] and bits[i] == yb[0] and tags[i:i + 1].tobytes() == yt.tobytes()):
            bad.append((c.name, "yardstick", int(st[i]), int(ys[0]), int(bits[i]), int(yb[0])))
        # what the case intends, and the builder's own expectation
        es, eid, exy, eb = c.expect
        ref = np.zeros(1, TAG_DTYPE)
        if es == DECODED:
            ref[0]["id"], ref[0]["xy"] = eid, exy
        if not (st[i] == es and int(bits[i]) == eb and tags[i:i + 1].tobytes() == ref.tobytes()):
            bad.append((c.name, "expectation", int(st[i]), es, int(bits[i]), eb))
        if "status" in c.intent and st[i] != c.intent["status"]:
            bad.append((c.name, "intended status", int(st[i]), c.intent["status"]))
        if "not_status" in c.intent and st[i] == c.intent["not_status"]:
            bad.append((c.name, "status not intended", int(st[i])))
    assert not bad, (len(bad), bad[:12])
    assert len(np.unique(st)) == 5, np.bincount(st.astype(np.int64))


def tail_detector(fam, device_tail):
    import aprilgrid_rs_amd as A
    d = A.TagDetector(fam, None, device=0)
    try:
        d.set_option("device_tail", device_tail)
    except A.AgxError as e:  # this process's atan2f is not the routine the kernel restates: the device tail is refused
        d.close()
        if device_tail == 1 and e.status == AGX_ERR_STATE:
            pytest.skip("device tail refused on this host (AGX_ERR_STATE)")
        raise
    return d


@pytest.mark.parametrize("device_tail", [1, 0])
@pytest.mark.parametrize("fam", sorted(T.TAIL_SPEC))
def test_boards_with_flipped_bits_through_both_tails(fam, device_tail):
    frames, ks = T.tail_frames(fam)
    refs = T.tail_oracle(fam)
    thres = T.family(fam)[2]
    d = tail_detector(fam, device_tail)
    answered = 0
    try:
        for shape in sorted(set(f.shape for f in frames)):  # (the quarter turns have the other shape: a batch each)
            at = [i for i, f in enumerate(frames) if f.shape == shape]
            d.detect_batch_enqueue(dev(np.stack([frames[i] for i in at])), cap=64)
            got = d.detect_batch_fetch(n_threads=2)
            if device_tail == 1:
                assert d.get_option("last_device_tail_frames") == len(at)
                answered += len(at) - d.get_option("last_device_tail_fallbacks")
            else:
                assert d.get_option("last_device_tail_frames") == 0
            for i, g in zip(at, got):
                check_tags(g, refs[i], "%s frame %d, device_tail %d" % (fam, i, device_tail))
                assert all(ks[t] < thres for t in g)
    finally:
        d.close()
    print(fam, "device_tail", device_tail, "frames answered by the kernel:", answered, "of", len(frames))
    if device_tail == 1:
        assert answered >= 1, "every frame was handed back to the host tail: nothing was asked of k_board_tail"
