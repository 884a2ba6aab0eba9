"""The crafted find_longest_line cases (tests/longest_line_cases.py; their checks are asserted on the oracle by
tests/test_longest_line_host.py) through Vision::find_longest_line on the device -- mode 1 of k_lsd -- against the oracle on the
oracle's own mask: all four coordinates and len², bit for bit, no tolerance (NaN equal to NaN for the non-finite starts).

Per (size, family): every case's frame through the trait sequence, the lsd image equal to the reference mask, then the case's
calls forward and once more reversed on the same loaded frame (the answers may not depend on the call before: unit_key / cand_*
are reset per call, and GLOBAL's row cache is re-centred).  Beside that: the calls touch no record but their own (find_marker_lines
and lsd_stats before and after a block of them), a frame loaded from a torch tensor, and a FrameBatch run in between on the same
context."""
import numpy as np
import pytest

import longest_line_cases as L
import lsd_cases as C
from oracle import oracle as o

pytestmark = pytest.mark.gpu

SIZE_IDS = {C.SMALL: "768p", C.HD: "1080p", C.QHD: "1440p", C.WIDE: "ultrawide"}


def _load(vision, frame):
    """The trait sequence up to the marker mask (vision-gpu/src/lib.rs:562-622)."""
    vision.load_frame(frame)
    assert vision.crop_to_map(True) is not None
    vision.isolate_map_markers()
    vision.mask_marker_lines()


def _calls(vision, P, calls, tag=""):
    """Every call against the oracle; -> the device's answers."""
    got = []
    for (px, py, gap) in calls:
        line, l2 = vision.find_longest_line((px, py), gap)
        ref = o.find_longest_line(P.mask, px, py, gap)
        print("%s %s (%r, %r) gap %r: device %s %r, oracle %s %r" % (P.case.name, tag, px, py, gap, line, l2, ref[0], ref[1]))
        assert L.same((line, l2), ref), (P.case.name, P.size, tag, px, py, gap, line, l2, ref)
        got.append((line, l2))
    return got


PARAMS = [(size, family) for size in C.SIZES for family in L.FAMILIES if L.cases_at(size, family)]


@pytest.mark.parametrize("size,family", PARAMS, ids=["%s-%s" % (SIZE_IDS[s_], f) for s_, f in PARAMS])
def test_find_longest_line_equals_the_oracle(vision, size, family):
    n = 0
    for P in L.reference(size):
        if P.case.family != family:
            continue
        _load(vision, L.frame(P.case, *size))
        assert np.array_equal(vision.lsd_image(), P.mask), P.case.name
        fwd = _calls(vision, P, P.calls, "forward")
        rev = _calls(vision, P, P.calls[::-1], "reversed")[::-1]
        assert all(L.same(a, b) for a, b in zip(fwd, rev)), P.case.name
        n += len(P.calls)
    assert 0 < n <= L.MAX_CALLS


def _placed(size, name):
    return [P for P in L.reference(size) if P.case.name == name][0]


@pytest.mark.parametrize("size,name", [(C.SMALL, "tie_cross_70"), (C.HD, "hand_fatal_from_64"), (C.QHD, "res_xwin"), (C.QHD, "res_global")],
                         ids=lambda v: SIZE_IDS.get(v, v))
def test_the_scratch_record_is_the_only_one_touched(vision, size, name):
    P = _placed(size, name)
    _load(vision, L.frame(P.case, *size))
    ref_lines, ref_stats = o.find_lines(P.mask, 15)
    before = (vision.find_marker_lines(15), vision.lsd_stats(15, exact=False), vision.lsd_stats(15, exact=True))
    assert np.array_equal(before[0], ref_lines) and before[2] == (ref_stats["rounds"], ref_stats["steps"]), (name, before, ref_lines, ref_stats)
    _calls(vision, P, P.calls)
    after = (vision.find_marker_lines(15), vision.lsd_stats(15, exact=False), vision.lsd_stats(15, exact=True))
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:], (name, before, after)
    assert np.array_equal(vision.lsd_image(), P.mask)
    _calls(vision, P, P.calls, "after find_marker_lines")


def test_a_frame_in_a_torch_tensor(vision):
    import torch
    for size, name in ((C.HD, "hand_white_again_at_64"), (C.QHD, "res_global")):
        P = _placed(size, name)
        d = torch.from_numpy(L.frame(P.case, *size)).cuda()
        torch.cuda.synchronize()
        vision.load_frame_device(d.data_ptr(), size[0], size[1])
        assert vision.crop_to_map(True) is not None
        vision.isolate_map_markers()
        vision.mask_marker_lines()
        assert np.array_equal(vision.lsd_image(), P.mask)
        _calls(vision, P, P.calls)
        del d


def test_a_frame_batch_in_between_changes_nothing(vision):
    """The per-call batch's state (its frame, mask, bounding box and scratch record) does not depend on a FrameBatch of other frames
    run on the same context."""
    import torch
    import squad_mortar_helper_amd as smh
    size = C.HD
    P = _placed(size, "over_rect_200x120")
    others = [_placed(size, n) for n in ("tie_cross_70", "short_h_K49", "hand_fatal_from_64")]
    _load(vision, L.frame(P.case, *size))
    first = _calls(vision, P, P.calls)
    d = torch.from_numpy(np.stack([L.frame(Q.case, *size) for Q in others])).cuda()
    fb = smh.FrameBatch(vision, size[0], size[1], len(others))
    try:
        fb.run(d.data_ptr(), len(others), stages=smh.STAGE_MARKERS, max_gap=15, stream=torch.cuda.current_stream().cuda_stream)
        recs = smh.results_to_dicts(fb.read_results(0, len(others)))
        for r, Q in zip(recs, others):
            assert np.array_equal(r["lines"], o.find_lines(Q.mask, 15)[0]), Q.case.name
        again = _calls(vision, P, P.calls, "after the batch")
        assert all(L.same(a, b) for a, b in zip(first, again))
        assert np.array_equal(vision.lsd_image(), P.mask)
    finally:
        fb.close()
