"""The heightmap overlay on the device, byte for byte against the restatement (tests/overlay_ref.py): the per-call path on the
golden fixtures, SMHV_STAGE_HEIGHTMAP_OVERLAY through a batch and both pipeline schedules, heightmap switching and lifetime, and
the stage's validation."""
import numpy as np
import pytest

import firing_ref as R
import overlay_ref as O
from fixtures import OPEN_STEMS, load_fixture
from test_firing_gpu import _frames_with_minimaps

pytestmark = pytest.mark.gpu


def _hm(seed, w, h, lo=0, hi=65536):
    return np.random.default_rng(seed).integers(lo, hi, size=(h, w), dtype=np.uint16)


def test_per_call_path_on_the_golden_fixtures(vision):
    import squad_mortar_helper_amd as smh
    maps = [(_hm(1, 640, 480), ((-15, 9), (0, 0))),               # smaller than the rectangles
            (_hm(2, 2049, 1537, 100, 60000), ((37, -21), (0, 0))),    # larger, odd sizes
            (_hm(3, 333, 97), ((-333, 5), (0, 0))),                   # W + b00 == 0 in offset mode: nothing covered
            (np.full((17, 23), 4242, np.uint16), ((4, 4), (0, 0)))]   # constant
    hms = [(smh.Heightmap(vision, d, b, (1.0, 1.0, 1.0)), R.color_map(d), b) for d, b in maps]
    checked = 0
    for stem in OPEN_STEMS:
        frame, _, _ = load_fixture(stem)
        for gray in (True, False):
            vision.load_frame(frame)
            r = vision.crop_to_map(grayscale=gray)
            assert r is not None, stem
            ui = r[0]
            rect = vision.find_minimap()
            ui_seen = vision.ui_map(copy=True)
            if rect is None:
                continue
            for k, (hm, cm, b) in enumerate(hms):
                for fit in (True, False):
                    got = vision.heightmap_overlay(hm, fit_to_minimap=fit)
                    want = O.overlay(ui, rect, cm, b[0][0], b[0][1], fit)
                    assert got.shape == ui.shape and np.array_equal(got, want), (stem, gray, k, fit, np.argwhere(got != want)[:4])
                    checked += 1
                    if k == 2 and not fit:
                        assert np.array_equal(got, ui), stem
            # the call changes nothing of what the trait path hands out
            assert vision.find_minimap() == rect and np.array_equal(vision.ui_map(copy=True), ui_seen), stem
    assert checked >= 40, checked
    # errors follow the trait path: a closed map is SMHV_E_STATE
    frame, _, _ = load_fixture("a_point_png")
    vision.load_frame(frame)
    assert vision.crop_to_map() is None
    with pytest.raises(smh.VisionError) as ei:
        vision.heightmap_overlay(hms[0][0])
    assert ei.value.code == smh._lib.E_STATE
    for hm, _, _ in hms:
        hm.close()


def _images(fb, N):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    return [bytes(fb.read_image(w, f).tobytes()) for f in range(N) for w in (L.IMAGE_UI_MAP, L.VIEW_LSD_INPUT, L.VIEW_OCR_INPUT, L.VIEW_FIND_SCALES_INPUT)]


def _covered_frames(N):
    """_frames_with_minimaps: the walk stops at once on a flat rectangle (a zero-size quad: nothing covered); frames i % 4 == 3 have
    none and the walk reaches the ROI's edges (the whole ROI covered); the last frame is closed."""
    return sum(1 for f in range(N - 1) if f % 4 == 3)


def _check_overlays(get, recs, uis, cm, b, fit, ctx):
    """Every open frame's overlay against the restatement -> how many of them differ from their ui_map."""
    covered = 0
    for f, rec in enumerate(recs):
        if not rec["map_open"]:
            continue
        got = get(f)
        want = O.overlay(uis[f], rec["minimap"], cm, b[0][0], b[0][1], fit)
        assert np.array_equal(got, want), (ctx, f, np.argwhere(got != want)[:4])
        covered += int(np.any(got != uis[f]))
    return covered


def test_stage_through_a_batch_leaves_every_other_output_alone(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 16
    frames, anchors = _frames_with_minimaps(N, 500)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    data, bounds = _hm(7, 1201, 803), ((-40, 25), (0, 0))
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 30.0))
    cm = R.color_map(data)
    base = smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_FIRING
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    fb.set_firing(hm, fit_to_minimap=False)
    for read in (lambda: fb.read_overlay(0), fb.overlay_ptr):   # nothing to read before the first overlay run
        with pytest.raises(smh.VisionError) as ei:
            read()
        assert ei.value.code == smh._lib.E_STATE
    fb.run(d.data_ptr(), N, stages=base, anchors=anchors, stream=s)
    recs_plain = bytes(fb.read_results(0, N))
    imgs_plain = _images(fb, N)
    fire_plain = [a.tobytes() for a in fb.read_firing(0, N)]
    fb.run(d.data_ptr(), N, stages=base | smh.STAGE_HEIGHTMAP_OVERLAY, anchors=anchors, stream=s)
    raw = fb.read_results(0, N)
    assert bytes(raw) == recs_plain and _images(fb, N) == imgs_plain and [a.tobytes() for a in fb.read_firing(0, N)] == fire_plain
    recs = smh.results_to_dicts(raw)
    assert not recs[N - 1]["map_open"] and all(recs[f]["map_open"] for f in range(N - 1))
    uis = [fb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]
    assert _check_overlays(fb.read_overlay, recs, uis, cm, bounds, False, "batch") == _covered_frames(N) == 3
    assert not np.any(fb.read_overlay(N - 1)), "a closed frame is left alone (the fresh slab's zeros)"
    assert fb.overlay_ptr() != 0
    fb.close()
    hm.close()


def test_both_pipeline_schedules_give_the_batch_overlays(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 12
    frames, anchors = _frames_with_minimaps(N, 900)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    data, bounds = _hm(8, 800, 600), ((-40, 25), (0, 0))
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 30.0))
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_HEIGHTMAP_OVERLAY
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    fb.set_firing(hm)
    fb.run(d.data_ptr(), N, stages=stages, anchors=anchors, stream=s)
    recs = bytes(fb.read_results(0, N))
    want = [fb.read_overlay(f).tobytes() for f in range(N - 1)]
    uis = [fb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]
    assert _check_overlays(fb.read_overlay, smh.results_to_dicts(fb.read_results(0, N)), uis, R.color_map(data), bounds, True, "batch") == _covered_frames(N) == 2
    fb.close()
    for depth, search in ((4, "batch"), (3, "frame")):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=depth, search=search)
        p.set_firing(hm)
        slots = [p.submit(d.data_ptr(), N, stages=stages, anchors=anchors) for _ in range(depth + 1)]
        p.wait()
        for sl in set(slots):
            assert bytes(p.slots[sl].read_results(0, N)) == recs, (search, sl)
            assert [p.slots[sl].read_overlay(f).tobytes() for f in range(N - 1)] == want, (search, sl)
            assert p.slots[sl].overlay_ptr() != 0
        p.close()
    hm.close()


def test_switching_heightmaps_between_submissions_and_destroying_a_bound_one(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 8
    frames, anchors = _frames_with_minimaps(N, 1300)
    d = torch.from_numpy(frames).cuda()
    a_data, b_data = _hm(21, 500, 400), _hm(22, 901, 301, 7, 40000)
    ba, bb = ((3, -2), (0, 0)), ((-50, 11), (0, 0))
    B = smh.Heightmap(vision, b_data, bb, (1.0, 1.0, 70.0))
    ref = {"A": (R.color_map(a_data), ba, True), "B": (R.color_map(b_data), bb, False)}
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_HEIGHTMAP_OVERLAY

    def check(p, sl, key, ctx):
        fbs = p.slots[sl]
        recs = smh.results_to_dicts(fbs.read_results(0, N))
        uis = [fbs.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]
        cm, b, fit = ref[key]
        assert _check_overlays(fbs.read_overlay, recs, uis, cm, b, fit, ctx) == _covered_frames(N) == 1

    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=3, search=search)
        A = smh.Heightmap(vision, a_data, ba, (1.0, 1.0, 10.0))
        p.set_firing(A)
        A.close()                                               # destroyed while bound: the pipeline keeps its own reference
        s0 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        p.set_firing(B, fit_to_minimap=False)                   # s0 is in flight with A and keeps it
        s1 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        p.wait()
        check(p, s0, "A", (search, "A"))
        check(p, s1, "B", (search, "B"))
        # slot 0 again, now with B: its last reference of A goes with this rebinding
        p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        s3 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        assert s3 == s0
        p.wait()
        check(p, s3, "B", (search, "B again"))
        p.close()
    B.close()


def test_validation_enqueues_nothing(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 4
    frames, anchors = _frames_with_minimaps(N, 77)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    hm = smh.Heightmap(vision, _hm(5, 64, 48), ((0, 0), (0, 0)), (1.0, 1.0, 1.0))
    O_ = smh.STAGE_HEIGHTMAP_OVERLAY
    bad = [smh.STAGE_MARKERS | smh.STAGE_MINIMAP | O_, smh.STAGE_ALL | O_]
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    with pytest.raises(smh.VisionError) as ei:                  # no heightmap bound
        fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP | O_, anchors=anchors, stream=s)
    assert ei.value.code == smh._lib.E_INVALID
    fb.set_firing(hm)
    for st in bad:
        with pytest.raises(smh.VisionError) as ei:
            fb.run(d.data_ptr(), N, stages=st, anchors=anchors, stream=s)
        assert ei.value.code == smh._lib.E_INVALID, st
    with pytest.raises(smh.VisionError) as ei:                  # nothing was enqueued: the slab was never allocated
        fb.overlay_ptr()
    assert ei.value.code == smh._lib.E_STATE
    fb.close()
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=3, search=search)
        with pytest.raises(smh.VisionError) as ei:
            p.submit(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP | O_, anchors=anchors)
        assert ei.value.code == smh._lib.E_INVALID
        p.set_firing(hm)
        for st in bad:
            with pytest.raises(smh.VisionError) as ei:
                p.submit(d.data_ptr(), N, stages=st, anchors=anchors)
            assert ei.value.code == smh._lib.E_INVALID, (search, st)
        # the failed calls took no slot: the first good submission is slot 0
        assert p.submit(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP | O_, anchors=anchors) == 0
        p.wait()
        assert p.slots[0].overlay_ptr() != 0
        for sl in (1, 2):
            with pytest.raises(smh.VisionError):
                p.slots[sl].read_overlay(0)
        p.close()
    hm.close()
