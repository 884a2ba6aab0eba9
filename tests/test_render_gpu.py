"""The map view on the device, byte for byte against the restatement (tests/render_ref.py), no tolerance and no excluded pixels:
the per-call path on the golden fixtures, smhv_batch_render on a batch and on the slots of both pipeline schedules, every form of
the overlay's tap fetch forced, the validation, and the heightmap's lifetime."""
import numpy as np
import pytest

import firing_ref as R
import render_ref as RR
from fixtures import OPEN_STEMS, load_fixture
from test_firing_gpu import _frames_with_minimaps

pytestmark = pytest.mark.gpu

BG = (12, 34, 56, 255)
WINDOWS = ((1280, 720), (2560, 1440), (640, 360))


def _hm(seed, side, lo=0, hi=65536, height=None):
    return np.random.default_rng(seed).integers(lo, hi, size=(side if height is None else height, side), dtype=np.uint16)


HM_SMALL = (lambda: (_hm(31, 1024, height=640), ((-15, 9), (0, 0))))   # not square: 1024 wide, 640 high
HM_LARGE = (lambda: (_hm(32, 4096, 100, 60000), ((37, -21), (0, 0))))


def _vp_tuple(vp):
    return vp.quad, (vp.scale_factor_w, vp.scale_factor_h), vp.top_left


def _want(ui, map_open, minimap, lines, vp, out_w, out_h, heightmap, markers, fit, cm=None, bounds=None):
    quad, scale, tl = _vp_tuple(vp)
    flags = (RR.HEIGHTMAP if heightmap else 0) | (RR.MARKERS if markers else 0) | (0 if fit else RR.BOUNDS_OFFSET)
    b = bounds[0] if bounds is not None else (0, 0)
    return RR.render(ui, map_open, minimap, lines, out_w, out_h, quad, scale, tl, flags, cm, b[0], b[1], BG)


def _same(got, want, ctx):
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=2))
        raise AssertionError((ctx, len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist()))


def test_per_call_path_on_the_golden_fixtures(vision):
    import squad_mortar_helper_amd as smh
    maps = []
    for data, bounds in (HM_SMALL(), HM_LARGE()):
        maps.append((smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0)), R.color_map(data), bounds))
    checked = overlays = with_lines = 0
    for stem in OPEN_STEMS:
        frame, _, _ = load_fixture(stem)
        vision.load_frame(frame)
        r = vision.crop_to_map(grayscale=True)
        assert r is not None, stem
        ui = r[0]
        rect = vision.find_minimap()
        vision.isolate_map_markers()
        vision.mask_marker_lines()
        lines = vision.find_marker_lines(15)
        with_lines += len(lines) > 0
        h, w = ui.shape[:2]
        for (ow, oh) in WINDOWS:
            vp = smh.MapViewport.calc(ow, oh, w, h)
            got = vision.render_map(vp, ow, oh, lines=lines, background=BG)
            _same(got, _want(ui, True, rect, lines, vp, ow, oh, False, len(lines) > 0, True), (stem, ow, oh, "no heightmap"))
            checked += 1
            for k, (hm, cm, b) in enumerate(maps):
                for fit in (True, False):
                    got = vision.render_map(vp, ow, oh, lines=lines, heightmap=hm, fit_to_minimap=fit, background=BG)
                    want = _want(ui, True, rect, lines, vp, ow, oh, True, len(lines) > 0, fit, cm, b)
                    _same(got, want, (stem, ow, oh, k, fit))
                    checked += 1
                    overlays += rect is not None
        # the call changes nothing of what the trait path hands out
        assert vision.find_minimap() == rect and np.array_equal(vision.ui_map(copy=True), ui), stem
    assert checked == len(OPEN_STEMS) * 15 and overlays >= 60 and with_lines >= 10, (checked, overlays, with_lines)
    # more explicit lines than a record holds, through a zoomed viewport
    rng = np.random.default_rng(4)
    many = rng.uniform(-40.0, 900.0, size=(200, 4)).astype(np.float32)
    many[17] = many[18][[2, 3, 2, 3]]                              # a line of zero length
    vp = smh.MapViewport.calc(1280, 720, w, h, 3, (0.4, 0.6), (30.0, -12.0))
    got = vision.render_map(vp, 1280, 720, lines=many, heightmap=maps[0][0], background=BG)
    _same(got, _want(ui, True, rect, many, vp, 1280, 720, True, True, True, maps[0][1], maps[0][2]), "200 explicit lines")
    with pytest.raises(smh.VisionError) as ei:
        vision.render_map(vp, 1280, 720, lines=np.zeros((257, 4), np.float32))
    assert ei.value.code == smh._lib.E_INVALID
    # errors follow the trait path: a closed map is SMHV_E_STATE
    frame, _, _ = load_fixture("a_point_png")
    vision.load_frame(frame)
    assert vision.crop_to_map() is None
    with pytest.raises(smh.VisionError) as ei:
        vision.render_map(vp, 1280, 720)
    assert ei.value.code == smh._lib.E_STATE
    for hm, _, _ in maps:
        hm.close()


def _batch_frames(N, first_idx):
    """_frames_with_minimaps with frame 7 replaced by a scene of 36 marker lines (the search returns its maximum, 32)."""
    from squad_mortar_helper_amd import synth
    frames, anchors = _frames_with_minimaps(N, first_idx)
    frames[7], _ = synth.make_frame(1920, 1080, frame_idx=5000, n_lines=36)
    return frames, anchors


def _state(fb, N):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    return (bytes(fb.read_results(0, N)),
            [bytes(fb.read_image(w, f).tobytes()) for f in range(N) for w in (L.IMAGE_UI_MAP, L.VIEW_LSD_INPUT, L.VIEW_OCR_INPUT, L.IMAGE_HEIGHTMAP_OVERLAY)])


def _check_batch(fb, recs, uis, vp, ow, oh, heightmap, markers, fit, cm, bounds, ctx, frames=None):
    for f in (range(len(recs)) if frames is None else frames):
        rec = recs[f]
        want = _want(uis[f], bool(rec["map_open"]), rec["minimap"], rec["lines"], vp, ow, oh, heightmap, markers, fit, cm, bounds)
        _same(fb.read_render(f), want, (ctx, f))


def test_batch_render_identities_viewports_and_both_forms(vision):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    N = 12
    frames, anchors = _batch_frames(N, 500)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    (da, ba), (db, bb) = HM_SMALL(), HM_LARGE()
    A, B = smh.Heightmap(vision, da, ba, (1.0, 1.0, 30.0)), smh.Heightmap(vision, db, bb, (1.0, 1.0, 30.0))
    cma, cmb = R.color_map(da), R.color_map(db)
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    _, _, rw, rh = fb.roi
    ident = smh.MapViewport.identity(rw, rh)
    with pytest.raises(smh.VisionError) as ei:                    # no ui_map yet
        fb.render(ident, rw, rh, stream=s)
    assert ei.value.code == L.E_STATE
    with pytest.raises(smh.VisionError) as ei:
        fb.render_ptr()
    assert ei.value.code == L.E_STATE
    fb.set_firing(A, fit_to_minimap=False)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_HEIGHTMAP_OVERLAY, anchors=anchors, stream=s)
    before = _state(fb, N)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    assert not recs[N - 1]["map_open"] and all(r["map_open"] for r in recs[:N - 1])
    assert recs[7]["n_lines"] == 32 and sum(r["minimap"] is not None for r in recs) >= 8
    uis = [fb.read_image(L.IMAGE_UI_MAP, f) for f in range(N)]

    # ---- the two identities ----
    fb.render(ident, rw, rh, background=BG, stream=s)
    for f in range(N - 1):
        assert np.array_equal(fb.read_render(f), uis[f]), f
    assert np.all(fb.read_render(N - 1) == np.array(BG, np.uint8)), "a closed frame is background"
    ptr, stride = fb.render_ptr()
    assert ptr != 0 and stride == rw * rh * 4
    fb.render(ident, rw, rh, heightmap=A, fit_to_minimap=False, background=BG, stream=s)
    covered = 0
    for f in range(N - 1):
        got = fb.read_render(f)
        assert np.array_equal(got, fb.read_overlay(f)), f
        covered += int(np.any(got != uis[f]))
    assert covered >= 2, covered
    assert np.all(fb.read_render(N - 1) == np.array(BG, np.uint8))

    # ---- viewports: zoomed and panned (the quad partly outside the window, up to 5x), a tiny window, an odd width ----
    views = [(1280, 720, 3, (0.4, 0.6), (30.0, -12.0)), (1280, 720, 10, (0.55, 0.35), (-200.0, 150.0)), (50, 40, 0, (0.0, 0.0), (0.0, 0.0)),
             (641, 361, 1, (0.2, 0.9), (5.0, 5.0))]
    for vi, (ow, oh, zoom, zp, pp) in enumerate(views):
        vp = smh.MapViewport.calc(ow, oh, rw, rh, zoom, zp, pp)
        hm, cm, b = (A, cma, ba) if vi % 2 == 0 else (B, cmb, bb)
        fit = vi < 2
        fb.render(vp, ow, oh, heightmap=hm, markers=True, fit_to_minimap=fit, background=BG, stream=s)
        _check_batch(fb, recs, uis, vp, ow, oh, True, True, fit, cm, b, ("view", vi))
        assert fb.render_ptr()[1] == ow * oh * 4
    # a sub-range: frames [5, 9) only; the others keep the previous render's bytes (the slab holds the whole batch)
    vp = smh.MapViewport.calc(640, 360, rw, rh)
    fb.render(vp, 640, 360, markers=True, background=BG, stream=s)
    keep = [fb.read_render(f).copy() for f in range(N)]
    fb.render(vp, 640, 360, first=5, n=4, heightmap=A, markers=True, background=BG, stream=s)
    _check_batch(fb, recs, uis, vp, 640, 360, True, True, True, cma, ba, "sub-range", frames=range(5, 9))
    for f in list(range(5)) + list(range(9, N)):
        assert np.array_equal(fb.read_render(f), keep[f]), f

    # ---- each form of the overlay's tap fetch forced ----
    try:
        for (hm, cm, b, name) in ((A, cma, ba, "1024"), (B, cmb, bb, "4096")):
            for (ow, oh) in ((640, 360), (2560, 1440)):
                vp = smh.MapViewport.calc(ow, oh, rw, rh)
                want = {f: _want(uis[f], bool(recs[f]["map_open"]), recs[f]["minimap"], recs[f]["lines"], vp, ow, oh, True, True, False, cm, b) for f in (2, 3, 7, N - 1)}
                for form in (L.RENDER_FORM_GATHER, L.RENDER_FORM_STAGED, L.RENDER_FORM_TABLE):
                    L.check(L.load().smhv_debug_render_form(form))
                    fb.render(vp, ow, oh, heightmap=hm, markers=True, fit_to_minimap=False, background=BG, stream=s)
                    for f, w in want.items():
                        _same(fb.read_render(f), w, ("form", form, name, ow, oh, f))
    finally:
        L.check(L.load().smhv_debug_render_form(L.RENDER_FORM_RULE))

    # ---- rendering leaves every other output of the batch alone ----
    assert _state(fb, N) == before
    # ---- a run without the minimap stage: no frame has a rectangle, no overlay is drawn ----
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL, anchors=anchors, stream=s)
    recs2 = smh.results_to_dicts(fb.read_results(0, N))
    assert all(r["minimap"] is None for r in recs2)
    vp = smh.MapViewport.calc(1280, 720, rw, rh, 3, (0.4, 0.6), (30.0, -12.0))
    fb.render(vp, 1280, 720, heightmap=B, markers=True, background=BG, stream=s)
    _check_batch(fb, recs2, uis, vp, 1280, 720, True, True, True, cmb, bb, "no rectangle", frames=(0, 3, 7, N - 1))
    fb.close()
    A.close()
    B.close()


def test_render_on_the_slots_of_both_pipeline_schedules(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 8
    frames, anchors = _batch_frames(N, 900)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    data, bounds = HM_SMALL()
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 30.0))
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    _, _, rw, rh = fb.roi
    small = smh.MapViewport.calc(640, 360, rw, rh)
    big = smh.MapViewport.calc(1280, 720, rw, rh, 3, (0.4, 0.6), (30.0, -12.0))
    fb.run(d.data_ptr(), N, stages=stages, anchors=anchors, stream=s)
    recs = bytes(fb.read_results(0, N))
    fb.render(small, 640, 360, heightmap=hm, markers=True, background=BG, stream=s)
    want_small = [fb.read_render(f).tobytes() for f in range(N)]
    fb.render(big, 1280, 720, heightmap=hm, markers=True, background=BG, stream=s)         # a larger slab: re-allocated
    want_big = [fb.read_render(f).tobytes() for f in range(N)]
    rd = smh.results_to_dicts(fb.read_results(0, N))
    uis = [fb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]
    _check_batch(fb, rd, uis, big, 1280, 720, True, True, True, R.color_map(data), bounds, "plain batch")
    fb.close()
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=6, search=search)
        slots = [p.submit(d.data_ptr(), N, stages=stages, anchors=anchors) for _ in range(7)]
        p.wait()
        for sl in sorted(set(slots)):
            sb = p.slots[sl]
            st = p.stream_of(sl)
            assert bytes(sb.read_results(0, N)) == recs, (search, sl)
            # two renders with different windows back to back on the slot's stream
            sb.render(small, 640, 360, heightmap=hm, markers=True, background=BG, stream=st)
            sb.render(big, 1280, 720, heightmap=hm, markers=True, background=BG, stream=st)
            assert [sb.read_render(f).tobytes() for f in range(N)] == want_big, (search, sl)
            sb.render(small, 640, 360, heightmap=hm, markers=True, background=BG, stream=st)
            assert [sb.read_render(f).tobytes() for f in range(N)] == want_small, (search, sl)
            assert bytes(sb.read_results(0, N)) == recs, (search, sl)
        # the pipeline goes on after its slots were rendered
        assert p.submit(d.data_ptr(), N, stages=stages, anchors=anchors) == slots[1]
        p.wait()
        p.close()
    hm.close()


def test_validation_enqueues_nothing_and_a_correct_call_follows(vision):
    import ctypes as C
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    N = 4
    frames, anchors = _frames_with_minimaps(N, 77)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    hm = smh.Heightmap(vision, _hm(5, 64), ((0, 0), (0, 0)), (1.0, 1.0, 1.0))
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    _, _, rw, rh = fb.roi
    vp = smh.MapViewport.identity(rw, rh)
    lib = L.load()

    def call(opt, first=0, n=N, h=None):
        return lib.smhv_batch_render(fb._b, first, n, h._hm if h is not None else None, C.byref(opt) if opt is not None else None, s)

    good = smh.render_options(vp, 320, 200, background=BG)
    assert call(good) == L.E_STATE                                # the batch has never produced a ui_map
    fb.run(d.data_ptr(), N, stages=smh.STAGE_MARKERS, anchors=None, stream=s)
    assert call(good) == L.E_STATE                                # ... still not: the run had no SMHV_STAGE_UI_MAP
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, anchors=anchors, stream=s)
    bad = []
    for w, h in ((0, 200), (320, 0)):
        bad.append((smh.render_options(vp, w, h), 0, N, None))
    o = smh.render_options(vp, 320, 200)
    o.size = 48
    bad.append((o, 0, N, None))
    o = smh.render_options(vp, 320, 200)
    o.flags = 8
    bad.append((o, 0, N, None))
    bad.append((good, 1, N, None))                                # first + n beyond the capacity
    bad.append((good, N, 1, None))
    bad.append((good, 0, 0, None))
    bad.append((smh.render_options(vp, 320, 200, heightmap=True), 0, N, None))   # SMHV_RENDER_HEIGHTMAP without hm
    bad.append((None, 0, N, None))
    for i, v in ((0, float("-inf")), (2, float("nan")), (3, float("inf"))):   # a quad edge that is not finite
        o = smh.render_options(vp, 320, 200)
        o.quad[i] = v
        bad.append((o, 0, N, None))
    for opt, first, n, h in bad:
        assert call(opt, first, n, h) == L.E_INVALID, (first, n)
    for q in (fb.render_ptr, fb.render_size, lambda: fb.read_render(0)):   # nothing was enqueued or allocated
        with pytest.raises(smh.VisionError) as ei:
            q()
        assert ei.value.code == L.E_STATE
    assert call(good) == 0
    recs = smh.results_to_dicts(fb.read_results(0, N))
    uis = [fb.read_image(L.IMAGE_UI_MAP, f) for f in range(N)]
    assert fb.render_size() == (320, 200)
    _check_batch(fb, recs, uis, vp, 320, 200, False, False, True, None, None, "after the failed calls")
    assert call(smh.render_options(vp, 320, 200, heightmap=True, background=BG), h=hm) == 0
    assert lib.smhv_batch_read_render(fb._b, N, np.empty(4, np.uint8).ctypes.data) == L.E_INVALID
    fb.close()
    hm.close()


def test_destroying_the_heightmap_right_after_enqueueing_a_render_is_safe(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 8
    frames, anchors = _frames_with_minimaps(N, 1300)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    _, _, rw, rh = fb.roi
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    uis = [fb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]
    vp = smh.MapViewport.calc(1280, 720, rw, rh)
    for seed, side, bounds in ((41, 700, ((3, -2), (0, 0))), (42, 1500, ((-50, 11), (0, 0)))):
        data = _hm(seed, side)
        hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 10.0))
        fb.render(vp, 1280, 720, heightmap=hm, markers=True, fit_to_minimap=False, background=BG, stream=s)
        hm.close()                                                # the batch keeps its own reference while the render is enqueued
        _check_batch(fb, recs, uis, vp, 1280, 720, True, True, False, R.color_map(data), bounds, ("destroyed", seed))
    fb.close()
