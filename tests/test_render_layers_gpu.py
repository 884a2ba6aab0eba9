"""The map view's layers on the device (smhv_batch_render_layers / smhv_render_map_layers), byte for byte against the restatement
(tests/render_layers_ref.py), no tolerance and no excluded pixels: the identity with the calls without layers, 256 prims of both
kinds around tile borders in every form of the tap fetch, the paint order, the minimap bounds from the records' real rectangles
on a plain batch and both pipeline schedules, every map source on the batch and on the per-call path, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import firing_ref as R
import minimap_scenes as S
import render_geometry_cases as G
import render_layers_cases as LC
import render_layers_ref as LR
import render_ref as RR

pytestmark = pytest.mark.gpu

BG = G.BG
N = S.N_SCENES
FORMS = ("gather", "staged", "table")


def _set_form(name):
    from squad_mortar_helper_amd import _lib as L
    L.check(L.load().smhv_debug_render_form({"rule": L.RENDER_FORM_RULE, "gather": L.RENDER_FORM_GATHER, "staged": L.RENDER_FORM_STAGED, "table": L.RENDER_FORM_TABLE}[name]))


def _vp(view):
    import squad_mortar_helper_amd as smh
    return smh.MapViewport(view.quad, view.scale, view.top_left)


def _layers(prims=(), bounds=False, source=0):
    import squad_mortar_helper_amd as smh
    return smh.RenderLayers(prims, minimap_bounds=bounds, map_source=source)


def _want(ui, rec, view, ow, oh, prims=(), bounds=False, markers=True, cm=None, b=(0, 0), lines=None, rect=None):
    """The restatement's image: from a record, or (rec None) the per-call path's explicit lines and rectangle."""
    flags = (RR.HEIGHTMAP if cm is not None else 0) | (RR.MARKERS if markers else 0)
    is_open = True
    if rec is not None:
        is_open, rect, lines = bool(rec["map_open"]), rec["minimap"], rec["lines"]
    return LR.render(ui, is_open, rect, lines, ow, oh, view.quad, view.scale, view.top_left, flags, prims, bounds, cm, b[0], b[1], BG)


def _same(got, want, ctx):
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=2))
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d pixels differ" % len(bad), "first (y, x)", bad[:4].tolist(), "tile (x, y)", G.tile_of(x, y),
                              "got", got[y, x].tolist(), "want", want[y, x].tolist()))


def _gray(img):
    return np.dstack([img, img, img, np.full_like(img, 255)])


@pytest.fixture(scope="module")
def world(vision):
    """The scenes on the device in a plain batch that has run once with a COLOUR ui_map: records, ui_maps, the gray planes."""
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    frames, anchor_list, rects, names = S.make_scenes()
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    _, _, rw, rh = fb.roi
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    for f in range(N - 1):
        assert recs[f]["map_open"] and recs[f]["minimap"] == rects[f] and recs[f]["n_lines"] >= 1, (f, names[f])
    assert not recs[N - 1]["map_open"]
    w = dict(frames=frames, d=d, s=s, anchors=anchors, rects=rects, names=names, fb=fb, rw=rw, rh=rh, recs=recs, stages=stages,
             uis=[fb.read_image(L.IMAGE_UI_MAP, f) for f in range(N)], mask=[fb.read_image(L.VIEW_LSD_INPUT, f) for f in range(N)],
             ocr=[fb.read_image(L.VIEW_OCR_INPUT, f) for f in range(N)], scales=[fb.read_image(L.VIEW_FIND_SCALES_INPUT, f) for f in range(N)])
    data, bounds, _ = G.heightmaps()["narrow"]
    w["hm"], w["cm"], w["hb"] = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0)), R.color_map(data), bounds[0]
    yield w
    _set_form("rule")
    w["hm"].close()
    fb.close()


def _per_call(vision, world, grayscale=True):
    """Scene 0 as the current frame of the per-call path, through the whole trait sequence -> (ui_map, rectangle, lines)."""
    vision.load_frame(world["frames"][0])
    r = vision.crop_to_map(grayscale=grayscale)
    assert r is not None
    rect = vision.find_minimap()
    assert rect == world["rects"][0]
    vision.isolate_map_markers()
    vision.mask_marker_lines()
    lines = vision.find_marker_lines(15)
    assert len(lines) >= 1
    return r[0], rect, lines


def test_no_layers_is_the_render_without_layers_in_every_form(vision, world):
    """n_prims = 0, flags = 0, the ui_map as the source: the layers' kernels give smhv_batch_render's / smhv_render_map's bytes."""
    fb, s, rw, rh = (world[k] for k in ("fb", "s", "rw", "rh"))
    views = {"anisotropic": (G.matrix_views(rw, rh)["anisotropic"],) + G.WINDOW, "identity": (G.View(*RR.identity(rw, rh)), rw, rh)}
    ui, rect, lines = _per_call(vision, world)
    try:
        for vn, (view, ow, oh) in views.items():
            for form in FORMS + (None,):
                hm = world["hm"] if form is not None else None
                _set_form(form or "rule")
                fb.render(_vp(view), ow, oh, heightmap=hm, markers=True, background=BG, stream=s)
                plain = [fb.read_render(f).copy() for f in range(N)]
                fb.render(_vp(view), ow, oh, heightmap=hm, markers=True, background=BG, stream=s, layers=_layers())
                for f in range(N):
                    _same(fb.read_render(f), plain[f], (vn, form, "batch", f))
                if vn == "anisotropic":                           # ... and they are the restatement's
                    for f in (0, 3, N - 1):
                        _same(plain[f], _want(world["uis"][f], world["recs"][f], view, ow, oh, cm=world["cm"] if hm else None, b=world["hb"]), (vn, form, f))
                a = vision.render_map(_vp(view), ow, oh, lines=lines, heightmap=hm, background=BG)
                _same(vision.render_map(_vp(view), ow, oh, lines=lines, heightmap=hm, background=BG, layers=_layers()), a, (vn, form, "per call"))
    finally:
        _set_form("rule")


@pytest.mark.parametrize("view_name", ("identity", "zoom 10, far pan"))
def test_256_prims_of_both_kinds_around_tile_borders(vision, world, view_name):
    fb, s, rw, rh, recs, uis = (world[k] for k in ("fb", "s", "rw", "rh", "recs", "uis"))
    ow, oh = LC.WINDOW
    view = LC.views(rw, rh)[view_name]
    prims = LC.prim_list(view)
    masks = LC.check_prim_list(prims, view)
    ui, rect, _ = _per_call(vision, world)
    cm, hb = world["cm"], world["hb"]
    try:
        for form in FORMS + (None,):
            hm = world["hm"] if form is not None else None
            c = cm if hm else None
            _set_form(form or "rule")
            # the per-call path, no lines: the kernel's list has the prims' own order, the pairs sit at the waves' borders
            want = _want(ui, None, view, ow, oh, prims, True, False, c, hb, rect=rect)
            base = _want(ui, None, view, ow, oh, (), False, False, c, hb, rect=rect)
            assert LC.changed(want, base) >= LC.PRIMS_MIN[view_name], (view_name, LC.changed(want, base))
            for (i, j), (cx, cy) in zip(G.PAIRS, G.PAIR_CENTRES):
                assert not any(m[cy, cx] for m in masks[j + 1:]) and tuple(want[cy, cx]) == prims[j][4], (i, j)
            _same(vision.render_map(_vp(view), ow, oh, heightmap=hm, background=BG, layers=_layers(prims, True)), want, (view_name, form, "per call"))
            # a batch, the records' lines between the two classes of prims
            fb.render(_vp(view), ow, oh, heightmap=hm, markers=True, background=BG, stream=s, layers=_layers(prims, True))
            for f in range(N):
                want = _want(uis[f], recs[f], view, ow, oh, prims, True, True, c, hb)
                if f < N - 1:
                    assert LC.changed(want, _want(uis[f], recs[f], view, ow, oh, (), False, True, c, hb)) >= LC.PRIMS_MIN[view_name], (view_name, f)
                _same(fb.read_render(f), want, (view_name, form, "batch", f))
    finally:
        _set_form("rule")


def test_paint_order_where_a_below_prim_a_detected_line_and_a_foreground_prim_cross(vision, world):
    fb, s, rw, rh, recs, uis = (world[k] for k in ("fb", "s", "rw", "rh", "recs", "uis"))
    view = G.View(*RR.identity(rw, rh))
    f = 0
    lines = recs[f]["lines"]
    n = len(lines)
    x0, y0, x1, y1 = [float(v) for v in lines[n - 1]]               # the last detected line: nothing detected paints over it
    d = np.array([x1 - x0, y1 - y0])
    d /= np.hypot(*d)
    nrm = np.array([-d[1], d[0]])
    pa, pb = np.array([x0, y0]) + 0.3 * (np.array([x1, y1]) - [x0, y0]), np.array([x0, y0]) + 0.7 * (np.array([x1, y1]) - [x0, y0])
    MAG, CYAN, WHITE = (255, 0, 255, 255), (0, 255, 255, 255), (255, 255, 255, 255)
    below_a = tuple(pa - 20 * nrm) + tuple(pa + 20 * nrm) + (MAG, LR.LINE)            # crosses the detected line at pa and at pb
    below_b = tuple(pb - 20 * nrm) + tuple(pb + 20 * nrm) + (MAG, LR.LINE)
    fg = tuple(pa - 20 * nrm) + tuple(pa + 20 * nrm) + (CYAN, LR.LINE | LR.FOREGROUND)   # ... and the foreground one at pa only
    far = (5.0, 5.0, 9.0, 9.0, WHITE, LR.RECT | LR.FOREGROUND)
    prims = [fg, below_a, far, below_b]
    want = _want(uis[f], recs[f], view, rw, rh, prims)
    plain = _want(uis[f], recs[f], view, rw, rh)
    mask = lambda p: LR.prim_mask(rw, rh, p, view.scale, view.top_left)
    lm = np.zeros((rh, rw), bool)                                   # what the detected lines paint
    for ln in lines:
        lm |= RR.line_mask(rw, rh, ln, view.scale, view.top_left)
    fgm = mask(fg) | mask(far)
    all3, first2, alone = mask(below_a) & lm & mask(fg), mask(below_b) & lm & ~fgm, mask(below_b) & ~lm & ~fgm
    assert all3.sum() >= 2 and first2.sum() >= 2 and alone.sum() >= 20, (all3.sum(), first2.sum(), alone.sum())
    assert np.all(want[all3] == np.array(CYAN, np.uint8))           # all three cross: the foreground prim's colour
    assert np.array_equal(want[first2], plain[first2]) and np.all(plain[first2][:, 2] == 0)   # the first two: the detected line's (a ramp colour)
    assert np.all(want[alone] == np.array(MAG, np.uint8))
    ca = (int(pa[1]), int(pa[0]))
    assert all3[ca] and tuple(plain[ca]) == tuple(RR.line_color(n - 1, n))
    assert tuple(want[6, 6]) == tuple(plain[6, 6]) and tuple(want[5, 5]) == WHITE
    # the detected lines keep the ramp colours they have without prims, wherever no foreground prim lies
    assert (lm & ~fgm).sum() >= 100 and np.array_equal(want[lm & ~fgm], plain[lm & ~fgm])
    fb.render(_vp(view), rw, rh, markers=True, background=BG, stream=s, layers=_layers(prims), first=f, n=1)
    _same(fb.read_render(f), want, "batch")
    ui, rect, _ = _per_call(vision, world, grayscale=False)
    assert np.array_equal(ui, uis[f])
    _same(vision.render_map(_vp(view), rw, rh, lines=lines, background=BG, layers=_layers(prims)), want, "per call")


def test_minimap_bounds_from_the_records_rectangles_on_a_batch_and_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    fb, d, s, anchors, rw, rh, recs, uis, names = (world[k] for k in ("fb", "d", "s", "anchors", "rw", "rh", "recs", "uis", "names"))
    views = {"identity": (G.View(*RR.identity(rw, rh)), rw, rh), "anisotropic": (G.matrix_views(rw, rh)["anisotropic"],) + G.WINDOW}
    # the scenes' rectangles: generic, at the ROI's own edges, 17 px narrow, 13 px flat
    widths = [r[1] - r[0] for r in world["rects"][:N - 1]]
    heights = [r[3] - r[2] for r in world["rects"][:N - 1]]
    assert min(widths) == 17 and min(heights) == 13 and world["rects"][6] == (0, rw - 1, 0, rh - 1)
    wants = {}
    for vn, (view, ow, oh) in views.items():
        wants[vn] = [_want(uis[f], recs[f], view, ow, oh, (), True) for f in range(N)]
        for f in range(N - 1):
            G.assert_changes(wants[vn][f], _want(uis[f], recs[f], view, ow, oh), LC.BOUNDS_MIN[vn][f], (vn, f, names[f]))
        assert np.all(wants[vn][N - 1] == np.array(BG, np.uint8))

    def check(b, stream, ctx):
        for vn, (view, ow, oh) in views.items():
            b.render(_vp(view), ow, oh, markers=True, background=BG, stream=stream, layers=_layers((), True))
            for f in range(N):
                _same(b.read_render(f), wants[vn][f], (ctx, vn, "frame %d (%s)" % (f, names[f])))
    check(fb, s, "plain batch")
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, N, depth=3, search=search)
        slot = p.submit(d.data_ptr(), N, stages=world["stages"], grayscale=False, anchors=anchors)
        p.wait()
        check(p.slots[slot], p.stream_of(slot), search)
        p.close()
    # no rectangle (a run without the minimap stage): nothing is drawn
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=smh.STAGE_ALL, grayscale=False, anchors=anchors, stream=s)
    recs2 = smh.results_to_dicts(fb2.read_results(0, N))
    assert all(r["minimap"] is None for r in recs2)
    view, ow, oh = views["anisotropic"]
    fb2.render(_vp(view), ow, oh, markers=True, background=BG, stream=s, layers=_layers((), True))
    for f in (0, 3, 4, N - 1):
        want = _want(uis[f], recs2[f], view, ow, oh, (), True)
        assert np.array_equal(want, _want(uis[f], recs2[f], view, ow, oh))
        _same(fb2.read_render(f), want, ("no rectangle", f))
    fb2.close()


def _source_images(world, f):
    """The five views of frame f as the header defines them for a batch -> {VIEW_*: uint8 [h, w, 4]}."""
    from squad_mortar_helper_amd import _lib as L
    ui = world["uis"][f]
    rh, rw = ui.shape[:2]
    iso = ui.copy()
    iso[~LC.marker_predicate(ui[..., 0], ui[..., 1], ui[..., 2])] = (0, 0, 0, 255)
    return {L.VIEW_OCR_INPUT: _gray(world["ocr"][f]), L.VIEW_FIND_SCALES_INPUT: _gray(world["scales"][f]), L.VIEW_LSD_INPUT: _gray(world["mask"][f]),
            L.VIEW_LSD_PREPROCESS: iso, L.VIEW_CROPPED_BRQ: ui[rh // 2:rh // 2 + rh // 2, rw // 2:rw // 2 + rw // 2].copy()}


def test_every_map_source_on_a_batch(vision, world):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    fb, d, s, anchors, rw, rh, recs, uis = (world[k] for k in ("fb", "d", "s", "anchors", "rw", "rh", "recs", "uis"))
    imgs = [_source_images(world, f) for f in range(N)]
    assert imgs[0][L.VIEW_OCR_INPUT].shape == (rh // 2, rw // 2, 4) and (fb.layout.brq_w, fb.layout.brq_h) == (rw // 2, rh // 2)
    zoomed = G.View.calc(*LC.WINDOW, rw, rh, 3, (0.4, 0.6), (30.0, -12.0))
    prims = LC.prim_list(G.View(*RR.identity(rw, rh)))[:40]
    for src in (L.VIEW_OCR_INPUT, L.VIEW_FIND_SCALES_INPUT, L.VIEW_LSD_PREPROCESS, L.VIEW_LSD_INPUT, L.VIEW_CROPPED_BRQ):
        h, w = imgs[0][src].shape[:2]
        ident = G.View(*RR.identity(w, h))
        # at the identity viewport of its own size the image is the view
        fb.render(_vp(ident), w, h, background=BG, stream=s, layers=_layers(source=src))
        for f in range(N - 1):
            _same(fb.read_render(f), imgs[f][src], (src, "identity", f))
            assert np.array_equal(_want(imgs[f][src], recs[f], ident, w, h, markers=False), imgs[f][src])
            base = _want(uis[f], recs[f], ident, w, h, markers=False)
            assert LC.changed(imgs[f][src], base) >= LC.SOURCE_MIN[src], (src, f, LC.changed(imgs[f][src], base))
        assert np.all(fb.read_render(N - 1) == np.array(BG, np.uint8))
        # through a zoomed, panned viewport with the heightmap, the markers, prims and the bounds on top, in the table form and the gathers
        ow, oh = LC.WINDOW
        for hm in (world["hm"], None):
            fb.render(_vp(zoomed), ow, oh, heightmap=hm, markers=True, background=BG, stream=s, layers=_layers(prims, True, src))
            for f in (0, 3, 4, N - 1):
                want = _want(imgs[f][src], recs[f], zoomed, ow, oh, prims, True, True, world["cm"] if hm else None, world["hb"])
                _same(fb.read_render(f), want, (src, "zoomed", hm is not None, f))
    # a run that did not produce the source refuses it; nothing is enqueued: the slab keeps the previous image
    view, ow, oh = G.View(*RR.identity(rw, rh)), rw, rh
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=smh.STAGE_UI_MAP | smh.STAGE_MINIMAP, grayscale=True, anchors=None, stream=s)
    fb2.render(_vp(view), ow, oh, background=BG, stream=s, layers=_layers())
    before = fb2.read_render(0).copy()
    for src in (L.VIEW_LSD_PREPROCESS, L.VIEW_CROPPED_BRQ, L.VIEW_OCR_INPUT, L.VIEW_FIND_SCALES_INPUT, L.VIEW_LSD_INPUT):
        with pytest.raises(smh.VisionError) as ei:                # a grayscale ui_map, and no OCR / SCALES / MARKERS stage
            fb2.render(_vp(view), ow, oh, background=BG, stream=s, layers=_layers(source=src))
        assert ei.value.code == L.E_STATE, src
    assert np.array_equal(fb2.read_render(0), before)
    # scales without anchors are not produced either; a colour run with the stages makes all five available
    fb2.run(d.data_ptr(), N, stages=smh.STAGE_ALL, grayscale=False, anchors=None, stream=s)
    with pytest.raises(smh.VisionError) as ei:
        fb2.render(_vp(view), ow, oh, background=BG, stream=s, layers=_layers(source=L.VIEW_FIND_SCALES_INPUT))
    assert ei.value.code == L.E_STATE
    fb2.render(_vp(view), ow, oh, background=BG, stream=s, layers=_layers(source=L.VIEW_LSD_PREPROCESS))
    _same(fb2.read_render(2), imgs[2][L.VIEW_LSD_PREPROCESS], "after the colour run")
    fb2.close()


def test_every_map_source_on_the_per_call_path(vision, world):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    for grayscale in (True, False):
        ui, rect, lines = _per_call(vision, world, grayscale)
        vision.ocr_preprocess()
        for src in (L.VIEW_OCR_INPUT, L.VIEW_FIND_SCALES_INPUT, L.VIEW_LSD_PREPROCESS, L.VIEW_LSD_INPUT, L.VIEW_CROPPED_BRQ):
            view_img = vision.get_debug_view(src)
            h, w = view_img.shape[:2]
            ident = G.View(*RR.identity(w, h))
            got = vision.render_map(_vp(ident), w, h, background=BG, layers=_layers(source=src))
            _same(got, view_img, (grayscale, src, "identity"))
            assert LC.changed(view_img, _want(ui, None, ident, w, h, markers=False)) >= LC.SOURCE_MIN[src], (grayscale, src)
            ow, oh = LC.WINDOW
            zoomed = G.View.calc(ow, oh, world["rw"], world["rh"], 3, (0.4, 0.6), (30.0, -12.0))
            got = vision.render_map(_vp(zoomed), ow, oh, lines=lines, background=BG, layers=_layers((), True, src))
            _same(got, _want(view_img, None, zoomed, ow, oh, (), True, True, lines=lines, rect=rect), (grayscale, src, "zoomed"))


def test_argument_errors_enqueue_nothing(vision, world):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s, rw, rh = (world[k] for k in ("fb", "s", "rw", "rh"))
    view = G.matrix_views(rw, rh)["anisotropic"]
    ow, oh = G.WINDOW
    opt = smh.render_options(_vp(view), ow, oh, markers=True, background=BG)
    fb.render(_vp(view), ow, oh, markers=True, background=BG, stream=s, layers=_layers((), True))
    before = [fb.read_render(f).copy() for f in range(N)]
    ok = (10.0, 10.0, 90.0, 40.0, (1, 2, 3, 255), L.PRIM_RECT)

    def layers(prims=(ok,), **kw):
        ly, keep = _layers(list(prims)).struct()
        for k, v in kw.items():
            setattr(ly, k, v)
        return ly, keep
    bad = [layers(size=20), layers(size=32), layers(flags=2), layers(flags=0x80000001), layers(map_source=6), layers(map_source=100),
           layers(n_prims=257), layers([(0, 0, 1, 1, (1, 2, 3, 255), 2)]), layers([(0, 0, 1, 1, (1, 2, 3, 255), 0x400)]),
           layers([ok, (0, 0, 1, 1, (1, 2, 3, 255), 0x10001)]), layers([ok, ok, (0, 0, 1, 1, (1, 2, 3, 254), 0)]), layers([(0, 0, 1, 1, (1, 2, 3, 0), 1)])]
    ly, keep = layers()
    ly.prims = None                                                 # n_prims != 0 with prims == NULL
    bad.append((ly, keep))
    many, _ = _layers([ok] * 257).struct()
    bad.append((many, _))
    for i, (ly, keep) in enumerate(bad):
        assert lib.smhv_batch_render_layers(fb._b, 0, N, None, C.byref(opt), C.byref(ly), s) == L.E_INVALID, i
    assert lib.smhv_batch_render_layers(fb._b, 0, N, None, C.byref(opt), None, s) == L.E_INVALID
    # ... and the siblings' own errors
    ly, keep = layers()
    assert lib.smhv_batch_render_layers(fb._b, 1, N, None, C.byref(opt), C.byref(ly), s) == L.E_INVALID
    assert lib.smhv_batch_render_layers(fb._b, 0, N, None, None, C.byref(ly), s) == L.E_INVALID
    o2 = smh.render_options(_vp(view), ow, oh, heightmap=True)
    assert lib.smhv_batch_render_layers(fb._b, 0, N, None, C.byref(o2), C.byref(ly), s) == L.E_INVALID
    for f in range(N):
        assert np.array_equal(fb.read_render(f), before[f]), f
    assert fb.render_size() == (ow, oh)
    # the per-call path: the same checks, and the explicit lines' limit
    ui, rect, lines = _per_call(vision, world)
    out = np.zeros((oh, ow, 4), np.uint8)
    for i, (ly, keep) in enumerate(bad):
        assert lib.smhv_render_map_layers(vision._ctx, None, C.byref(opt), C.byref(ly), None, 0, out.ctypes.data) == L.E_INVALID, i
    assert lib.smhv_render_map_layers(vision._ctx, None, C.byref(opt), None, None, 0, out.ctypes.data) == L.E_INVALID
    assert not out.any()
    with pytest.raises(smh.VisionError) as ei:
        vision.render_map(_vp(view), ow, oh, lines=np.zeros((257, 4), np.float32), layers=_layers())
    assert ei.value.code == L.E_INVALID
    # a correct call follows
    ly, keep = layers()
    assert lib.smhv_batch_render_layers(fb._b, 0, N, None, C.byref(opt), C.byref(ly), s) == 0
    _same(fb.read_render(0), _want(world["uis"][0], world["recs"][0], view, ow, oh, [ok]), "after the failed calls")
    # a closed map is SMHV_E_STATE on the per-call path, as for smhv_render_map
    vision.load_frame(world["frames"][N - 1])
    assert vision.crop_to_map() is None
    with pytest.raises(smh.VisionError) as ei:
        vision.render_map(_vp(view), ow, oh, layers=_layers())
    assert ei.value.code == L.E_STATE
