"""The map view, the overlay stage and the firing solutions on the device where their inputs' geometry is not the easy one, byte
for byte against the restatements (tests/render_ref.py, tests/overlay_ref.py, tests/firing_ref.py; no tolerance, no excluded
pixels -- the firing bearings keep _check_line's one-ulp atan2f allowance): batches whose minimap rectangles are proper parts of
the ROI (tests/minimap_scenes.py) on a plain batch and both pipeline schedules, heightmaps that are not square, tiny, flat or of a
narrow value range in every form of the tap fetch, windows at the tile's edges, and 256 explicit lines around tile borders, across
wave boundaries of the line compaction, at coordinates of 1e4 and with end points that are not finite."""
import ctypes as C

import numpy as np
import pytest

import firing_ref as R
import minimap_scenes as S
import overlay_ref as O
import render_geometry_cases as G
import render_ref as RR
from test_firing_gpu import _check_slab

pytestmark = pytest.mark.gpu

BG = G.BG
N = S.N_SCENES
FORMS = ("rule", "gather", "staged", "table")


def _form_code(name):
    from squad_mortar_helper_amd import _lib as L
    return {"rule": L.RENDER_FORM_RULE, "gather": L.RENDER_FORM_GATHER, "staged": L.RENDER_FORM_STAGED, "table": L.RENDER_FORM_TABLE}[name]


def _set_form(name):
    from squad_mortar_helper_amd import _lib as L
    L.check(L.load().smhv_debug_render_form(_form_code(name)))


def _rule(rw, rh, view, W, H):
    """(LDS texels of the staged form, the form the rule takes) for a heightmap of W x H through `view`."""
    from squad_mortar_helper_amd import _lib as L
    tx, fm = C.c_uint32(), C.c_uint32()
    L.check(L.load().smhv_debug_render_rule(rw, rh, float(view.scale[0]), float(view.scale[1]), W, H, None, None, C.byref(tx), C.byref(fm)))
    return tx.value, fm.value


def _vp(view):
    import squad_mortar_helper_amd as smh
    return smh.MapViewport(view.quad, view.scale, view.top_left)


def _want(ui, rec, view, ow, oh, cm=None, b=(0, 0), fit=True, markers=True, lines=None, rect="record"):
    flags = (RR.HEIGHTMAP if cm is not None else 0) | (RR.MARKERS if markers else 0) | (0 if fit else RR.BOUNDS_OFFSET)
    if rec is not None:
        is_open, rect, lines = bool(rec["map_open"]), rec["minimap"], rec["lines"]
    else:
        is_open = True
    return RR.render(ui, is_open, rect, lines, ow, oh, view.quad, view.scale, view.top_left, flags, cm, b[0], b[1], BG)


def _same(got, want, ctx):
    """ctx names the case (heightmap, view, form, frame ...); the failure adds the first differing pixels (y, x) and the tile of
    the first."""
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=2))
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d pixels differ" % len(bad), "first (y, x)", bad[:4].tolist(), "tile (x, y)", G.tile_of(x, y),
                              "got", got[y, x].tolist(), "want", want[y, x].tolist()))


@pytest.fixture(scope="module")
def world(vision):
    """The scenes on the device in a plain batch that has run once: records, ui_maps, and the restatement's renders without a
    heightmap that the cases share."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, anchor_list, rects, names = S.make_scenes()
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    _, _, rw, rh = fb.roi
    assert (rw, rh) == tuple(S.roi()[2:])
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    uis = [fb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]
    # the records' rectangles are the designed ones; the last frame is closed; every open frame has lines
    for f in range(N - 1):
        assert recs[f]["map_open"] and recs[f]["minimap"] == rects[f] and recs[f]["n_lines"] >= 1, (f, names[f], recs[f]["minimap"], rects[f])
        assert (recs[f]["mpx"] is None) == (f == S.NO_ANCHORS), (f, names[f])
    assert not recs[N - 1]["map_open"]
    w = dict(frames=frames, d=d, s=s, anchors=anchors, rects=rects, names=names, fb=fb, rw=rw, rh=rh, recs=recs, uis=uis, base={})
    ow, oh = G.WINDOW
    for vn, view in G.matrix_views(rw, rh).items():
        w["base"][vn] = [_want(uis[f], recs[f], view, ow, oh) for f in range(N)]
    yield w
    fb.close()


def test_batch_with_real_rectangles_on_a_plain_batch_and_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    fb, d, s, anchors, rects, names, uis, rw, rh = (world[k] for k in ("fb", "d", "s", "anchors", "rects", "names", "uis", "rw", "rh"))
    ow, oh = G.WINDOW
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_FIRING | smh.STAGE_HEIGHTMAP_OVERLAY
    rng = np.random.default_rng(77)
    # bounds of both signs on both axes: -15 / 49 and 12 / 92 of the rectangle's width, 9 / 57 and -7 / 43 of its height
    maps = {"A": (rng.integers(0, 65536, size=(48, 64), dtype=np.uint16), ((-15, 9), (0, 0)), (1.0, 1.0, 30.0)),
            "B": (rng.integers(0, 65536, size=(50, 80), dtype=np.uint16), ((12, -7), (0, 0)), (1.0, 1.0, 30.0))}
    hms = {k: smh.Heightmap(vision, *v) for k, v in maps.items()}
    cms = {k: R.color_map(v[0]) for k, v in maps.items()}
    views = {"anisotropic": G.matrix_views(rw, rh)["anisotropic"], "zoom 3": G.View.calc(ow, oh, rw, rh, 3, (0.4, 0.6), (30.0, -12.0))}
    # at zoom 3 the map is 91 x 147 px in a window 67 px high: the narrow scene's rectangle is 4 px wide there
    view_min = {"anisotropic": G.MATRIX_MIN["anisotropic"], "zoom 3": (200,) * (N - 1)}
    configs = (("A", True), ("A", False), ("B", False))
    verified = {}

    def check(b, key, fit, stream, ctx):
        """Everything of one run against the restatements -> (record bytes, overlay bytes)."""
        data, bounds, scale = maps[key]
        raw = b.read_results(0, N)
        recs = smh.results_to_dicts(raw)
        for f in range(N - 1):
            assert recs[f]["minimap"] == rects[f], (ctx, f, names[f], recs[f]["minimap"], rects[f])
        nl, slab = b.read_firing(0, N)
        seen = _check_slab(recs, nl, slab, maps[key], fit, tuple(float(v) for v in view.scale + view.top_left), ctx)
        assert seen == {R.NONE, R.SCALES, R.HEIGHTMAP}, (ctx, seen)
        ovl = []
        for f in range(N - 1):
            got = b.read_overlay(f)
            want = O.overlay(uis[f], recs[f]["minimap"], cms[key], bounds[0][0], bounds[0][1], fit)
            assert np.array_equal(got, want), (ctx, "overlay", f, names[f], np.argwhere(np.any(got != want, axis=2))[:4].tolist())
            # the flat scene's rectangle, the smallest, is 318 x 13 px, and an offset takes at most a sixth of it
            assert G.changed(want, uis[f]) >= 3000, (ctx, f)
            ovl.append(got.tobytes())
        for vn, v in views.items():
            b.render(_vp(v), ow, oh, heightmap=hms[key], markers=True, fit_to_minimap=fit, background=BG, stream=stream)
            for f in range(N):
                want = _want(uis[f], recs[f], v, ow, oh, cms[key], bounds[0], fit)
                if f < N - 1:
                    G.assert_changes(want, _want(uis[f], recs[f], v, ow, oh), view_min[vn][f], (ctx, vn, f))
                _same(b.read_render(f), want, (ctx, "render", vn, "frame %d (%s)" % (f, names[f])))
        return bytes(raw), ovl

    view = views["anisotropic"]                                   # the viewport the firing solutions are bound with
    fv = _vp(view).firing_viewport()
    for key, fit in configs:
        fb.set_firing(hms[key], fit_to_minimap=fit, viewport=fv)
        fb.run(d.data_ptr(), N, stages=stages, anchors=anchors, stream=s)
        verified[(key, fit)] = check(fb, key, fit, s, ("plain batch", key, fit))
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, N, depth=3, search=search)        # (the frame-granular search needs depth >= 3)
        for key, fit in configs:
            p.set_firing(hms[key], fit_to_minimap=fit, viewport=fv)
            slot = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
            p.wait()
            got = check(p.slots[slot], key, fit, p.stream_of(slot), (search, key, fit))
            assert got == verified[(key, fit)], (search, key, fit)
        p.close()
    fb.set_firing(None)
    for hm in hms.values():
        hm.close()


@pytest.mark.parametrize("name", list(G.heightmaps()))
def test_every_form_draws_every_heightmap_through_real_rectangles(vision, world, name):
    """Every form of the tap fetch on one heightmap, through the three views of the matrix, with fit_to_minimap both ways, on every
    scene.  A forced form is the one launched by construction (launch_render_map takes it whenever the call has a heightmap, and
    every call here has one); the rule's form is asked of smhv_debug_render_rule: the table."""
    import squad_mortar_helper_amd as smh
    fb, s, names, recs, uis, rw, rh = (world[k] for k in ("fb", "s", "names", "recs", "uis", "rw", "rh"))
    ow, oh = G.WINDOW
    data, bounds, nothing = G.heightmaps()[name]
    H, W = data.shape
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0))
    cm = R.color_map(data)
    try:
        for vn, view in G.matrix_views(rw, rh).items():
            lds, rule_form = _rule(rw, rh, view, W, H)
            assert rule_form == _form_code("table"), (name, vn, rule_form)
            for fit in (True, False):
                wants = [_want(uis[f], recs[f], view, ow, oh, cm, bounds[0], fit) for f in range(N)]
                for f in range(N - 1):
                    G.assert_changes(wants[f], world["base"][vn][f], 0 if (nothing and not fit) else G.MATRIX_MIN[vn][f], (name, vn, fit, f, names[f]))
                if name == "1024x640" and vn == "thin":
                    # The staged launch has the most LDS there is, 12,288 texels.  The tiles left of x = 256 hold most of a
                    # rectangle's width, hundreds of tap columns: a band there fits only when it holds a single covered row (the
                    # rectangle's first or last); with two or more it spans 15 texel rows or more and falls back to the gathers.
                    # Right of x = 256 lie the rectangle's last 3 px or so, a few hundred tap columns: most bands there fit.
                    assert lds == 12288
                    st = ga = 0
                    for f in range(N - 1):
                        x0, y0, r, b = RR.hm_rect(recs[f]["minimap"], W, H, bounds[0][0], bounds[0][1], fit, view.scale, view.top_left)
                        sx, sy = np.float32(r - x0), np.float32(b - y0)
                        a, g = G.staged_bands(ow, oh, (x0, y0, np.float32(x0 + sx), np.float32(y0 + sy), sx, sy), W, H, lds)
                        st, ga = st + a, ga + g
                    assert st >= 20 and ga >= 20, (st, ga)
                for form in FORMS:
                    _set_form(form)
                    fb.render(_vp(view), ow, oh, heightmap=hm, markers=True, fit_to_minimap=fit, background=BG, stream=s)
                    for f in range(N):
                        _same(fb.read_render(f), wants[f], (name, vn, "fit" if fit else "offset", "form " + form, "frame %d (%s)" % (f, names[f])))
                        if nothing and not fit:                   # ... and equals the render without the heightmap
                            assert np.array_equal(wants[f], world["base"][vn][f])
    finally:
        _set_form("rule")
        hm.close()


@pytest.mark.parametrize("window", G.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_windows_at_the_tiles_edges(vision, world, window):
    import squad_mortar_helper_amd as smh
    fb, s, names, recs, uis, rw, rh = (world[k] for k in ("fb", "s", "names", "recs", "uis", "rw", "rh"))
    ow, oh = window
    data, bounds, _ = G.heightmaps()[G.WINDOW_MAP]
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0))
    cm = R.color_map(data)
    view = G.window_view(rw, rh, ow, oh)
    try:
        assert _rule(rw, rh, view, data.shape[1], data.shape[0])[1] == _form_code("table")
        for fit in (True, False):
            for f in range(N - 1):                                # (without lines: in a window of one pixel a line hides the overlay)
                G.assert_changes(_want(uis[f], recs[f], view, ow, oh, cm, bounds[0], fit, markers=False), _want(uis[f], recs[f], view, ow, oh, markers=False),
                                 G.WINDOW_MIN[window][fit][f], (window, fit, f, names[f]))
            for markers in (False, True):
                wants = [_want(uis[f], recs[f], view, ow, oh, cm, bounds[0], fit, markers=markers) for f in range(N)]
                for form in FORMS:
                    _set_form(form)
                    fb.render(_vp(view), ow, oh, heightmap=hm, markers=markers, fit_to_minimap=fit, background=BG, stream=s)
                    assert fb.render_size() == (ow, oh)
                    for f in range(N):
                        _same(fb.read_render(f), wants[f], (window, "fit" if fit else "offset", "markers %d" % markers, "form " + form, "frame %d (%s)" % (f, names[f])))
        # without a heightmap: the four-wave gather kernel
        fb.render(_vp(view), ow, oh, markers=True, background=BG, stream=s)
        for f in range(N):
            _same(fb.read_render(f), _want(uis[f], recs[f], view, ow, oh), (window, "no heightmap", "frame %d (%s)" % (f, names[f])))
    finally:
        _set_form("rule")
        hm.close()


def _per_call(vision, world):
    """Scene 0 as the current frame of the per-call path -> (ui_map, rectangle)."""
    vision.load_frame(world["frames"][0])
    r = vision.crop_to_map(grayscale=True)
    assert r is not None
    rect = vision.find_minimap()
    assert rect == world["rects"][0]
    return r[0], rect


@pytest.mark.parametrize("view_name", ("identity", "zoom 10, far pan"))
def test_256_explicit_lines_around_tile_borders_and_across_waves(vision, world, view_name):
    """vision.render_map with the maximum of explicit lines, in each forced form with a heightmap (a forced form is the one
    launched whenever the call has a heightmap; the table form compacts the lines with 16 waves, the others with 4) and once
    without a heightmap (the gather kernel, 4 waves)."""
    import squad_mortar_helper_amd as smh
    rw, rh = world["rw"], world["rh"]
    ow, oh = G.WINDOW
    ui, rect = _per_call(vision, world)
    view = G.line_views(rw, rh)[view_name]
    lines, fam = G.line_list(view)
    assert len(lines) == smh._lib.RENDER_MAX_LINES == 256
    masks = G.check_line_family(lines, fam, view, ow, oh)
    data, bounds, _ = G.heightmaps()["narrow"]
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0))
    cm = R.color_map(data)
    try:
        want = _want(ui, None, view, ow, oh, cm, bounds[0], True, lines=lines, rect=rect)
        G.check_pairs(want, masks, len(lines))
        assert _rule(rw, rh, view, data.shape[1], data.shape[0])[1] == _form_code("table")
        for form in FORMS:
            _set_form(form)
            got = vision.render_map(_vp(view), ow, oh, lines=lines, heightmap=hm, background=BG)
            _same(got, want, (view_name, "form " + form, "256 lines"))
        want = _want(ui, None, view, ow, oh, lines=lines, rect=rect)
        G.check_pairs(want, masks, len(lines))
        _same(vision.render_map(_vp(view), ow, oh, lines=lines, background=BG), want, (view_name, "no heightmap", "256 lines"))
    finally:
        _set_form("rule")
        hm.close()


def test_lines_with_an_end_point_that_is_not_finite(vision, world):
    """The kernel keeps such a line in every tile's list and the pixel test decides, as the restatement does over the whole
    window; no index depends on a line's coordinates."""
    import squad_mortar_helper_amd as smh
    rw, rh = world["rw"], world["rh"]
    ow, oh = G.WINDOW
    ui, rect = _per_call(vision, world)
    view = G.line_views(rw, rh)["identity"]
    data, bounds, _ = G.heightmaps()["narrow"]
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0))
    cm = R.color_map(data)
    cases = [(np.array([ln], np.float32), count) for ln, count in G.NON_FINITE]
    # all four between ordinary lines: 33,835 + 670 pixels of them, less what the later lines paint over
    mixed = np.array([[5, 40, 60, 44]] + [ln for ln, _ in G.NON_FINITE] + [[300, 3, 340, 60]], np.float32)
    cases.append((mixed, None))
    try:
        for lines, count in cases:
            if count is not None:
                assert int(RR.line_mask(ow, oh, lines[0], view.scale, view.top_left).sum()) == count, lines.tolist()
            want = _want(ui, None, view, ow, oh, cm, bounds[0], True, lines=lines, rect=rect)
            for form in FORMS:
                _set_form(form)
                _same(vision.render_map(_vp(view), ow, oh, lines=lines, heightmap=hm, background=BG), want, (lines.tolist(), "form " + form))
            want = _want(ui, None, view, ow, oh, lines=lines, rect=rect)
            _same(vision.render_map(_vp(view), ow, oh, lines=lines, background=BG), want, (lines.tolist(), "no heightmap"))
            if count is not None:
                assert G.changed(want, _want(ui, None, view, ow, oh, lines=None, rect=rect, markers=False)) == count
    finally:
        _set_form("rule")
        hm.close()
