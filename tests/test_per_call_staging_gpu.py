"""The context's pinned staging block (d_fire / h_fire) across the per-call entry points that share it: smhv_firing_solutions,
smhv_reach_map, smhv_clearance_lines, smhv_clearance_map, smhv_relief_map and the four forms of smhv_render_map lay it out each in
their own way and grow it on demand.  One context of its own runs them one after another, grows the block under another layout in
between, and runs them again: every result is the restatement's (tests/*_ref.py), compared as the per-call tests of each family
compare, and every repeated call gives its first result's bytes."""
import numpy as np
import pytest

import clearance_cases as CC
import clearance_ref as CR
import debug_text_cases as DC
import debug_text_ref as DR
import firing_ref as FR
import label_cases as LC
import minimap_scenes as S
import reach_cases as RC
import reach_ref as RR_
import relief_cases as EC
import relief_ref as ER
import render_geometry_cases as G
import test_clearance_gpu as TC
import test_debug_text_gpu as TD
import test_firing_gpu as TF
import test_labels_gpu as TL
import test_reach_gpu as TR
import test_relief_gpu as TE
import test_render_layers_gpu as TY

pytestmark = pytest.mark.gpu

RW, RH = 360, 585                                                # the map ROI of the scenes' frames
WINDOW = (96, 64)
MPX = 0.8372
FIRE_VIEW = (1.37, 0.81, -12.5, 33.0)


def _bytes(x):
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def _firing(v, w, lines):
    got = v.firing_solutions(lines, mpx=MPX, minimap=w["rect"], heightmap=w["hm"], fit_to_minimap=True, viewport=FIRE_VIEW)
    assert got.shape == (len(lines),)
    for i, ln in enumerate(lines):
        want = FR.firing_line(tuple(float(x) for x in ln), w["rect"], FR.record_meters(ln, MPX), w["ref_hm"], True, FIRE_VIEW)
        TF._check_line(got[i], want, ("firing", i, ln))
    return [got]


def _reach(v, w, case):
    r = w["reach"].setdefault(case.name, RC.restate(case))
    base, img, cls, res = TR._per_call(v, lambda hm: w["hm"], case, palette=TR.PALETTE)
    TR._same_classes(cls, r["classes"], case.name)
    assert np.array_equal(img, RR_.paint(base.copy(), r["classes"], TR.PALETTE)), case.name
    TR._same_summary(res, r, case.name)
    return [img, cls, res]


def _clearance_lines(v, w, case):
    if "clear_lines" not in w:
        w["clear_lines"] = CC.restate_lines(case)
    out, prof = TC._lines_call(v, lambda hm: w["hm"], case)        # (profiles=True)
    TC._same_lines(out, prof, *w["clear_lines"], case.name)
    return [out, prof]


def _clearance_map(v, w, case):
    if "clear_map" not in w:
        w["clear_map"] = CC.restate_map(case)
    r = w["clear_map"]
    base, img, b, res = TC._map_call(v, lambda hm: w["hm"], case)
    TC._same_bytes(b, r["bytes"], case.name)
    assert np.array_equal(img, CR.paint(base.copy(), r["bytes"], TC.PALETTE)), case.name
    TC._same_summary(res, r, case.name)
    return [img, b, res]


def _relief(v, w, case):
    """Every plane and the image in one call, then the heights alone: the layouts with the most and the fewest parts."""
    if "relief" not in w:
        w["relief"] = EC.restate(case)
    r = w["relief"]
    base, img, fb, sh, hs, res = TE._per_call(v, lambda hm: w["hm"], case)
    TE._same_plane(fb, r["bytes"], "flag bytes", case.name)
    TE._same_plane(sh, r["shades"], "shades", case.name)
    TE._same_plane(hs, r["heights"], "heights", case.name)
    assert np.array_equal(img, ER.paint(base.copy(), r, case.opt)), case.name
    TE._same_summary(res, r, case.name)
    _, none, fb1, sh1, alone, res1 = TE._per_call(v, lambda hm: w["hm"], case, paint=False, bytes=False, shades=False)
    assert none is None and fb1 is None and sh1 is None
    TE._same_plane(alone, r["heights"], "heights", case.name + ", the heights alone")
    TE._same_summary(res1, r, case.name + ", the heights alone")
    return [img, fb, sh, hs, res, alone, res1]


def _render(v, w):
    ow, oh = WINDOW
    got = v.render_map(TY._vp(w["view"]), ow, oh, lines=w["five"], heightmap=w["hm"], background=G.BG)
    TY._same(got, TY._want(w["ui"], None, w["view"], ow, oh, cm=w["cm"], b=w["hb"], lines=w["five"], rect=w["rect"]), "render_map")
    return [got]


def _layers(v, w):
    from squad_mortar_helper_amd import _lib as L
    ow, oh = WINDOW
    view_img = v.get_debug_view(L.VIEW_LSD_INPUT)
    got = v.render_map(TY._vp(w["view"]), ow, oh, lines=w["det"], background=G.BG, layers=TY._layers((), True, L.VIEW_LSD_INPUT))
    TY._same(got, TY._want(view_img, None, w["view"], ow, oh, (), True, True, lines=w["det"], rect=w["rect"]), "render_map_layers")
    return [got]


def _labeled(v, w):
    import squad_mortar_helper_amd as smh
    case, det = w["label_case"], w["det"]
    ow, oh = case.window
    opt = TL._options(case.view, ow, oh, markers=True)
    base = v.render_map(TL._vp(case.view), ow, oh, lines=det, options=opt)
    got, res = v.render_map(TL._vp(case.view), ow, oh, lines=det, heightmap=w["hm"], options=opt,
                            labels=smh.LabelOptions(case.lines, detected=True, scale=case.S, mpx=MPX))
    lines = [l for l, _ in case.lines] + [tuple(float(x) for x in l) for l in det]
    colors = [c for _, c in case.lines] + [tuple(int(x) for x in TL.RR.line_color(i, len(det))) for i in range(len(det))]
    firing = v.firing_solutions(np.array(lines, np.float32).reshape(-1, 4), mpx=MPX, minimap=w["rect"], heightmap=w["hm"], viewport=TL._viewport(case.view))
    want, n, _ = TL._slots_and_image(res, firing, lines, colors, case.view, case.S or 2, base, "render_map_labeled")
    TL._same(got, want, "render_map_labeled")
    assert n > 0
    return [base, got, res]


def _debug(v, w):
    case = w["debug_case"]
    ow, oh = case.window
    opt = TD._options(case.view, ow, oh)
    base = v.render_map(TD._vp(case.view), ow, oh, options=opt)
    got, res, probes = v.render_map(TD._vp(case.view), ow, oh, options=opt, debug=TD._debug(case))
    item_list, want_probes = DR.items(w["ui"], True, True, case.runs, case.points, case.flags, case.S, ow, oh, case.view.scale, case.view.top_left, TD.CONSTS)
    want = base.copy()
    assert DR.draw(want, item_list, case.S) > 0
    TD._same(got, want, "render_map_debug")
    TD._same_probes(probes, want_probes, len(case.points), "render_map_debug")
    assert res is None
    return [base, got, probes]


def _nine(v, w):
    seam = w["seam"]
    return [_firing(v, w, w["three"]), _reach(v, w, seam), _clearance_lines(v, w, w["clear_lines_case"]), _clearance_map(v, w, w["clear_map_case"]),
            _relief(v, w, w["relief_case"]), _render(v, w), _layers(v, w), _labeled(v, w), _debug(v, w)]


def test_the_entry_points_one_after_another_on_one_context(built):
    import squad_mortar_helper_amd as smh
    frames, _, rects, _ = S.make_scenes()
    assert tuple(S.roi()[2:]) == (RW, RH)
    v = smh.HipVision.init(0)                                       # a context of its own: its staging block starts empty
    hm = None
    try:
        v.load_frame(frames[0])
        ui = v.crop_to_map(grayscale=False)[0].copy()
        rect = v.find_minimap()
        assert rect == rects[0]
        v.isolate_map_markers()
        v.mask_marker_lines()
        det = v.find_marker_lines(15)[:8]
        assert len(det) >= 1
        data, bounds, scale = RC.steep_map()
        hm = smh.Heightmap(v, data, bounds, scale)
        rng = np.random.default_rng(31)
        lines = rng.uniform(-20.0, 600.0, size=(smh._lib.RENDER_MAX_LINES, 4)).astype(np.float32)
        debug_case = DC.tile_cases(RW, RH)[0]
        seam = RC.Case("staging", RC.steep_map(), (20, 70, 10, 50), 21.0, (44.0, 31.0), WINDOW, None, True, 10.0, None)
        big = seam._replace(name="staging, 640 x 360", window=(640, 360), viewport=(640.0 / 96.0, 360.0 / 64.0, 0.0, 0.0), origin=(293.0, 174.0))
        terrain, mm = (data, bounds, scale), seam.minimap
        three_lines = ((22.0, 12.0, 68.0, 48.0), (30.5, 40.25, 60.0, 15.0), (25.0, 30.0, 25.0, 30.0))   # inside the rectangle; the last has no length
        w = dict(ui=ui, rect=rect, det=det, hm=hm, ref_hm=(data, bounds, scale), cm=FR.color_map(data), hb=bounds[0], view=G.window_view(RW, RH, *WINDOW),
                 three=lines[:3], five=lines[3:8], label_case=LC.window_cases(RW, RH)[3], seam=seam, reach={},
                 clear_lines_case=CC.LineCase("staging", terrain, mm, three_lines, 64, 0.0, None, True, None),
                 clear_map_case=CC.MapCase("staging", terrain, mm, seam.origin, WINDOW, 64, 0.0, None, True, None),
                 relief_case=EC.Case("staging", "staging", terrain, mm, WINDOW, None, True, TE.OPT, None),
                 debug_case=DC.Case("staging", debug_case.window, debug_case.view, 1, debug_case.runs[:3], [(100.5, 200.5)], DR.DRAW_PROBES))
        first = _nine(v, w)
        assert {RR_.SCALES, RR_.HEIGHTMAP} <= set(int(x) for x in np.unique(w["reach"]["staging"]["source"]))
        _reach(v, w, big)                                           # the block grows, under the reach map's layout
        _firing(v, w, lines)                                        # SMHV_RENDER_MAX_LINES lines
        again = _nine(v, w)
        for step, (a, b) in enumerate(zip(first, again)):
            assert [_bytes(x) for x in a] == [_bytes(x) for x in b], "step %d differs when it is repeated" % (step + 1)
    finally:
        if hm is not None:
            hm.close()
        v.shutdown()
