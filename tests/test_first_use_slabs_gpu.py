"""The result slabs a batch allocates on a family's first call (the reach map, the line clearance, the clearance map, the relief, the
marker labels, the probes, the scale labels, their text, the firing solutions): before that call the family's read_* and *_ptr answer
E_STATE; the first call covers one frame only, and the whole slab is read afterwards -- every row the call did not cover is zero
bytes (the scale labels' crop cells: 255), and the covered row is what the family's own test computes for that frame."""
import ctypes as C

import numpy as np
import pytest

import clearance_ref as CR
import debug_text_cases as DC
import debug_text_ref as DR
import label_text_cases as XC
import label_text_ref as XR
import minimap_scenes as S
import reach_cases as RC
import reach_ref as RR
import relief_ref as ER
import scale_labels_ref as SR
import test_clearance_gpu as TC
import test_debug_text_gpu as TD
import test_firing_gpu as TF
import test_label_text_gpu as TX
import test_labels_gpu as TL
import test_reach_gpu as TR
import test_relief_gpu as TE
import test_scale_labels_gpu as TS

pytestmark = pytest.mark.gpu

N = S.N_SCENES
ONE = 2                                                          # the frame the windowed families' first call covers: first=2, n=1
ORIGIN = (150.0, 260.0)
FIRE_VIEW = (1.25, 1.25, -30.0, 12.0)


def _others_zero(rows, covered, row_bytes, ctx):
    raw = bytes(rows)
    assert len(raw) == row_bytes * N, (ctx, len(raw), row_bytes)
    for f in range(N):
        if f != covered:
            assert raw[f * row_bytes:(f + 1) * row_bytes] == bytes(row_bytes), (ctx, "row %d is not zero" % f)


def _readers(fb):
    return dict(read_reach=lambda: fb.read_reach(0, 1), reach_ptr=fb.reach_ptr, read_clearance=lambda: fb.read_clearance(0, 1), clearance_ptr=fb.clearance_ptr,
                read_clearance_map=lambda: fb.read_clearance_map(0, 1), clearance_map_ptr=fb.clearance_map_ptr, read_relief=lambda: fb.read_relief(0, 1),
                relief_ptr=fb.relief_ptr, read_labels=lambda: fb.read_labels(0, 1), labels_ptr=fb.labels_ptr, read_probes=lambda: fb.read_probes(0, 1),
                probes_ptr=fb.probes_ptr, read_scale_labels=lambda: fb.read_scale_labels(0, 1), scale_labels_ptr=fb.scale_labels_ptr,
                read_label_text=lambda: fb.read_label_text(0, 1), label_text_ptr=fb.label_text_ptr, read_firing=lambda: fb.read_firing(0, 1),
                firing_ptr=fb.firing_ptr)


def _reach(fb, s, hm, hm_data, rec):
    import squad_mortar_helper_amd as smh
    fb.reach(TR._options(TR.VIEW, TR.WINDOW), smh.ReachOptions(origin=ORIGIN, ring_m=TR.RING, paint=False), first=ONE, n=1, heightmap=hm, stream=s)
    res = fb.read_reach(0, N)
    _others_zero(res, ONE, 64, "reach")
    want = RR.reach(ORIGIN, TR.WINDOW, TR.VIEW, rec["minimap"], rec["mpx"], hm_data, True, TR.RING)
    assert want["valid"]
    TR._same_summary(res[ONE], want, "reach")
    assert fb.reach_ptr() != 0


def _clearance(fb, s, hm, hm_data, rec):
    import squad_mortar_helper_amd as smh
    fb.clearance(smh.ClearanceOptions(samples=64), first=ONE, n=1, heightmap=hm, fit_to_minimap=False, viewport=TC.LINE_VIEW, stream=s)
    out = fb.read_clearance(0, N)
    _others_zero(out, ONE, 8 + 64 * 32, "clearance")
    want, _ = CR.lines(rec["lines"], 64, 0.0, rec["minimap"], hm_data, False, TC.LINE_VIEW)
    assert out[ONE].n_lines == rec["n_lines"] >= 1 and out[ONE].reserved == 0
    TC._same_lines(out[ONE].line[:rec["n_lines"]], None, want, None, "clearance")
    assert bytes(out[ONE])[8 + 64 * rec["n_lines"]:] == bytes(64 * (32 - rec["n_lines"]))
    assert fb.clearance_ptr() != 0


def _clearance_map(fb, s, hm, hm_data, rec):
    import squad_mortar_helper_amd as smh
    fb.clearance_map(TC._options(TC.VIEW, TC.WINDOW), smh.ClearanceOptions(samples=64, origin=ORIGIN, paint=False), first=ONE, n=1, heightmap=hm, stream=s)
    res = fb.read_clearance_map(0, N)
    _others_zero(res, ONE, 32, "clearance map")
    want = CR.clearance_map(ORIGIN, TC.WINDOW, 64, 0.0, TC.VIEW, rec["minimap"], hm_data, True)
    assert want["valid"]
    TC._same_summary(res[ONE], want, "clearance map")
    assert fb.clearance_map_ptr() != 0


def _relief(fb, s, hm, hm_data, rec):
    assert fb.relief(TE._options(TE.VIEW, TE.WINDOW), TE._relief_options(TE.OPT, paint=False), first=ONE, n=1, heightmap=hm, stream=s) == {}
    res = fb.read_relief(0, N)
    _others_zero(res, ONE, 48, "relief")
    want = ER.relief(TE.WINDOW, TE.VIEW, rec["minimap"], hm_data, True, TE.OPT)
    assert want["valid"]
    TE._same_summary(res[ONE], want, "relief")
    assert fb.relief_ptr() != 0


def _labels(vision, fb, s, hm, rec):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    view = TL.G.matrix_views(TL.RW, TL.RH)["anisotropic"]
    ow, oh = TL.G.WINDOW
    opt = TL._options(view, ow, oh, markers=True)
    fb.render(TL._vp(view), ow, oh, options=opt, stream=s)
    base = [fb.read_render(f).copy() for f in range(N)]
    extras = TL._batch_extras(view)
    fb.render_labels(opt, smh.LabelOptions(extras, detected=True, scale=1), first=ONE, n=1, heightmap=hm, stream=s)
    res = fb.read_labels(0, N)
    _others_zero(res, ONE, C.sizeof(L.LabelResult), "labels")
    lines = [l for l, _ in extras] + [tuple(float(v) for v in l) for l in rec["lines"]]
    colors = [c for _, c in extras] + [tuple(int(v) for v in TL.RR.line_color(i, rec["n_lines"])) for i in range(rec["n_lines"])]
    firing = vision.firing_solutions(np.array(lines, np.float32).reshape(-1, 4), mpx=rec["mpx"], minimap=rec["minimap"], heightmap=hm, fit_to_minimap=True,
                                     viewport=TL._viewport(view))
    want, n, _ = TL._slots_and_image(res[ONE], firing, lines, colors, view, 1, base[ONE], "labels")
    assert n > 0
    for f in range(N):                                             # ... and the other frames' images are the render's
        TL._same(fb.read_render(f), want if f == ONE else base[f], ("labels", f))
    assert fb.labels_ptr() != 0


def _probes(fb, s):
    import squad_mortar_helper_amd as smh
    view = DC.probe_views(TD.RW, TD.RH)["zoomed"]
    pts = DC.probe_points(view, TD.RW, TD.RH, DC.cells(7))
    fb.probe(TD._options(view, 64, 32), pts, first=ONE, n=1, stream=s)
    got = fb.read_probes(0, N)
    _others_zero(got, ONE, 32 * DR.MAX_PROBES, "probes")
    ui = fb.read_image(smh._lib.IMAGE_UI_MAP, ONE)
    want = [DR.probe(ui, True, pt, view.scale, view.top_left, TD.CONSTS) for pt in pts]
    assert sum(w["valid"] for w in want) >= 9
    TD._same_probes(got[ONE * DR.MAX_PROBES:(ONE + 1) * DR.MAX_PROBES], want, len(pts), "probes")
    assert fb.probes_ptr() != 0


def _scale_labels(fb, s, d, frame):
    fb.scale_labels(d.data_ptr(), 1, stream=s)
    recs, cells = fb.read_scale_labels(0, N)
    _others_zero(recs, 0, 288, "scale labels")
    assert (cells[1:] == 255).all(), "a crop cell of a frame the call did not cover is not 255"
    want = SR.of_frame(frame)
    assert want is not None
    TS._check(recs[0], cells[0], want, "scale labels")
    assert (cells[0, want["header"][0]:] == 255).all()
    assert all(fb.scale_labels_ptr())
    return recs[0], want


def _label_text(vision, fb, s, sl_rec, want):
    import squad_mortar_helper_amd as smh
    atlas = XC.cases()[0]["atlas"]
    dev = smh.GlyphAtlas.from_templates(vision, XC.lib_templates(atlas), atlas.num, atlas.den)
    try:
        fb.label_text(dev, 1, stream=s)
        recs = fb.read_label_text(0, N)
        _others_zero(recs, 0, XR.REC_BYTES, "label text")
        TX._check(recs[0], sl_rec, want, atlas, "label text")
        d_text, d_anchors = fb.label_text_ptr()
        assert d_text and d_anchors
        tight = TX._d2h(d_anchors, 44 * N).tobytes()                # the anchors' slab, tightly packed
        assert tight[:44] == bytes(recs[0].anchors) and tight[44:] == bytes(44 * (N - 1))
    finally:
        dev.close()


def _firing(fb, s, d, anchors, stages, hm, hm_data):
    import squad_mortar_helper_amd as smh
    fb.set_firing(hm, fit_to_minimap=False, viewport=FIRE_VIEW)
    fb.run(d.data_ptr(), 1, stages=stages | smh.STAGE_FIRING, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, 1))
    n_lines, slab = fb.read_firing(0, N)
    assert not n_lines[1:].any() and slab[1:].tobytes() == bytes(48 * 32 * (N - 1))
    assert recs[0]["n_lines"] >= 1
    TF._check_slab(recs, n_lines[:1], slab[:1], hm_data, False, FIRE_VIEW, "firing")
    assert fb.firing_ptr() != 0


def test_a_first_call_over_one_frame_leaves_the_rest_of_its_slab_cleared(vision):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    frames, anchor_list, _, _ = S.make_scenes()
    assert (S.roi()[2], S.roi()[3]) == (TL.RW, TL.RH)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    hm_data = RC.long_map()
    hm = smh.Heightmap(vision, *hm_data)
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    try:
        fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
        recs = smh.results_to_dicts(fb.read_results(0, N))
        rec = recs[ONE]
        assert rec["map_open"] and rec["minimap"] is not None and rec["n_lines"] >= 1
        for name, call in _readers(fb).items():                    # no family has made its first call
            with pytest.raises(smh.VisionError) as ei:
                call()
            assert ei.value.code == L.E_STATE, name
        _reach(fb, s, hm, hm_data, rec)
        _clearance(fb, s, hm, hm_data, rec)
        _clearance_map(fb, s, hm, hm_data, rec)
        _relief(fb, s, hm, hm_data, rec)
        _labels(vision, fb, s, hm, rec)
        _probes(fb, s)
        sl_rec, want = _scale_labels(fb, s, d, frames[0])
        _label_text(vision, fb, s, sl_rec, want)
        _firing(fb, s, d, anchors, stages, hm, hm_data)
    finally:
        fb.close()
        hm.close()
