"""The marker labels on the device (smhv_batch_render_labels / smhv_render_map_labeled), every comparison exact: a slot's numbers
byte-equal to smhv_firing_solutions / the firing slab of the same lines, viewport and heightmap; the slot equal to the restatement
(tests/label_ref.py) fed THOSE numbers; the image equal to the restatement's draw over the image of the same call without labels,
byte for byte."""
import ctypes as C

import numpy as np
import pytest

import label_cases as LC
import label_ref as R
import minimap_scenes as S
import render_geometry_cases as G
import render_ref as RR

pytestmark = pytest.mark.gpu

BG = G.BG
N = S.N_SCENES
MPX = 0.8372
RW, RH = 360, 585                                                # the map ROI of the scenes' frames (asserted by the world fixture)
f32 = np.float32


def _vp(view):
    import squad_mortar_helper_amd as smh
    return smh.MapViewport(view.quad, view.scale, view.top_left)


def _viewport(view):
    return (view.scale[0], view.scale[1], view.top_left[0], view.top_left[1])


def _options(view, ow, oh, markers=False, fit=True, overlay=False):
    import squad_mortar_helper_amd as smh
    return smh.render_options(_vp(view), ow, oh, heightmap=overlay, markers=markers, fit_to_minimap=fit, background=BG)


def _fdict(rec):
    return {"meters": float(rec["meters"]), "alt_delta": float(rec["alt_delta"]), "mils": (float(rec["mils"][0]), float(rec["mils"][1])),
            "bearing": (float(rec["bearing"][0]), float(rec["bearing"][1])), "source": int(rec["source"])}


def _pack(slot, firing_rec):
    """The restatement's slot, with the device's firing record, as the bytes of a smhv_label."""
    from squad_mortar_helper_amd import _lib as L
    lab = L.Label()
    C.memmove(C.byref(lab), firing_rec.tobytes(), 48)
    lab.mid[0], lab.mid[1] = float(slot["mid"][0]), float(slot["mid"][1])
    lab.dir[0], lab.dir[1] = float(slot["dir"][0]), float(slot["dir"][1])
    for k in range(4):
        lab.rgba[k] = slot["rgba"][k]
    lab.n_runs = len(slot["runs"])
    for k, (x2, y2, text) in enumerate(slot["runs"]):
        lab.run[k].x2, lab.run[k].y2, lab.run[k].n = x2, y2, len(text)
        for j, ch in enumerate(text):
            lab.run[k].text[j] = ch
    return bytes(lab)


def _same(got, want, ctx):
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=2))
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d pixels differ" % len(bad), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // LC.TW, y // LC.TH),
                              "got", got[y, x].tolist(), "want", want[y, x].tolist()))


def _slots_and_image(res, firing, lines, colors, view, S_, base, ctx):
    """The device's result against the restatement fed the device's numbers -> (the restatement's image, pixels changed, sources)."""
    from squad_mortar_helper_amd import _lib as L
    assert res.n_labels == len(lines), (ctx, res.n_labels, len(lines))
    slots = []
    for i, (line, rgba) in enumerate(zip(lines, colors)):
        slot = R.format_label(line, _fdict(firing[i]), _viewport(view), rgba)
        got = bytes(res.label[i])
        assert got[:48] == firing[i].tobytes(), (ctx, "slot %d: the numbers are not smhv_firing_solutions'" % i)
        want = _pack(slot, firing[i])
        assert got == want, (ctx, "slot %d" % i, [(r.x2, r.y2, bytes(r.text[:r.n])) for r in res.label[i].run[:res.label[i].n_runs]], slot["runs"],
                             tuple(res.label[i].mid), slot["mid"], tuple(res.label[i].dir), slot["dir"])
        slots.append(slot)
    zero = bytes(C.sizeof(L.Label))
    for i in range(len(lines), L.LABEL_SLOTS):
        assert bytes(res.label[i]) == zero, (ctx, "slot %d beyond n_labels is not zero" % i)
    want = base.copy()
    n = R.draw(want, slots, S_)
    return want, n, [int(f["source"]) for f in firing]


@pytest.fixture(scope="module")
def world(vision):
    """The scenes of tests/minimap_scenes.py with the closed frame moved between open ones, in a plain batch that has run once with
    the firing stage; a heightmap whose altitudes differ from texel to texel."""
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    frames, anchor_list, rects, names = S.make_scenes()
    order = [0, 1, N - 1] + list(range(2, N - 1))                   # the closed scene becomes frame 2
    frames = np.ascontiguousarray(frames[order])
    anchor_list, rects, names = [anchor_list[i] for i in order], [rects[i] for i in order], [names[i] for i in order]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    _, _, rw, rh = fb.roi
    assert (rw, rh) == (RW, RH)
    data = G.heightmaps()["from 0"][0]
    hm = smh.Heightmap(vision, data, ((9, -15), (0, 0)), (1.0, 1.0, 40.0))
    view = G.matrix_views(rw, rh)["anisotropic"]
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_FIRING
    fb.set_firing(hm, True, _viewport(view))
    fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    assert not recs[2]["map_open"] and all(recs[f]["map_open"] and recs[f]["n_lines"] >= 1 for f in range(N) if f != 2)
    w = dict(frames=frames, d=d, s=s, anchors=anchors, rects=rects, names=names, fb=fb, rw=rw, rh=rh, recs=recs, stages=stages, hm=hm, view=view,
             fired=fb.read_firing(0, N))
    yield w
    hm.close()
    fb.close()


@pytest.fixture(scope="module")
def current(vision, world):
    """Scene 0 as the current frame of the per-call path -> (rectangle, detected lines)."""
    vision.load_frame(world["frames"][0])
    assert vision.crop_to_map(grayscale=False) is not None
    rect = vision.find_minimap()
    assert rect == world["rects"][0]
    vision.isolate_map_markers()
    vision.mask_marker_lines()
    lines = vision.find_marker_lines(15)
    assert len(lines) >= 1
    return rect, lines


def _call(vision, world, rect, case, hm, mpx, fit=True, detected=None, layers=None, overlay=False):
    """One per-call render with labels against the same call without them -> (pixels changed on the restatement, sources)."""
    import squad_mortar_helper_amd as smh
    ow, oh = case.window
    det = np.zeros((0, 4), np.float32) if detected is None else np.asarray(detected, np.float32).reshape(-1, 4)
    opt = _options(case.view, ow, oh, markers=len(det) > 0, fit=fit, overlay=overlay)
    base = vision.render_map(_vp(case.view), ow, oh, lines=det, heightmap=hm if overlay else None, options=opt, layers=layers)
    lo = smh.LabelOptions(case.lines, detected=detected is not None, scale=case.S, mpx=mpx)
    got, res = vision.render_map(_vp(case.view), ow, oh, lines=det, heightmap=hm, options=opt, layers=layers, labels=lo)
    lines = [l for l, _ in case.lines] + [tuple(float(v) for v in l) for l in det]
    colors = [c for _, c in case.lines] + [tuple(int(v) for v in RR.line_color(i, len(det))) for i in range(len(det))]
    firing = vision.firing_solutions(np.array(lines, np.float32).reshape(-1, 4), mpx=mpx, minimap=rect, heightmap=hm, fit_to_minimap=fit,
                                     viewport=_viewport(case.view))
    want, n, sources = _slots_and_image(res, firing, lines, colors, case.view, case.S or 2, base, case)
    _same(got, want, case)
    return n, sources, base, got


@pytest.mark.parametrize("case", LC.all_cases(RW, RH), ids=lambda c: c.name)
def test_every_case_on_the_per_call_path(vision, world, current, case):
    """Windows at the tile's edges, labels across tile borders and corners, S = 1 .. 4, vertical lines both ways, d.x < 0, labels
    outside the window, 64 labels on one spot, zoom 10, a scale per axis, zero-length and non-finite lines: with a heightmap and
    m/px, so lines inside the minimap rectangle take the heightmap's range and the others the scales'."""
    rect, _ = current
    n, sources, base, got = _call(vision, world, rect, case, world["hm"], MPX)
    if case.minimum is None:
        assert n == 0 and np.array_equal(got, base)
    else:
        assert n >= case.minimum, (case, n)
    assert R.NONE not in sources


def test_sources_none_scales_and_heightmap_with_and_without_the_offset(vision, world, current):
    rect, _ = current
    case = LC.scale_cases(world["rw"], world["rh"])[1]                 # S = 2
    n, sources, base, got = _call(vision, world, rect, case, None, None)
    assert set(sources) == {R.NONE} and n == 0 and np.array_equal(got, base)
    n, sources, _, _ = _call(vision, world, rect, case, None, MPX)
    assert set(sources) == {R.SCALES} and n >= case.minimum
    for fit in (True, False):
        for overlay in (False, True):
            n, sources, _, _ = _call(vision, world, rect, case, world["hm"], MPX, fit=fit, overlay=overlay)
            assert set(sources) == {R.SCALES, R.HEIGHTMAP} and n >= case.minimum, (fit, overlay, sources)
    # the heightmap alone: lines outside the rectangle have no range and no label
    n, sources, _, _ = _call(vision, world, rect, case, world["hm"], None)
    assert set(sources) == {R.NONE, R.HEIGHTMAP} and n >= LC.ink(2)
    # scale 0 means 2
    c0 = LC.Case("S = 0", case.window, case.view, 0, case.lines, case.minimum)
    _, _, _, got0 = _call(vision, world, rect, c0, world["hm"], MPX)
    _, _, _, got2 = _call(vision, world, rect, case, world["hm"], MPX)
    assert np.array_equal(got0, got2)


def test_96_slots_on_one_spot_the_last_one_wins(vision, world, current):
    rect, _ = current
    case = LC.stack_case(world["rw"], world["rh"], 64)
    det = np.array([case.lines[0][0]] * 32, np.float32)
    n, sources, base, got = _call(vision, world, rect, case, None, MPX, detected=det)
    assert n >= case.minimum
    # the 32 strokes of the detected lines lie under the text; wherever text was painted it has the last ramp colour, (0, 255, 0)
    changed = np.any(got != base, axis=2)
    assert changed.sum() >= case.minimum and np.all(got[changed] == np.array([0, 255, 0, 255], np.uint8))
    # the same 64 alone: the last extra's colour
    n, _, base, got = _call(vision, world, rect, case, None, MPX)
    changed = np.any(got != base, axis=2)
    assert np.all(got[changed] == np.array(case.lines[-1][1], np.uint8))


def test_dir_of_256_random_lines_is_numpy_f32(vision, world, current):
    """sqrtf and the two divisions are correctly rounded: mid and dir bit-equal to numpy's f32 for 256 random lines."""
    import squad_mortar_helper_amd as smh
    rect, _ = current
    rng = np.random.default_rng(20)
    view = G.View.direct(world["rw"], world["rh"], 1.37, 0.61, -3.25, 7.5)
    ow, oh = 257, 33
    opt = _options(view, ow, oh)
    for part in range(4):
        pts = rng.uniform(-300.0, 900.0, size=(64, 4)).astype(np.float32)
        extras = [(tuple(float(v) for v in p), LC.MAGENTA) for p in pts]
        _, res = vision.render_map(_vp(view), ow, oh, options=opt, labels=smh.LabelOptions(extras, detected=False, scale=1, mpx=MPX))
        assert res.n_labels == 64
        for i, p in enumerate(pts):
            p0x, p0y = f32(p[0] * view.scale[0]) + view.top_left[0], f32(p[1] * view.scale[1]) + view.top_left[1]
            p1x, p1y = f32(p[2] * view.scale[0]) + view.top_left[0], f32(p[3] * view.scale[1]) + view.top_left[1]
            dx, dy = f32(p0x - p1x), f32(p0y - p1y)
            ln = np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))
            s = f32(1) if dx > 0 else f32(-1)
            want = np.array([f32(f32(p0x + p1x) / f32(2)), f32(f32(p0y + p1y) / f32(2)), f32(f32(s * dx) / ln), f32(f32(s * dy) / ln)], np.float32)
            lab = res.label[i]
            got = np.array([lab.mid[0], lab.mid[1], lab.dir[0], lab.dir[1]], np.float32)
            assert lab.n_runs == 4 and got.tobytes() == want.tobytes(), (part, i, got, want)


def test_layers_none_and_the_layers_image_under_the_labels(vision, world, current):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    rect, det = current
    case = LC.scale_cases(world["rw"], world["rh"])[1]
    prims = [smh.prim(20, 20, 300, 200, (1, 2, 3, 255), L.PRIM_RECT | L.PRIM_FOREGROUND), smh.prim(0, 64, 600, 64, (250, 250, 0, 255), L.PRIM_LINE),
             smh.prim(100, 30, 500, 90, (0, 250, 250, 255), L.PRIM_LINE | L.PRIM_FOREGROUND)]
    for layers in (None, smh.RenderLayers(), smh.RenderLayers(prims, minimap_bounds=True), smh.RenderLayers(prims, map_source=L.VIEW_LSD_INPUT)):
        n, _, base, got = _call(vision, world, rect, case, world["hm"], MPX, detected=det[:32], layers=layers)
        assert n >= case.minimum
        if layers is not None and layers.prims:
            # the layers' image is there under the labels: every pixel no label painted is the call's without labels
            keep = ~np.any(got != base, axis=2)
            assert np.any(np.all(got[keep] == np.array((1, 2, 3, 255), np.uint8), axis=1))
    # more detected lines than a record holds: rendered by the sibling, refused with labels
    many = np.tile(det[:1], (33, 1))
    vision.render_map(_vp(case.view), *case.window, lines=many, options=_options(case.view, *case.window, markers=True))
    with pytest.raises(smh.VisionError) as ei:
        vision.render_map(_vp(case.view), *case.window, lines=many, options=_options(case.view, *case.window, markers=True),
                          labels=smh.LabelOptions(detected=True))
    assert ei.value.code == L.E_INVALID
    # ... and not refused when the detected lines are not labelled
    vision.render_map(_vp(case.view), *case.window, lines=many, options=_options(case.view, *case.window, markers=True), labels=smh.LabelOptions(detected=False))


def _batch_extras(view):
    return [LC._line(view, 150.0, 3.0, 4.0, 90.0, LC.CYAN), LC._line(view, 64.0, 32.0, -15.0, 70.0, LC.RED), LC._line(view, 384.0, 2.0, 183.0, 60.0)]


def _check_batch(vision, world, b, stream, recs, extras, detected, ctx, parts=None, fit=True, view=None, window=G.WINDOW, S_=1, fired=None):
    """Render, read the images, draw the labels (in `parts`: [(first, n)]), and hold every frame against the restatement."""
    import squad_mortar_helper_amd as smh
    view = view or world["view"]
    ow, oh = window
    opt = _options(view, ow, oh, markers=True, fit=fit)
    b.render(_vp(view), ow, oh, options=opt, stream=stream)
    base = [b.read_render(f).copy() for f in range(N)]
    lo = smh.LabelOptions(extras, detected=detected, scale=S_)
    for first, n in parts or [(0, N)]:
        b.render_labels(opt, lo, first=first, n=n, heightmap=world["hm"], stream=stream)
    res = b.read_labels(0, N)
    total, seen = 0, set()
    for f in range(N):
        rec = recs[f]
        got = b.read_render(f)
        if not rec["map_open"]:
            assert res[f].n_labels == 0 and np.array_equal(got, base[f]) and np.all(got == np.array(BG, np.uint8)), (ctx, f)
            continue
        det = rec["lines"] if detected else np.zeros((0, 4), np.float32)
        lines = [l for l, _ in extras] + [tuple(float(v) for v in l) for l in det]
        colors = [c for _, c in extras] + [tuple(int(v) for v in RR.line_color(i, len(det))) for i in range(len(det))]
        firing = vision.firing_solutions(np.array(lines, np.float32).reshape(-1, 4), mpx=rec["mpx"], minimap=rec["minimap"], heightmap=world["hm"],
                                         fit_to_minimap=fit, viewport=_viewport(view))
        if fired is not None and detected:                        # ... and the detected lines' numbers are the firing slab's
            n_fired, lines_fired = fired
            assert n_fired[f] == len(det)
            for i in range(len(det)):
                assert bytes(res[f].label[len(extras) + i])[:48] == lines_fired[f][i].tobytes(), (ctx, f, i)
        want, n, sources = _slots_and_image(res[f], firing, lines, colors, view, S_, base[f], (ctx, f, world["names"][f]))
        _same(got, want, (ctx, f, world["names"][f]))
        total += n
        seen |= set(sources)
    return total, seen


def test_the_batch_call_on_a_plain_batch_and_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    fb, d, s, anchors, recs = (world[k] for k in ("fb", "d", "s", "anchors", "recs"))
    extras = _batch_extras(world["view"])
    total, seen = _check_batch(vision, world, fb, s, recs, extras, True, "plain batch", fired=world["fired"])
    # nine open frames, three extras each wholly inside the window
    assert total >= LC.ink(1, 3 * (N - 1)) and seen == {R.NONE, R.SCALES, R.HEIGHTMAP}, (total, seen)
    assert fb.labels_ptr() != 0
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, N, depth=3, search=search)
        slot = p.submit(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors)
        p.wait()
        total, _ = _check_batch(vision, world, p.slots[slot], p.stream_of(slot), recs, extras, True, search)
        assert total >= LC.ink(1, 3 * (N - 1))
        p.close()


def test_the_batch_call_in_two_parts_with_the_offset_and_other_scales(vision, world):
    fb, s, recs = (world[k] for k in ("fb", "s", "recs"))
    view = LC.unit_view(world["rw"], world["rh"])
    extras = [LC._line(view, 192.0, 160.0, 45.0, 80.0), LC._line(view, 400.0, 64.0, -60.0, 80.0, LC.RED)]
    for S_, fit, parts in ((2, False, [(0, 4), (4, N - 4)]), (3, True, [(7, N - 7), (0, 7)]), (0, True, [(0, 1), (1, N - 1)])):
        total, seen = _check_batch(vision, world, fb, s, recs, extras, True, ("parts", S_, fit), parts=parts, fit=fit, view=view, window=(640, 360), S_=S_ or 2)
        assert total >= LC.ink(S_ or 2, 2 * (N - 1)) and R.HEIGHTMAP in seen


def test_a_frame_with_no_lines_and_a_call_with_no_labels(vision, world):
    import squad_mortar_helper_amd as smh
    d, s = world["d"], world["s"]
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=smh.STAGE_UI_MAP | smh.STAGE_MINIMAP, grayscale=True, anchors=None, stream=s)
    recs2 = smh.results_to_dicts(fb2.read_results(0, N))
    assert all(r["n_lines"] == 0 and r["mpx"] is None for r in recs2)
    extras = _batch_extras(world["view"])
    # no lines, extras alone: no m/px, so a label only where the heightmap gives the range
    total, seen = _check_batch(vision, world, fb2, s, recs2, extras, True, "no lines")
    assert seen == {R.NONE, R.HEIGHTMAP} and total >= LC.ink(1)
    # neither extras nor detected lines: the slab says so and the image stays
    total, _ = _check_batch(vision, world, fb2, s, recs2, [], True, "nothing to label")
    assert total == 0
    total, _ = _check_batch(vision, world, fb2, s, recs2, [], False, "nothing asked")
    assert total == 0
    fb2.close()


def test_argument_errors_enqueue_nothing(vision, world, current):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s, recs = (world[k] for k in ("fb", "s", "recs"))
    view = world["view"]
    ow, oh = G.WINDOW
    opt = _options(view, ow, oh, markers=True)
    extras = _batch_extras(view)
    # before any render: SMHV_E_STATE, and no slab to read
    fb0 = smh.FrameBatch(vision, S.W, S.H, 2)
    fb0.run(world["d"].data_ptr(), 2, stages=smh.STAGE_UI_MAP, grayscale=True, anchors=None, stream=s)
    lo, keep = smh.LabelOptions(extras).struct()
    assert lib.smhv_batch_render_labels(fb0._b, 0, 2, None, C.byref(opt), C.byref(lo), s) == L.E_STATE
    out1 = (L.LabelResult * 1)()
    assert lib.smhv_batch_read_labels(fb0._b, 0, 1, out1) == L.E_STATE
    ptr = C.c_void_p()
    assert lib.smhv_batch_labels_ptr(fb0._b, C.byref(ptr)) == L.E_STATE
    fb0.close()

    fb.render(_vp(view), ow, oh, options=opt, stream=s)
    fb.render_labels(opt, smh.LabelOptions(extras), heightmap=world["hm"], stream=s)
    images = [fb.read_render(f).copy() for f in range(N)]
    slab = bytes(fb.read_labels(0, N))

    def options(**kw):
        lo, keep = smh.LabelOptions(extras, detected=True, scale=2).struct()
        for k, v in kw.items():
            setattr(lo, k, v)
        return lo, keep
    bad = [options(size=24), options(size=40), options(flags=2), options(flags=0x80000001), options(scale=5), options(n_extra=65)]
    lo, keep = options()
    lo.extra = None                                                 # n_extra != 0 with extra == NULL
    bad.append((lo, keep))
    bad.append(smh.LabelOptions([(extras[0][0], (1, 2, 3, 254))]).struct())
    bad.append(smh.LabelOptions(extras + [(extras[0][0], (1, 2, 3, 0))]).struct())
    bad.append(smh.LabelOptions([extras[0]] * 65).struct())
    for i, (lo, keep) in enumerate(bad):
        assert lib.smhv_batch_render_labels(fb._b, 0, N, None, C.byref(opt), C.byref(lo), s) == L.E_INVALID, i
    lo, keep = options()
    assert lib.smhv_batch_render_labels(fb._b, 0, N, None, C.byref(opt), None, s) == L.E_INVALID
    assert lib.smhv_batch_render_labels(fb._b, 0, N, None, None, C.byref(lo), s) == L.E_INVALID
    assert lib.smhv_batch_render_labels(fb._b, 1, N, None, C.byref(opt), C.byref(lo), s) == L.E_INVALID        # beyond the capacity
    assert lib.smhv_batch_render_labels(fb._b, 0, 0, None, C.byref(opt), C.byref(lo), s) == L.E_INVALID
    assert lib.smhv_batch_render_labels(fb._b, 0, N, None, C.byref(_options(view, ow, oh, overlay=True)), C.byref(lo), s) == L.E_INVALID   # the overlay without hm
    for w, h in ((ow + 1, oh), (ow, oh - 1), (oh, ow)):            # not the most recent render's window
        assert lib.smhv_batch_render_labels(fb._b, 0, N, None, C.byref(_options(view, w, h)), C.byref(lo), s) == L.E_STATE, (w, h)
    assert lib.smhv_batch_read_labels(fb._b, 1, N, out1) == L.E_INVALID
    assert lib.smhv_batch_read_labels(fb._b, 0, 1, None) == L.E_INVALID
    for f in range(N):
        assert np.array_equal(fb.read_render(f), images[f]), f
    assert bytes(fb.read_labels(0, N)) == slab
    # the per-call path: the same checks; the image and the result stay as they were
    rect, det = current
    out = np.zeros((oh, ow, 4), np.uint8)
    res = L.LabelResult()
    for i, (lo, keep) in enumerate(bad):
        assert lib.smhv_render_map_labeled(vision._ctx, None, C.byref(opt), None, None, 0, C.byref(lo), out.ctypes.data, C.byref(res)) == L.E_INVALID, i
    lo, keep = options()
    assert lib.smhv_render_map_labeled(vision._ctx, None, C.byref(opt), None, None, 0, None, out.ctypes.data, C.byref(res)) == L.E_INVALID
    assert lib.smhv_render_map_labeled(vision._ctx, None, C.byref(opt), None, None, 0, C.byref(lo), None, C.byref(res)) == L.E_INVALID
    assert not out.any() and bytes(res) == bytes(C.sizeof(L.LabelResult))
    # a correct call follows, without a result
    assert lib.smhv_render_map_labeled(vision._ctx, None, C.byref(opt), None, None, 0, C.byref(lo), out.ctypes.data, None) == 0
    assert out.any()
    total, _ = _check_batch(vision, world, fb, s, recs, extras, True, "after the failed calls")
    assert total >= LC.ink(1, 3 * (N - 1))
