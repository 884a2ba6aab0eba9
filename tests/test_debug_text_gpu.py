"""The vision debugger and the debug text on the device (smhv_batch_probe / smhv_batch_render_debug / smhv_render_map_debug), every
comparison exact: a probe byte-equal to the restatement's (tests/debug_text_ref.py) of the ui_map the batch or the context holds; the
image equal to the restatement's pass over the image of the same call without it, byte for byte; and every drawing case changes
at least the pixels its claims stand for (tests/debug_text_cases.py), or none."""
import ctypes as C

import numpy as np
import pytest

import debug_text_cases as DC
import debug_text_ref as R
import label_cases as LC
import minimap_scenes as S
import render_geometry_cases as G

pytestmark = pytest.mark.gpu

BG = G.BG
RW, RH = 360, 585                                                # the map ROI of the scenes' frames (asserted by the fixtures)
NF = 4                                                           # frames of a batch here: two open scenes, the closed one, one more open
CLOSED = 2
CONSTS = R.load_consts()


def _vp(view):
    import squad_mortar_helper_amd as smh
    return smh.MapViewport(view.quad, view.scale, view.top_left)


def _options(view, ow, oh, markers=False):
    import squad_mortar_helper_amd as smh
    return smh.render_options(_vp(view), ow, oh, markers=markers, background=BG)


def _debug(case_or_runs, points=(), flags=0, scale=0):
    import squad_mortar_helper_amd as smh
    if isinstance(case_or_runs, DC.Case):
        c = case_or_runs
        return _debug(c.runs, c.points, c.flags, c.S)
    do = smh.DebugOptions(draw_probes=bool(flags & R.DRAW_PROBES), minimap_caption=bool(flags & R.MINIMAP_CAPTION), scale=scale)
    do.runs, do.probes = list(case_or_runs), [(float(x), float(y)) for x, y in points]
    return do


def _pack(p):
    from squad_mortar_helper_amd import _lib as L
    q = L.Probe()
    q.valid, q.px, q.py, q.luma, q.h, q.s, q.v, q.mono, q.brightness, q.team_bits = (p["valid"], p["px"], p["py"], p["luma"], p["h"], p["s"], p["v"], p["mono"],
                                                                                      p["brightness"], p["team_bits"])
    for k in range(3):
        q.rgb[k] = p["rgb"][k]
    return bytes(q)


def _same_probes(got, want, n_points, ctx):
    """got: MAX_PROBES device entries of one frame; want: the restatement's dicts."""
    for k in range(R.MAX_PROBES):
        w = _pack(want[k]) if k < n_points else bytes(32)
        assert bytes(got[k]) == w, (ctx, "probe %d" % k, [getattr(got[k], f) for f in ("valid", "px", "py", "h", "s", "v", "mono", "team_bits")],
                                    want[k] if k < n_points else None)


def _same(got, want, ctx):
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=2))
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d pixels differ" % len(bad), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // DC.TW, y // DC.TH),
                              "got", got[y, x].tolist(), "want", want[y, x].tolist()))


def _frames():
    """Four frames of tests/minimap_scenes.py: scenes 0 and 1, the closed one, scene 3 -- with the threshold colours painted on
    one ROI row of every open frame, and the ROI's first and last pixel in colours of their own."""
    frames, anchor_list, rects, names = S.make_scenes()
    pick = [0, 1, S.N_SCENES - 1, 3]
    frames = np.ascontiguousarray(frames[pick])
    x0, y0, rw, rh = S.roi()
    assert (rw, rh) == (RW, RH)
    colours = DC.threshold_colours(CONSTS)
    cells = DC.cells(len(colours))
    assert 42 < cells[0][0] and cells[-1][0] < rw // 2 - 12        # clear of the scenes' stripes (columns 40 .. 42, 168 and up): the rectangles stay
    for f in range(NF):
        if f == CLOSED:
            continue
        for (cx, cy), (_, (r, g, b), _) in zip(cells, colours):
            frames[f, y0 + cy, x0 + cx] = (b, g, r, 255)
        frames[f, y0, x0] = (3, 250, 99, 255)
        frames[f, y0 + rh - 1, x0 + rw - 1] = (240, 7, 130, 255)
    return frames, [anchor_list[i] for i in pick], [rects[i] for i in pick], cells, colours


@pytest.fixture(scope="module")
def world(vision):
    """The four frames in a plain batch that has run once in colour with every stage and the minimap."""
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    frames, anchor_list, rects, cells, colours = _frames()
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    fb = smh.FrameBatch(vision, S.W, S.H, NF)
    assert tuple(fb.roi[2:]) == (RW, RH)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb.run(d.data_ptr(), NF, stages=stages, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, NF))
    assert [bool(r["map_open"]) for r in recs] == [f != CLOSED for f in range(NF)]
    assert all(r["minimap"] is not None for f, r in enumerate(recs) if f != CLOSED)
    ui = [fb.read_image(L.IMAGE_UI_MAP, f).copy() for f in range(NF)]
    for (cx, cy), (_, c, _) in zip(cells, colours):
        assert tuple(int(v) for v in ui[0][cy, cx, :3]) == c
    w = dict(frames=frames, d=d, s=s, anchors=anchors, rects=rects, fb=fb, recs=recs, stages=stages, ui=ui, cells=cells, colours=colours)
    yield w
    fb.close()


@pytest.fixture(scope="module")
def current(vision, world):
    """Frame 0 as the current frame of the per-call path -> (its ui_map, detected lines)."""
    vision.load_frame(world["frames"][0])
    got = vision.crop_to_map(grayscale=False)
    assert got is not None
    ui = got[0].copy()
    assert np.array_equal(ui, world["ui"][0])
    assert vision.find_minimap() == world["rects"][0]
    vision.isolate_map_markers()
    vision.mask_marker_lines()
    lines = vision.find_marker_lines(15)
    return ui, lines


# ---- the probe ------------------------------------------------------------------------------------------------------------------
def _probe_batch(world, fb, stream, ui, open_, view, ctx):
    """Every threshold colour, the ROI's corners, its edges, negative, NaN and FLT_MAX positions, seven cells a call."""
    cells = world["cells"]
    opt = _options(view, 64, 32)
    seen_bits = set()
    for at in range(0, len(cells), 7):
        pts = DC.probe_points(view, RW, RH, cells[at:at + 7])
        fb.probe(opt, pts, stream=stream)
        got = fb.read_probes(0, NF)
        for f in range(NF):
            want = [R.probe(ui[f], open_[f], pt, view.scale, view.top_left, CONSTS) for pt in pts]
            _same_probes(got[f * R.MAX_PROBES:(f + 1) * R.MAX_PROBES], want, len(pts), (ctx, at, f))
            if open_[f]:
                # the positions do what they are there for
                assert [w["valid"] for w in want[:9]] == [1, 1, 0, 0, 0, 0, 1, 0, 0], (ctx, [w["valid"] for w in want[:9]])
                assert (want[0]["px"], want[0]["py"], want[1]["px"], want[1]["py"], want[6]["px"], want[6]["py"]) == (0, 0, RW - 1, RH - 1, 0, 7)
                for (cx, cy), w in zip(cells[at:at + 7], want[9:]):
                    assert (w["valid"], w["px"], w["py"]) == (1, cx, cy), (ctx, cx, cy, w)
                    seen_bits.add(w["team_bits"])
            else:
                assert all(w == R.ZERO_PROBE for w in want)
    return seen_bits


@pytest.mark.parametrize("name", ["identity", "zoomed", "sw < 1"])
def test_batch_probe_round_every_threshold_under_three_viewports(vision, world, name):
    fb, s = world["fb"], world["s"]
    view = DC.probe_views(RW, RH)[name]
    open_ = [f != CLOSED for f in range(NF)]
    seen = _probe_batch(world, fb, s, world["ui"], open_, view, name)
    assert len(seen) >= 12                                          # the colours tell the nine bits apart
    assert fb.probes_ptr() != 0
    # the colours are what the ui_map holds: a threshold colour probes as its own (h, s, v)
    pts = DC.probe_points(view, RW, RH, world["cells"][:7])
    fb.probe(_options(view, 64, 32), pts, first=1, n=1, stream=s)   # ... and a call over one frame leaves the others' entries alone
    got = fb.read_probes(0, NF)
    for (what, c, hsv), p in zip(world["colours"][:7], got[R.MAX_PROBES + 9:R.MAX_PROBES + 16]):
        assert (tuple(p.rgb), (p.h, p.s, p.v)) == (c, hsv), what


def test_probe_after_a_grayscale_run_and_state_errors(vision, world):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    d, s = world["d"], world["s"]
    fb2 = smh.FrameBatch(vision, S.W, S.H, NF)
    view = DC.probe_views(RW, RH)["zoomed"]
    opt = _options(view, 64, 32)
    pts = DC.probe_points(view, RW, RH, world["cells"][:7])
    arr = (L.ProbePoint * 16)()
    out = (L.Probe * (16 * NF))()
    # before any run: no ui_map; before any probe: no slab
    assert lib.smhv_batch_probe(fb2._b, 0, NF, C.byref(opt), arr, 1, s) == L.E_STATE
    assert lib.smhv_batch_read_probes(fb2._b, 0, NF, out) == L.E_STATE and lib.smhv_batch_probes_ptr(fb2._b, C.byref(C.c_void_p())) == L.E_STATE
    fb2.run(d.data_ptr(), NF, stages=smh.STAGE_UI_MAP, grayscale=True, anchors=None, stream=s)
    assert lib.smhv_batch_read_probes(fb2._b, 0, NF, out) == L.E_STATE
    for bad in ((0, 0, opt, arr, 1), (1, NF, opt, arr, 1), (0, NF, None, arr, 1), (0, NF, opt, arr, 17), (0, NF, opt, None, 1)):
        first, n, o, a, k = bad
        assert lib.smhv_batch_probe(fb2._b, first, n, C.byref(o) if o is not None else None, a, k, s) == L.E_INVALID, bad[:2] + bad[4:]
    small = _options(view, 64, 32)
    small.size = 8
    assert lib.smhv_batch_probe(fb2._b, 0, NF, C.byref(small), arr, 1, s) == L.E_INVALID
    assert lib.smhv_batch_read_probes(fb2._b, 0, NF, out) == L.E_STATE                 # the failed calls enqueued and allocated nothing
    ui = [fb2.read_image(L.IMAGE_UI_MAP, f).copy() for f in range(NF)]
    assert all(np.array_equal(ui[f][..., 0], ui[f][..., 1]) and np.array_equal(ui[f][..., 0], ui[f][..., 2]) for f in range(NF))
    fb2.probe(opt, pts, stream=s)
    got = fb2.read_probes(0, NF)
    for f in range(NF):
        want = [R.probe(ui[f], f != CLOSED, pt, view.scale, view.top_left, CONSTS) for pt in pts]
        _same_probes(got[f * 16:(f + 1) * 16], want, len(pts), ("gray", f))
        if f != CLOSED:
            # gray bytes: no chroma; the f32 luma of (L, L, L) may truncate to L - 1
            assert all(w["mono"] == 0 and w["s"] == 0 and w["rgb"][0] == w["rgb"][1] == w["rgb"][2] == w["brightness"] and w["rgb"][0] - w["luma"] in (0, 1)
                       for w in want if w["valid"])
    # no points at all: the slab is zeroed
    fb2.probe(opt, [], stream=s)
    assert bytes(fb2.read_probes(0, NF)) == bytes(32 * 16 * NF)
    fb2.close()


# ---- the per-call path: every case ------------------------------------------------------------------------------------------------
def _call(vision, ui, case, lines=None, labels=None, layers=None):
    """One per-call render with the debug pass against the same call without it -> (base, got, pixels changed on the restatement,
    the restatement's items and probes)."""
    ow, oh = case.window
    det = np.zeros((0, 4), np.float32) if lines is None else np.asarray(lines, np.float32).reshape(-1, 4)
    opt = _options(case.view, ow, oh, markers=len(det) > 0)
    base = vision.render_map(_vp(case.view), ow, oh, lines=det, options=opt, layers=layers, labels=labels)
    base = base[0] if labels is not None else base
    got, res, probes = vision.render_map(_vp(case.view), ow, oh, lines=det, options=opt, layers=layers, labels=labels, debug=_debug(case))
    S_ = case.S or 2
    item_list, want_probes = R.items(ui, True, True, case.runs, case.points, case.flags, S_, ow, oh, case.view.scale, case.view.top_left, CONSTS)
    want = base.copy()
    n = R.draw(want, item_list, S_)
    _same(got, want, case)
    _same_probes(probes, want_probes, len(case.points), case)
    return base, got, n, item_list, want_probes


@pytest.mark.parametrize("case", DC.all_cases(RW, RH), ids=lambda c: c.name)
def test_every_case_on_the_per_call_path(vision, world, current, case):
    """Runs across tile corners and borders at S = 1 .. 4, cut by each edge, eight lines, one character, 64 on one spot, map and
    window anchors, anchors that are not finite; probe windows that stay, flip at either edge and at both, and lie partly outside;
    the pixel frame at floorf(sw) = 0 .. 3; sixteen probes."""
    ui, _ = current
    base, got, n, item_list, probes = _call(vision, ui, case)
    minimum = DC.minimum_of(case, base, item_list, probes)
    if minimum is None:
        assert n == 0 and np.array_equal(got, base)
    else:
        assert n >= minimum, (case, n, minimum)
    if case.name.startswith("stack"):
        changed = np.any(got != base, axis=2)
        assert np.all(got[changed] == np.array(case.runs[-1][2], np.uint8))


def test_over_layers_and_labels_and_the_identities(vision, world, current):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    ui, det = current
    case = DC.tile_cases(RW, RH)[1]
    case = DC.Case("over layers and labels", case.window, DC.view_at(RW, RH, world["cells"][20], 100.5, 200.5), 2, case.runs[:3] + [DC.run(420, 250, "x")],
                   [(100.5, 200.5)], R.DRAW_PROBES | R.MINIMAP_CAPTION, claim_runs=(3,), claim_probes=(0,), partly_outside=True)
    prims = [smh.prim(20, 20, 300, 200, (1, 2, 3, 255), L.PRIM_RECT | L.PRIM_FOREGROUND), smh.prim(0, 64, 600, 64, (250, 250, 0, 255), L.PRIM_LINE)]
    extras = [LC._line(case.view, 150.0, 100.0, 4.0, 90.0, LC.CYAN)]
    plain = vision.render_map(_vp(case.view), *case.window, options=_options(case.view, *case.window))
    for layers, labels in ((smh.RenderLayers(prims, minimap_bounds=True), smh.LabelOptions(extras, detected=True, scale=1, mpx=0.8372)),
                           (smh.RenderLayers(prims), None), (None, smh.LabelOptions(extras, detected=False, scale=2, mpx=0.8372)), (None, None)):
        base, got, n, item_list, probes = _call(vision, ui, case, lines=det[:8], labels=labels, layers=layers)
        assert n >= DC.minimum_of(case, base, item_list, probes)
        assert not np.array_equal(base, plain)                     # the lines, the layers and the labels are there under the pass
        # the context's frame has a rectangle: no caption (the only red the pass could paint)
        assert not any(it[0] == "text" and it[2] == R.CAPTION_RED for it in item_list)
        # identity: no runs, no probes, no flags -- that call's image, byte for byte
        nothing = DC.Case("nothing", case.window, case.view, 0, nothing=True)
        base2, got2, n2, _, _ = _call(vision, ui, nothing, lines=det[:8], labels=labels, layers=layers)
        assert n2 == 0 and np.array_equal(got2, base2) and np.array_equal(base2, base)
    # the labels' result comes back with the image
    lo = smh.LabelOptions(extras, detected=False, scale=2, mpx=0.8372)
    _, res0 = vision.render_map(_vp(case.view), *case.window, options=_options(case.view, *case.window), labels=lo)
    _, res1, _ = vision.render_map(_vp(case.view), *case.window, options=_options(case.view, *case.window), labels=lo, debug=_debug(case))
    assert bytes(res0) == bytes(res1) and res1.n_labels == 1
    # HipVision.probe: the numbers alone
    pts = DC.probe_points(case.view, RW, RH, world["cells"][:7])
    got = vision.probe(_vp(case.view), pts)
    _same_probes(got, [R.probe(ui, True, pt, case.view.scale, case.view.top_left, CONSTS) for pt in pts], len(pts), "HipVision.probe")


# ---- the batch call ---------------------------------------------------------------------------------------------------------------
def _batch_case():
    """Runs on tile corners, two probes whose windows flip (the first lies partly outside and under the second), the caption;
    window 640 x 360, the map at the whole-window scales with painted cell 3 under the second probe."""
    sw, sh = 640 / RW, 360 / RH
    view = DC.view_at(RW, RH, DC.cells(4)[3], 600.0, 200.0, sw, sh)
    runs = [DC.run(64 - 9, 32 - 4, "Ag[%]"), DC.run(100, 60, "map", DC.AMBER, True), DC.run(500, 300, "{0}", DC.MINT)]
    return DC.Case("batch", (640, 360), view, 1, runs, [(560.5, 100.25), (600.0, 200.0)], R.DRAW_PROBES | R.MINIMAP_CAPTION, claim_runs=(0, 2), claim_probes=(1,))


def _check_batch(world, b, stream, ui, recs, case, ctx, parts=None, before=None):
    """Render, (before: more passes), read the images, run the debug pass (in `parts`: [(first, n)]), and hold every frame's image
    and probes against the restatement -> pixels changed in all frames."""
    ow, oh = case.window
    opt = _options(case.view, ow, oh, markers=True)
    b.render(_vp(case.view), ow, oh, options=opt, stream=stream)
    if before is not None:
        before(b, opt, stream)
    base = [b.read_render(f).copy() for f in range(NF)]
    for first, n in parts or [(0, NF)]:
        b.render_debug(opt, _debug(case), first=first, n=n, stream=stream)
    probes = b.read_probes(0, NF)
    total = 0
    S_ = case.S or 2
    for f in range(NF):
        got = b.read_render(f)
        open_ = bool(recs[f]["map_open"])
        item_list, want_probes = R.items(ui[f], open_, recs[f]["minimap"] is not None, case.runs, case.points, case.flags, S_, ow, oh, case.view.scale,
                                         case.view.top_left, CONSTS)
        want = base[f].copy()
        n = R.draw(want, item_list, S_)
        _same(got, want, (ctx, f))
        _same_probes(probes[f * 16:(f + 1) * 16], want_probes, len(case.points), (ctx, f))
        if not open_:
            assert n == 0 and np.all(got == np.array(BG, np.uint8)), (ctx, f)
            continue
        minimum = DC.minimum_of(case, base[f], item_list, want_probes)
        if minimum is None:
            assert n == 0 and np.array_equal(got, base[f]), (ctx, f, n)
        else:
            assert n >= minimum, (ctx, f, n, minimum)
        total += n
    return total


@pytest.fixture(scope="module")
def targets(vision, world):
    """Where the batch call runs: a plain batch whose frames 0 and 1 have a minimap rectangle and whose frame 3 has none (all four
    ran without the minimap stage, then the first two with it), and a slot of a pipeline of either search schedule
    -> name: (batch, stream, ui_maps, records)."""
    import squad_mortar_helper_amd as smh
    L = smh._lib
    d, s, anchors = world["d"], world["s"], world["anchors"]
    fb = smh.FrameBatch(vision, S.W, S.H, NF)
    fb.run(d.data_ptr(), NF, stages=smh.STAGE_ALL, grayscale=False, anchors=anchors, stream=s)
    fb.run(d.data_ptr(), 2, stages=world["stages"], grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, NF))
    assert [r["minimap"] is not None for r in recs] == [True, True, False, False] and recs[3]["map_open"] and not recs[CLOSED]["map_open"]
    out = {"plain batch": (fb, s, [fb.read_image(L.IMAGE_UI_MAP, f).copy() for f in range(NF)], recs)}
    pipes = []
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, NF, depth=3, search=search)
        slot = p.submit(d.data_ptr(), NF, stages=world["stages"], grayscale=False, anchors=anchors)
        p.wait()
        out[search + " pipeline"] = (p.slots[slot], p.stream_of(slot), world["ui"], world["recs"])
        pipes.append(p)
    yield out
    for p in pipes:
        p.close()
    fb.close()


@pytest.mark.parametrize("where", ["plain batch", "batch pipeline", "frame pipeline"])
@pytest.mark.parametrize("case", DC.all_cases(RW, RH), ids=lambda c: c.name)
def test_every_case_through_the_batch_call(vision, world, targets, case, where):
    """Every drawing case over four frames in one launch -- two scenes with a rectangle, the closed frame, a scene that has no
    rectangle on the plain batch -- each frame's image and probes against the restatement and the case's minimum."""
    b, stream, ui, recs = targets[where]
    parts = [(0, 1), (1, NF - 1)] if case.name.startswith(("tiles, S = 3", "sixteen")) else None
    assert _check_batch(world, b, stream, ui, recs, case, (where, case.name), parts=parts) >= 0
    if case.name.startswith("64 runs") and where == "plain batch":
        # frame 3 has no rectangle: 129 items, the caption among them
        ow, oh = case.window
        got = b.read_render(3)
        red = np.all(got[oh - 19:oh - 10] == np.array(R.CAPTION_RED + (255,), np.uint8), axis=2)
        assert int(red.sum()) >= 5 * DC.ink_of(R.CAPTION) and not np.any(np.all(b.read_render(0)[oh - 19:oh - 10] == np.array(R.CAPTION_RED + (255,), np.uint8), axis=2))


def test_the_batch_call_on_a_plain_batch_in_parts_and_on_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    fb, d, s, anchors, recs, ui = (world[k] for k in ("fb", "d", "s", "anchors", "recs", "ui"))
    case = _batch_case()
    assert _check_batch(world, fb, s, ui, recs, case, "plain batch") > 0
    assert _check_batch(world, fb, s, ui, recs, case, "two parts", parts=[(0, 1), (1, NF - 1)]) > 0
    assert _check_batch(world, fb, s, ui, recs, case, "two parts, backwards", parts=[(3, 1), (0, 3)]) > 0
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, NF, depth=3, search=search)
        slot = p.submit(d.data_ptr(), NF, stages=world["stages"], grayscale=False, anchors=anchors)
        p.wait()
        assert _check_batch(world, p.slots[slot], p.stream_of(slot), ui, recs, case, search) > 0
        p.close()


def test_the_caption_on_frames_without_a_rectangle_and_the_pass_over_layers_and_labels(vision, world):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    d, s, anchors = world["d"], world["s"], world["anchors"]
    fb2 = smh.FrameBatch(vision, S.W, S.H, NF)
    # all four without the minimap stage, then the first two with it: frames 0 and 1 have a rectangle, frame 3 has none
    fb2.run(d.data_ptr(), NF, stages=smh.STAGE_ALL, grayscale=False, anchors=anchors, stream=s)
    fb2.run(d.data_ptr(), 2, stages=world["stages"], grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb2.read_results(0, NF))
    assert [r["minimap"] is not None for r in recs] == [True, True, False, False] and recs[3]["map_open"]
    ui = [fb2.read_image(L.IMAGE_UI_MAP, f).copy() for f in range(NF)]
    for S_ in (1, 2):
        view = G.window_view(RW, RH, 640, 360)                    # the whole map across the window
        case = DC.Case("caption", (640, 360), view, S_, [DC.run(10, 10, "S = %d" % S_)], [], R.MINIMAP_CAPTION, claim_runs=(0,))
        ow, oh = case.window
        opt = _options(view, ow, oh, markers=True)
        fb2.render(_vp(view), ow, oh, options=opt, stream=s)
        base = [fb2.read_render(f).copy() for f in range(NF)]
        fb2.render_debug(opt, _debug(case), stream=s)
        red = np.array(R.CAPTION_RED + (255,), np.uint8)
        for f in range(NF):
            got = fb2.read_render(f)
            want = base[f].copy()
            n, _ = R.debug_pass(want, ui[f], bool(recs[f]["map_open"]), recs[f]["minimap"] is not None, case.runs, [], case.flags, S_, view.scale, view.top_left, CONSTS)
            _same(got, want, ("caption", S_, f))
            band = got[oh - 10 - 9 * S_:oh - 10]
            painted = int((np.all(band == red, axis=2) & np.any(band != base[f][oh - 10 - 9 * S_:oh - 10], axis=2)).sum())
            if f == 3:                                             # 58 characters, 49 of them ink; at S = 2 the window cuts the line after 105 columns
                inside = DC.ink_of(R.CAPTION[:min(58, (ow - 10) // (6 * S_))])
                assert painted >= 5 * S_ * S_ * inside and n >= painted + 5 * S_ * S_ * DC.ink_of(case.runs[0][4]), (S_, painted, n)
            else:
                assert painted == 0, (S_, f)

    # over a layers + labels image: the restatement of this pass over the device's image of the two passes before it
    def before(b, opt, stream):
        prims = [smh.prim(20, 20, 300, 200, (1, 2, 3, 255), L.PRIM_RECT | L.PRIM_FOREGROUND), smh.prim(0, 64, 350, 500, (250, 250, 0, 255), L.PRIM_LINE)]
        plain = [b.read_render(f).copy() for f in range(NF)]
        b.render(None, 0, 0, options=opt, layers=smh.RenderLayers(prims, minimap_bounds=True), stream=stream)
        layered = [b.read_render(f).copy() for f in range(NF)]
        b.render_labels(opt, smh.LabelOptions([LC._line(opt_view, 320.0, 150.0, 10.0, 120.0, LC.CYAN)], detected=True, scale=1), stream=stream)
        labelled = [b.read_render(f).copy() for f in range(NF)]
        for f in (0, 1, 3):
            assert not np.array_equal(plain[f], layered[f]) and not np.array_equal(layered[f], labelled[f]), f
    case = _batch_case()
    opt_view = case.view
    assert _check_batch(world, fb2, s, ui, recs, case, "over layers and labels", before=before) > 0
    # with nothing to draw the images stay, byte for byte, and the probes are still written
    nothing = DC.Case("nothing", case.window, case.view, 0, [], case.points, 0, nothing=True)
    opt = _options(case.view, *case.window, markers=True)
    images = [fb2.read_render(f).copy() for f in range(NF)]
    fb2.render_debug(opt, _debug(nothing), stream=s)
    for f in range(NF):
        assert np.array_equal(fb2.read_render(f), images[f]), f
    got = fb2.read_probes(0, NF)
    assert got[0].valid == 1 and got[R.MAX_PROBES * CLOSED].valid == 0 and got[R.MAX_PROBES * 3 + 1].valid == 1
    fb2.close()


def test_argument_errors_leave_the_images_and_the_probe_slab_unchanged(vision, world, current):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s, d = world["fb"], world["s"], world["d"]
    case = _batch_case()
    ow, oh = case.window
    opt = _options(case.view, ow, oh, markers=True)
    # before any render: SMHV_E_STATE
    fb0 = smh.FrameBatch(vision, S.W, S.H, 2)
    fb0.run(d.data_ptr(), 2, stages=smh.STAGE_UI_MAP, grayscale=True, anchors=None, stream=s)
    good, keep = _debug(case).struct()
    assert lib.smhv_batch_render_debug(fb0._b, 0, 2, C.byref(opt), C.byref(good), s) == L.E_STATE
    assert lib.smhv_batch_read_probes(fb0._b, 0, 1, (L.Probe * 16)()) == L.E_STATE
    fb0.close()

    fb.render(_vp(case.view), ow, oh, options=opt, stream=s)
    fb.render_debug(opt, _debug(case), stream=s)
    images = [fb.read_render(f).copy() for f in range(NF)]
    slab = bytes(fb.read_probes(0, NF))

    def options(runs=None, **kw):
        do, keep = _debug(runs if runs is not None else case.runs, case.points, case.flags, 1).struct()
        for k, v in kw.items():
            setattr(do, k, v)
        return do, keep
    bad = [options(size=32), options(size=48), options(flags=4), options(scale=5), options(n_runs=65), options(n_probes=17),
           options(runs=[DC.run(0, 0, "a", (1, 2, 3, 254))]), options(runs=[DC.run(0, 0, "1\n2\n3\n4\n5\n6\n7\n8\n9")]), options(runs=[DC.run(0, 0, b"caf\xe9")]),
           options(runs=[(0.0, 0.0, (1, 2, 3, 255), 2, b"flag")]), options(runs=[DC.run(0, 0, "a")] * 65)]
    do, keep1 = options()
    do.runs = None
    bad.append((do, keep1))
    do, keep2 = options()
    do.probes = None
    bad.append((do, keep2))
    for i, (do, _) in enumerate(bad):
        assert lib.smhv_batch_render_debug(fb._b, 0, NF, C.byref(opt), C.byref(do), s) == L.E_INVALID, i
    do, keep3 = options()
    assert lib.smhv_batch_render_debug(fb._b, 0, NF, C.byref(opt), None, s) == L.E_INVALID
    assert lib.smhv_batch_render_debug(fb._b, 0, NF, None, C.byref(do), s) == L.E_INVALID
    assert lib.smhv_batch_render_debug(fb._b, 1, NF, C.byref(opt), C.byref(do), s) == L.E_INVALID      # beyond the capacity
    assert lib.smhv_batch_render_debug(fb._b, 0, 0, C.byref(opt), C.byref(do), s) == L.E_INVALID
    wrong = _options(case.view, ow, oh)
    wrong.size = 40
    assert lib.smhv_batch_render_debug(fb._b, 0, NF, C.byref(wrong), C.byref(do), s) == L.E_INVALID
    for w, h in ((ow + 1, oh), (ow, oh - 1), (oh, ow)):            # not the most recent render's window
        assert lib.smhv_batch_render_debug(fb._b, 0, NF, C.byref(_options(case.view, w, h)), C.byref(do), s) == L.E_STATE, (w, h)
    for f in range(NF):
        assert np.array_equal(fb.read_render(f), images[f]), f
    assert bytes(fb.read_probes(0, NF)) == slab
    # the per-call path: the same checks; the image stays as it was
    out = np.zeros((oh, ow, 4), np.uint8)
    probes = (L.Probe * 16)()
    for i, (do, _) in enumerate(bad):
        assert lib.smhv_render_map_debug(vision._ctx, None, C.byref(opt), None, None, 0, None, C.byref(do), out.ctypes.data, None, probes) == L.E_INVALID, i
    assert lib.smhv_render_map_debug(vision._ctx, None, C.byref(opt), None, None, 0, None, None, out.ctypes.data, None, probes) == L.E_INVALID
    do, keep4 = options()
    assert lib.smhv_render_map_debug(vision._ctx, None, C.byref(opt), None, None, 0, None, C.byref(do), None, None, probes) == L.E_INVALID
    assert not out.any() and bytes(probes) == bytes(32 * 16)
    # a correct call follows
    assert lib.smhv_render_map_debug(vision._ctx, None, C.byref(opt), None, None, 0, None, C.byref(do), out.ctypes.data, None, probes) == 0
    assert out.any() and probes[0].valid == 1
    assert _check_batch(world, fb, s, world["ui"], world["recs"], case, "after the failed calls") > 0
