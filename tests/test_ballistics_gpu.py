"""Ballistics on the device (smhv_ballistic_lines / smhv_batch_ballistics, smhv_ballistic_map / smhv_batch_ballistic_map).  Class
bytes, the isochrone bit, the summary and the time-of-flight plane are bit-equal to the restatement (tests/ballistics_ref.py), NaN
matching NaN; painted bytes equal its blend; of a line's record everything but the two elevations is bit-equal and those lie within 4
ulps (the device's atan against the C library's).  The default weapon is tied to smhv_firing_solutions and smhv_reach_map."""
import ctypes as C
import struct

import numpy as np
import pytest

import ballistics_cases as BC
import ballistics_ref as B
import minimap_scenes as S
import reach_cases as RC
import reach_ref as R
from test_ballistics_host import ULPS, hold_solution, same_bits

pytestmark = pytest.mark.gpu

N = 3                                                             # a frame on the heightmap, a frame on the scales, a closed frame
SCENES = (0, 7, S.N_SCENES - 1)                                   # "generic", "generic, off centre" (its rectangle does not hold ORIGIN), "closed"
ORIGIN = (100.0, 150.0)
WINDOWS = ((130, 33), (65, 17))
ISO = 0.5
PALETTE = dict(pal=[(250 - 20 * k, 10 + 20 * k, 7 * k, 40 + 17 * k) for k in range(12)], iso=(3, 4, 5, 131))


def _weapon(w):
    import squad_mortar_helper_amd as smh
    return smh.Weapon(velocity=w.velocity, gravity=w.gravity, arc=("high", "low")[w.arc], unit=("mils6400", "mils6000", "degrees")[w.unit],
                      elev_min=w.elev_min, elev_max=w.elev_max, range_min=w.range_min, dispersion=w.dispersion)


def _options(viewport, window, fit=True):
    import squad_mortar_helper_amd as smh
    sw, sh, tx, ty = viewport or (1.0, 1.0, 0.0, 0.0)
    vp = smh.MapViewport((0.0, 0.0, float(window[0]), float(window[1])), (sw, sh), (tx, ty))
    return smh.render_options(vp, window[0], window[1], heightmap=False, markers=True, fit_to_minimap=fit, background=(9, 8, 7, 255))


def _view(window):
    """The 360 x 585 ROI of the scenes into the window, a scale per axis."""
    return (window[0] / 372.0, window[1] / 600.0, 1.25, -0.5)


def _same_plane(got, want, what, ctx):
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, what, got.shape, want.shape, got.dtype)
    a, b = got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want
    same = (a == b) | ((got != got) & (want != want)) if got.dtype == np.float32 else (a == b)
    if not same.all():
        bad = np.argwhere(~same)
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d elements of %s differ" % (len(bad), what), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // BC.TW, y // BC.TH),
                              "got", got[y, x].item(), "want", want[y, x].item()))


def _same_summary(res, r, ctx):
    want = B.summary(r)
    got = dict(valid=int(res.valid), source_mask=int(res.source_mask), origin=(float(res.origin[0]), float(res.origin[1])), count=[int(v) for v in res.count],
               iso=int(res.iso), n_tof=int(res.n_tof), tof_min=float(res.tof_min), tof_max=float(res.tof_max))
    assert got == want and tuple(res.reserved) == (0, 0), (ctx, got, want)
    assert same_bits(res.tof_min, want["tof_min"]) and same_bits(res.tof_max, want["tof_max"]), ctx
    assert np.array(res.origin[:], np.float32).tobytes() == np.array(want["origin"], np.float32).tobytes(), ctx


@pytest.fixture(scope="module")
def maps(vision):
    """The cases' heightmaps on the device, one copy each."""
    import squad_mortar_helper_amd as smh
    made = {}

    def get(hm):
        if hm is None:
            return None
        if id(hm[0]) not in made:
            made[id(hm[0])] = smh.Heightmap(vision, hm[0], hm[1], hm[2])
        return made[id(hm[0])]
    yield get
    for h in made.values():
        h.close()


def _per_call(vision, maps, c, paint=True, classes=True, tof=True, palette=None, seed=5):
    import squad_mortar_helper_amd as smh
    ow, oh = c.window
    opt = _options(c.viewport, c.window, c.fit)
    base = np.random.default_rng(seed).integers(0, 256, size=(oh, ow, 4)).astype(np.uint8)
    img = base.copy() if paint else None
    bo = smh.BallisticOptions(origin=c.origin, iso_s=c.iso_s, palette=palette)
    cls, tf, res = vision.ballistic_map(opt, _weapon(c.weapon), bo, mpx=c.mpx, minimap=c.minimap, heightmap=maps(c.hm), image=img, classes=classes, tof=tof)
    return base, img, cls, tf, res


@pytest.mark.parametrize("case", BC.maps(), ids=lambda c: c.name)
def test_every_map_on_the_per_call_path(vision, maps, case):
    r = BC.checked_map(case)
    base, img, cls, tf, res = _per_call(vision, maps, case, palette=PALETTE)
    _same_plane(cls, r["classes"], "class bytes", case.name)
    _same_plane(tf, r["tof"], "times of flight", case.name)
    assert np.array_equal(img, B.paint(base.copy(), r["classes"], PALETTE)), case.name
    assert np.array_equal(img[..., 3], base[..., 3])
    _same_summary(res, r, case.name)


def test_each_output_alone_and_the_default_palette(vision, maps):
    case = next(c for c in BC.maps() if c.name == "seam")
    r = BC.checked_map(case)
    base, img, cls, tf, res = _per_call(vision, maps, case, classes=False, tof=False)
    assert cls is None and tf is None and np.array_equal(img, B.paint(base.copy(), r["classes"])) and not np.array_equal(img, base)
    _same_summary(res, r, "paint alone")
    _, img, cls, tf, res = _per_call(vision, maps, case, paint=False, tof=False)
    assert img is None and tf is None
    _same_plane(cls, r["classes"], "class bytes", "classes alone")
    _, img, cls, tf, res = _per_call(vision, maps, case, paint=False, classes=False)
    assert img is None and cls is None
    _same_plane(tf, r["tof"], "times of flight", "times alone")
    _same_summary(res, r, "times alone")


# ---- the lines
def _hold_line(got, want, ctx):
    """A smhv_ballistic (ctypes) against ballistics_ref.line()'s two directions."""
    for d in (0, 1):
        if want[d] is None:
            assert bytes(got.dir[d]) == bytes(128), (ctx, d, "source NONE leaves a record of zeros")
        else:
            hold_solution(got.dir[d], want[d], (ctx, d), source=want[d]["source"])


def test_the_flat_ground_points_through_k_ballistic_lines(vision):
    """Every point with alt == 0 as the line (0, 0) - (1, 0) of a frame whose m/px is the point's range: the scales branch hands the
    kernel exactly (m, 0) for direction 0 and (m, -0) for direction 1."""
    pts = [p for p in BC.points() if p.alt == 0.0 and struct.pack("<d", p.alt) == bytes(8)]
    assert len(pts) >= 30 and sum(1 for p in pts if "T ==" in p.name) >= 4 and any(p.m == 0.0 for p in pts) and any(p.m != p.m for p in pts)
    line = np.array([[0.0, 0.0, 1.0, 0.0]], np.float32)
    for p in pts:
        got = vision.ballistic_lines(line, _weapon(p.weapon), mpx=p.m)
        for d, alt in ((0, 0.0), (1, -0.0)):
            want = B.solve(p.weapon, p.m, alt)
            hold_solution(got[0].dir[d], want, (p.name, d), source=B.SCALES)
        if "T ==" in p.name or "range_min" in p.name or "disc" in p.name:   # the decision the point is there for, on the device's own record
            p.check(p, dict(arc=[{f: getattr(got[0].dir[0].arc[i], f) for f in ("elevation", "tof", "apex", "fall", "along", "status", "band")} for i in (0, 1)],
                            cross=got[0].dir[0].cross))


@pytest.mark.parametrize("w", [BC.MORTAR, BC.ROCKET, BC.TUBE, BC.SHORT], ids=["mortar", "rocket", "tube", "short"])
def test_lines_over_terrain_and_the_tie_to_the_firing_solutions(vision, maps, w):
    sc = BC.lines_scene()
    hm = maps(sc["hm"])
    seen = set()
    for fit, viewport, mpx, minimap in ((True, None, sc["mpx"], sc["minimap"]), (False, (1.7, 0.95, -9.25, 2.5), sc["mpx"], sc["minimap"]), (True, None, None, sc["minimap"]),
                                        (True, None, sc["mpx"], None)):
        got = vision.ballistic_lines(sc["lines"], _weapon(w), mpx=mpx, minimap=minimap, heightmap=hm, fit_to_minimap=fit, viewport=viewport)
        fire = vision.firing_solutions(sc["lines"], mpx=mpx, minimap=minimap, heightmap=hm, fit_to_minimap=fit, viewport=viewport)
        for i, ln in enumerate(sc["lines"]):
            want = B.line(w, tuple(float(v) for v in ln), minimap, mpx, sc["hm"], fit, viewport)
            _hold_line(got[i], want, (i, fit, viewport, mpx))
            seen.add(int(got[i].dir[0].source))
            assert int(got[i].dir[0].source) == int(fire[i]["source"])
            if fire[i]["source"] != 0:                               # range and altitude are the firing solutions', bit for bit
                assert same_bits(got[i].dir[0].meters, fire[i]["meters"]) and same_bits(got[i].dir[0].alt_delta, fire[i]["alt_delta"]), i
                assert same_bits(got[i].dir[1].alt_delta, -float(fire[i]["alt_delta"])), i
                if w is BC.MORTAR:                                   # ... and the default weapon's high arc is its mils, on the same device
                    for d in (0, 1):
                        assert same_bits(got[i].dir[d].arc[B.HIGH].elevation, fire[i]["mils"][d]), (i, d, got[i].dir[d].arc[B.HIGH].elevation, fire[i]["mils"][d])
    assert seen == {B.NONE, B.SCALES, B.HEIGHTMAP}
    assert len(vision.ballistic_lines(np.zeros((0, 4), np.float32), _weapon(w))) == 0


def test_the_default_weapons_map_is_the_reach_map(vision, maps):
    """The class plane's reachable set equals smhv_reach_map's classes >= 2 on the same inputs, its out-of-range set the reach map's
    class 1, and nothing else appears."""
    import squad_mortar_helper_amd as smh
    for case in [c for c in BC.maps() if c.name in ("the mortar, every band", "seam", "window 130 x 33", "bounds offset", "m == 0, scales")]:
        c = case._replace(weapon=BC.MORTAR)
        _, _, cls, tf, _ = _per_call(vision, maps, c, paint=False)
        reach, _ = vision.reach_map(_options(c.viewport, c.window, c.fit), smh.ReachOptions(origin=c.origin), mpx=c.mpx, minimap=c.minimap, heightmap=maps(c.hm))
        c7 = cls & 0x7F
        assert np.array_equal(c7 >= B.C_BAND0, reach >= R.BAND0) and np.array_equal(c7 == B.C_OUT_OF_RANGE, reach == R.OUT_OF_RANGE), c.name
        assert np.array_equal(c7 == 0, reach == 0) and not ((c7 >= 2) & (c7 <= 4)).any(), c.name


# ---- batches
@pytest.fixture(scope="module")
def world(vision):
    """Three of the scenes of tests/minimap_scenes.py in a plain batch that has run once: ORIGIN lies in the first one's rectangle (the
    heightmap feeds it) and outside the second one's (the scales feed it); the third is closed."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, anchor_list, rects, names = S.make_scenes()
    frames = np.ascontiguousarray(frames[list(SCENES)])
    anchor_list, names = [anchor_list[i] for i in SCENES], [names[i] for i in SCENES]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    assert recs[0]["map_open"] and recs[1]["map_open"] and not recs[2]["map_open"] and recs[0]["n_lines"] >= 1 and recs[1]["n_lines"] >= 1
    assert recs[0]["minimap"] is not None and recs[1]["mpx"] is not None
    hm_data = RC.long_map()
    hm = smh.Heightmap(vision, *hm_data)
    w = dict(d=d, s=s, anchors=anchors, names=names, fb=fb, recs=recs, stages=stages, hm=hm, hm_data=hm_data)
    yield w
    hm.close()
    fb.close()


def _origin_of(rec, origin):
    if not rec["map_open"]:
        return None
    if isinstance(origin[0], str):
        if rec["n_lines"] <= origin[1]:
            return None
        ln = rec["lines"][origin[1]]
        return (ln[0], ln[1]) if origin[0] == "p0" else (ln[2], ln[3])
    return origin


def _want(world, rec, weapon, origin, window, fit, iso_s):
    return B.ballistic_map(weapon, _origin_of(rec, origin), window, _view(window), rec["minimap"], rec["mpx"], world["hm_data"], fit, iso_s)


def _check_batch(world, b, stream, weapon, origin, window, ctx, parts=None, fit=True, iso_s=ISO, palette=None, render=True):
    """Render, read the images, run the ballistic map (in `parts`: [(first, n)]) with every output, hold every frame against the
    restatement -> the restatements."""
    import torch
    import squad_mortar_helper_amd as smh
    ow, oh = window
    opt = _options(_view(window), window, fit)
    base = None
    if render:
        b.render(None, ow, oh, options=opt, stream=stream)
        base = [b.read_render(f).copy() for f in range(N)]
    bo = smh.BallisticOptions(origin=origin, iso_s=iso_s, paint=render, classes=True, tof=True, palette=palette)
    cls = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    tof = torch.full((N, oh, ow), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for first, n in parts or [(0, N)]:
        assert b.ballistic_map(opt, _weapon(weapon), bo, first=first, n=n, heightmap=world["hm"], classes_ptr=cls[first].data_ptr(), tof_ptr=tof[first].data_ptr(),
                               stream=stream) == {}
    res = b.read_ballistic_map(0, N)
    cls, tof = cls.cpu().numpy(), tof.cpu().numpy()
    out = []
    for f in range(N):
        r = _want(world, world["recs"][f], weapon, origin, window, fit, iso_s)
        _same_plane(cls[f], r["classes"], "class bytes", (ctx, f, world["names"][f]))
        _same_plane(tof[f], r["tof"], "times of flight", (ctx, f, world["names"][f]))
        if render:
            assert np.array_equal(b.read_render(f), B.paint(base[f].copy(), r["classes"], palette)), (ctx, f, world["names"][f])
        _same_summary(res[f], r, (ctx, f, world["names"][f]))
        out.append(r)
    assert not out[2]["valid"] and bytes(res[2]) == bytes(96)      # the closed frame: no origin, a result of zeros
    return out


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w)
def test_a_plain_batch_of_three_frames_that_differ(vision, world, window):
    fb, s = world["fb"], world["s"]
    out = _check_batch(world, fb, s, BC.SHORT, ORIGIN, window, "point", palette=PALETTE)
    assert [r["valid"] for r in out] == [1, 1, 0]
    assert (out[0]["source"] == B.HEIGHTMAP).any() and not (out[1]["source"] == B.HEIGHTMAP).any() and (out[1]["source"] == B.SCALES).any()
    print("classes per frame:", [sorted(BC._c7(r)) for r in out], "isochrone pixels:", [int(((r["classes"] & 0x80) != 0).sum()) for r in out])
    assert any((r["classes"] & B.C_ISO).any() for r in out) and len(set(c for r in out for c in BC._c7(r))) >= 3
    out0 = _check_batch(world, fb, s, BC.TUBE, ("p0", 0), window, "line p0", iso_s=0.0)
    out1 = _check_batch(world, fb, s, BC.ROCKET, ("p1", 0), window, "line p1", fit=False)
    assert [r["valid"] for r in out0] == [1, 1, 0] == [r["valid"] for r in out1] and out0[0]["origin"] != out1[0]["origin"]
    none = _check_batch(world, fb, s, BC.MORTAR, ("p0", 31), window, "line 31")
    assert not any(r["valid"] for r in none) or max(r["n_lines"] for r in world["recs"]) == 32
    assert fb.ballistic_map_ptr() != 0


def test_in_parts_and_the_lines_of_a_batch(vision, world):
    import squad_mortar_helper_amd as smh
    fb, s, recs = world["fb"], world["s"], world["recs"]
    _check_batch(world, fb, s, BC.SHORT, ORIGIN, WINDOWS[0], "parts", parts=[(1, 2), (0, 1)])
    _check_batch(world, fb, s, BC.ROCKET, ("p0", 0), WINDOWS[1], "parts, line", parts=[(0, 1), (1, 1), (2, 1)], iso_s=0.25)
    # smhv_batch_ballistics: the detected lines' records, the firing slab's numbers
    view = (1.25, 1.25, -30.0, 12.0)
    for w in (BC.MORTAR, BC.ROCKET):
        fb.ballistics(_weapon(w), first=1, n=2, heightmap=world["hm"], fit_to_minimap=False, viewport=view, stream=s)
        fb.ballistics(_weapon(w), first=0, n=1, heightmap=world["hm"], fit_to_minimap=False, viewport=view, stream=s)
        got = fb.read_ballistics(0, N)
        for f in range(N):
            rec = recs[f]
            n = rec["n_lines"]
            assert got[f].n_lines == n and tuple(got[f].reserved) == (0, 0, 0), f
            assert bytes(got[f])[16 + 256 * n:] == bytes(256 * (smh._lib.MAX_LINES - n)), (f, "lines beyond n_lines are zero")
            for i in range(n):                                     # (the record's own meters feed the scales branch, as in the firing slab)
                ln = tuple(float(v) for v in rec["lines"][i])
                fl = B.FR.firing_line(ln, rec["minimap"], float(rec["meters"][i]) if rec["mpx"] is not None else None, world["hm_data"], False, view)
                want = [None, None] if fl["source"] == B.NONE else [dict(B.solve(w, fl["meters"], a), source=fl["source"]) for a in (fl["alt_delta"], -fl["alt_delta"])]
                _hold_line(got[f].line[i], want, (f, i))
    assert fb.ballistics_ptr() != 0


def test_a_slot_of_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, N, depth=3, search=search)
        slot = p.submit(world["d"].data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"])
        p.wait()
        recs = smh.results_to_dicts(p.slots[slot].read_results(0, N))
        assert [r["n_lines"] for r in recs] == [r["n_lines"] for r in world["recs"]]
        out = _check_batch(world, p.slots[slot], p.stream_of(slot), BC.SHORT, ("p1", 0), WINDOWS[0], search)
        assert [r["valid"] for r in out] == [1, 1, 0]
        p.close()


def test_planes_without_any_render_first_use_and_paint_needs_the_window(vision, world):
    """A fresh batch: E_STATE before the family's first call; the first call covers one frame and leaves every other row of its slab
    zero; planes and summary need no render; PAINT before the first render, or at another window, is E_STATE."""
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    d, s = world["d"], world["s"]
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"], stream=s)
    window = WINDOWS[1]
    opt = _options(_view(window), window)
    for call in (lambda: fb2.read_ballistic_map(0, 1), fb2.ballistic_map_ptr, lambda: fb2.read_ballistics(0, 1), fb2.ballistics_ptr):
        with pytest.raises(smh.VisionError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    weapon = _weapon(BC.SHORT)
    fb2.ballistic_map(opt, weapon, smh.BallisticOptions(origin=ORIGIN, iso_s=ISO, paint=False), first=1, n=1, heightmap=world["hm"], stream=s)
    res = fb2.read_ballistic_map(0, N)
    assert bytes(res[0]) == bytes(96) and bytes(res[2]) == bytes(96)
    _same_summary(res[1], _want(world, world["recs"][1], BC.SHORT, ORIGIN, window, True, ISO), "the summary alone, a first call over one frame")
    fb2.ballistics(weapon, first=1, n=1, heightmap=world["hm"], stream=s)
    got = fb2.read_ballistics(0, N)
    row = C.sizeof(L.BallisticResult)
    assert bytes(got)[:row] == bytes(row) and bytes(got)[2 * row:] == bytes(row) and got[1].n_lines == world["recs"][1]["n_lines"]
    out = _check_batch(world, fb2, s, BC.SHORT, ORIGIN, window, "no render", render=False)
    assert out[0]["valid"]
    paint = smh.BallisticOptions(origin=ORIGIN, paint=True)
    with pytest.raises(smh.VisionError) as ei:
        fb2.ballistic_map(opt, weapon, paint, heightmap=world["hm"], stream=s)
    assert ei.value.code == L.E_STATE
    fb2.render(None, window[0], window[1], options=opt, stream=s)
    fb2.ballistic_map(opt, weapon, paint, heightmap=world["hm"], stream=s)
    for w, h in ((window[0] + 1, window[1]), (window[0], window[1] - 1), (window[1], window[0])):
        with pytest.raises(smh.VisionError) as ei:
            fb2.ballistic_map(_options(_view(window), (w, h)), weapon, paint, heightmap=world["hm"], stream=s)
        assert ei.value.code == L.E_STATE, (w, h)
    other = (33, 17)                                               # ... which the planes alone do not mind
    made = fb2.ballistic_map(_options(_view(other), other), weapon, smh.BallisticOptions(origin=ORIGIN, paint=False, classes=True, tof=True), first=0, n=1,
                             heightmap=world["hm"], stream=s)
    r = B.ballistic_map(BC.SHORT, ORIGIN, other, _view(other), world["recs"][0]["minimap"], world["recs"][0]["mpx"], world["hm_data"], True, 0.0)
    _same_plane(made["classes"][0].cpu().numpy(), r["classes"], "class bytes", "another window")
    _same_plane(made["tof"][0].cpu().numpy(), r["tof"], "times of flight", "another window")
    torch.cuda.synchronize()
    fb2.close()


def test_argument_errors_enqueue_nothing(vision, world):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s = world["fb"], world["s"]
    window = WINDOWS[1]
    ow, oh = window
    opt = _options(_view(window), window)
    hm = world["hm"]._hm
    fb.render(None, ow, oh, options=opt, stream=s)
    good = smh.BallisticOptions(origin=ORIGIN, iso_s=ISO, paint=True, classes=True, tof=True)
    weapon = _weapon(BC.SHORT)
    cls = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    tof = torch.full((N, oh, ow), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fb.ballistic_map(opt, weapon, good, heightmap=world["hm"], classes_ptr=cls.data_ptr(), tof_ptr=tof.data_ptr(), stream=s)
    fb.ballistics(weapon, heightmap=world["hm"], stream=s)
    images = [fb.read_render(f).copy() for f in range(N)]
    slab, lines_slab = bytes(fb.read_ballistic_map(0, N)), bytes(fb.read_ballistics(0, N))
    before = (cls.cpu().numpy().copy(), tof.cpu().numpy().copy())

    def options(**kw):
        o = good.struct()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def arms(**kw):
        w = weapon.struct()
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    nan, inf = float("nan"), float("inf")
    bad_opt = [options(size=92), options(size=100), options(size=0), options(flags=8), options(flags=0x80000007), options(origin_mode=3),
               options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=32), options(origin_mode=L.REACH_ORIGIN_LINE_P1, line=0xFFFFFFFF), options(iso_s=-1.0),
               options(iso_s=nan), options(iso_s=inf)]
    bad_arm = [arms(size=76), arms(arc=2), arms(unit=3), arms(velocity=0.0), arms(velocity=nan), arms(gravity=-1.0), arms(gravity=inf), arms(elev_min=nan),
               arms(elev_max=inf), arms(elev_min=46.0), arms(range_min=-1.0), arms(dispersion=-0.5), arms(dispersion=nan)]
    planes = L.BallisticPlanes(cls.data_ptr(), tof.data_ptr())
    pl, st, o, w = C.byref(planes), C.c_void_p(s), options(), arms()
    for i, bo in enumerate(bad_opt):
        assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(opt), C.byref(w), C.byref(bo), pl, st) == L.E_INVALID, i
    fo = L.firing_options(True, None)
    for i, bw in enumerate(bad_arm):
        assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(opt), C.byref(bw), C.byref(o), pl, st) == L.E_INVALID, i
        assert lib.smhv_batch_ballistics(fb._b, 0, N, hm, C.byref(fo), C.byref(bw), st) == L.E_INVALID, i
    assert lib.smhv_batch_ballistic_map(None, 0, N, hm, C.byref(opt), C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(opt), None, C.byref(o), pl, st) == L.E_INVALID
    assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(opt), C.byref(w), None, pl, st) == L.E_INVALID
    assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, None, C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(opt), C.byref(w), C.byref(o), None, st) == L.E_INVALID            # plane flags and no planes
    for p in (L.BallisticPlanes(None, tof.data_ptr()), L.BallisticPlanes(cls.data_ptr(), None)):                                   # a plane flag without its pointer
        assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(opt), C.byref(w), C.byref(o), C.byref(p), st) == L.E_INVALID
    assert lib.smhv_batch_ballistic_map(fb._b, 1, N, hm, C.byref(opt), C.byref(w), C.byref(o), pl, st) == L.E_INVALID              # beyond the capacity
    assert lib.smhv_batch_ballistic_map(fb._b, 0, 0, hm, C.byref(opt), C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    assert lib.smhv_batch_ballistics(fb._b, 1, N, hm, C.byref(fo), C.byref(w), st) == L.E_INVALID and lib.smhv_batch_ballistics(fb._b, 0, 0, hm, C.byref(fo), C.byref(w), st) == L.E_INVALID
    assert lib.smhv_batch_ballistics(None, 0, N, hm, C.byref(fo), C.byref(w), st) == L.E_INVALID and lib.smhv_batch_ballistics(fb._b, 0, N, hm, C.byref(fo), None, st) == L.E_INVALID
    wrong = _options(_view(window), window)
    wrong.size = 8
    assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(wrong), C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    for ww, hh in ((0, oh), (ow, 0), (16385, oh)):
        assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(_options(_view(window), (ww, hh))), C.byref(w), C.byref(o), pl, st) == L.E_INVALID, (ww, hh)
    assert lib.smhv_batch_ballistic_map(fb._b, 0, N, hm, C.byref(_options(_view(window), (ow + 1, oh))), C.byref(w), C.byref(o), pl, st) == L.E_STATE   # a stale window
    out1 = (L.BallisticMapResult * 1)()
    assert lib.smhv_batch_read_ballistic_map(fb._b, 1, N, out1) == L.E_INVALID and lib.smhv_batch_read_ballistic_map(fb._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_ballistic_map_ptr(fb._b, None) == L.E_INVALID and lib.smhv_batch_ballistics_ptr(fb._b, None) == L.E_INVALID
    torch.cuda.synchronize()
    for f in range(N):
        assert np.array_equal(fb.read_render(f), images[f]), f
    assert bytes(fb.read_ballistic_map(0, N)) == slab and bytes(fb.read_ballistics(0, N)) == lines_slab
    assert cls.cpu().numpy().tobytes() == before[0].tobytes() and tof.cpu().numpy().tobytes() == before[1].tobytes()   # (bytes: the times hold NaNs)
    # the per-call paths: the same checks, a line origin and no output besides; image, planes and result stay as they were
    img = np.full((oh, ow, 4), 77, np.uint8)
    cb = np.full((oh, ow), 0xEE, np.uint8)
    tb = np.full((oh, ow), 7.0, np.float32)
    res = L.BallisticMapResult()
    C.memset(C.byref(res), 0x5A, 96)
    args = (img.ctypes.data, cb.ctypes.data, tb.ctypes.data, C.byref(res))
    for i, bo in enumerate(bad_opt + [options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=0)]):
        assert lib.smhv_ballistic_map(vision._ctx, hm, C.byref(opt), C.byref(w), C.byref(bo), None, None, *args) == L.E_INVALID, i
    for i, bw in enumerate(bad_arm):
        assert lib.smhv_ballistic_map(vision._ctx, hm, C.byref(opt), C.byref(bw), C.byref(o), None, None, *args) == L.E_INVALID, i
    assert lib.smhv_ballistic_map(vision._ctx, hm, C.byref(opt), C.byref(w), C.byref(o), None, None, None, None, None, None) == L.E_INVALID
    assert lib.smhv_ballistic_map(None, hm, C.byref(opt), C.byref(w), C.byref(o), None, None, *args) == L.E_INVALID
    one = np.array([[1.0, 2.0, 30.0, 40.0]], np.float32)
    rec = (L.Ballistic * 1)()
    C.memset(rec, 0x5A, 256)
    for i, bw in enumerate(bad_arm):
        assert lib.smhv_ballistic_lines(vision._ctx, one.ctypes.data, 1, None, None, hm, C.byref(fo), C.byref(bw), rec) == L.E_INVALID, i
    assert lib.smhv_ballistic_lines(vision._ctx, None, 1, None, None, hm, C.byref(fo), C.byref(w), rec) == L.E_INVALID
    assert lib.smhv_ballistic_lines(vision._ctx, one.ctypes.data, 1, None, None, hm, C.byref(fo), C.byref(w), None) == L.E_INVALID
    assert (img == 77).all() and (cb == 0xEE).all() and (tb == 7.0).all() and bytes(res) == b"\x5a" * 96 and bytes(rec) == b"\x5a" * 256
    # a correct call follows, without a result
    mpx = C.c_double(2.0)
    assert lib.smhv_ballistic_map(vision._ctx, hm, C.byref(opt), C.byref(w), C.byref(o), C.byref(mpx), None, img.ctypes.data, cb.ctypes.data, tb.ctypes.data, None) == 0
    r = B.ballistic_map(BC.SHORT, ORIGIN, window, _view(window), None, 2.0, world["hm_data"], True, ISO)
    _same_plane(cb, r["classes"], "class bytes", "after the failed calls")
    _same_plane(tb, r["tof"], "times of flight", "after the failed calls")
    assert np.array_equal(img, B.paint(np.full((oh, ow, 4), 77, np.uint8), r["classes"]))
    _check_batch(world, fb, s, BC.SHORT, ORIGIN, window, "after the failed calls")


def test_the_staging_block_grown_between_calls(built):
    """A context of its own, whose pinned staging block starts empty: a small map, lines, a map forty times as large (the block grows under
    the map's layout), then the first two again -- every result the restatement's and every repeated call its first result's bytes."""
    import squad_mortar_helper_amd as smh
    v = smh.HipVision.init(0)
    hm = None
    try:
        small = next(c for c in BC.maps() if c.name == "seam")
        hm = smh.Heightmap(v, *small.hm)
        sc = BC.lines_scene()
        hm2 = smh.Heightmap(v, *sc["hm"])
        big = small._replace(name="staging, 640 x 360", window=(640, 360), viewport=(640.0 / 96.0, 360.0 / 64.0, 0.0, 0.0), origin=(293.0, 174.0))

        def run_map(c):
            r = BC.restate_map(c)
            base, img, cls, tf, res = _per_call(v, lambda h: hm, c, palette=PALETTE)
            _same_plane(cls, r["classes"], "class bytes", c.name)
            _same_plane(tf, r["tof"], "times of flight", c.name)
            assert np.array_equal(img, B.paint(base.copy(), r["classes"], PALETTE)), c.name
            _same_summary(res, r, c.name)
            return [img.tobytes(), cls.tobytes(), tf.tobytes(), bytes(res)]

        def run_lines():
            got = v.ballistic_lines(sc["lines"], _weapon(BC.TUBE), mpx=sc["mpx"], minimap=sc["minimap"], heightmap=hm2)
            for i, ln in enumerate(sc["lines"]):
                _hold_line(got[i], B.line(BC.TUBE, tuple(float(x) for x in ln), sc["minimap"], sc["mpx"], sc["hm"]), i)
            return [bytes(got)]
        first = [run_map(small), run_lines()]
        run_map(big)
        again = [run_map(small), run_lines()]
        assert first == again
        hm2.close()
    finally:
        if hm is not None:
            hm.close()
        v.shutdown()
