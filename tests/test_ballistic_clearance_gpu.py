"""Ballistic clearance on the device (smhv_ballistic_clearance_lines / smhv_batch_ballistic_clearance, smhv_ballistic_clearance_map /
smhv_batch_ballistic_clearance_map).  Records, class bytes, the margin plane (NaN matching NaN) and summaries are bit-equal to the
restatement (tests/ballistic_clearance_ref.py); painted bytes equal its blend.  The default weapon's high arc is tied to
smhv_clearance_lines / smhv_clearance_map, every line's range, altitude and status bits to smhv_ballistic_lines."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ballistic_clearance_cases as K
import ballistic_clearance_ref as R
import ballistics_ref as B
import clearance_cases as CC
import minimap_scenes as S
from test_ballistic_clearance_host import bad_options, hold_dir
from test_ballistics_host import same_bits

pytestmark = pytest.mark.gpu

N = 3                                                             # a frame on the heightmap, a frame on the scales, a closed frame
SCENES = (0, 7, S.N_SCENES - 1)                                   # "generic", "generic, off centre" (its rectangle does not hold ORIGIN), "closed"
ORIGIN = (100.0, 150.0)
WINDOWS = ((130, 33), (65, 17))
LINE_VIEW = (1.5, 0.75, -6.0, 2.0)                                # the viewport the batch's lines are asked at
PALETTE = dict(pal=[(250, 10, 20, 255), (10, 200, 30, 90), (3, 4, 5, 131), (200, 100, 0, 60)], switch_arc=(90, 0, 200, 77), los=(7, 8, 9, 33))


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
    if got.dtype == np.float32:
        same = (got.view(np.uint32) == want.view(np.uint32)) | ((got != got) & (want != want))
    else:
        same = got == want
    if not same.all():
        bad = np.argwhere(~same)
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d elements of %s differ" % (len(bad), what), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // K.TW, y // K.TH),
                              "got", got[y, x].item(), "want", want[y, x].item()))


def _same_summary(res, r, ctx):
    want = R.summary(r)
    got = dict(valid=int(res.valid), origin=(float(res.origin[0]), float(res.origin[1])), own=[int(v) for v in res.own], other=[int(v) for v in res.other],
               los_blocked=int(res.los_blocked), switch_arc=int(res.switch_arc))
    assert got == want and res.reserved0 == 0 and tuple(res.reserved) == (0, 0), (ctx, got, want)
    assert np.array(res.origin[:], np.float32).tobytes() == np.array(want["origin"], np.float32).tobytes(), ctx


def _same_lines(out, recs, ctx):
    assert len(out) == len(recs)
    for i, (rec, (fwd, bck)) in enumerate(zip(out, recs)):
        hold_dir(rec.dir[0], fwd, (ctx, i, 0))
        hold_dir(rec.dir[1], bck, (ctx, i, 1))


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


def _lines_call(vision, maps, c, margin=None, weapon=None):
    import squad_mortar_helper_amd as smh
    co = smh.BallisticClearanceOptions(samples=c.samples, margin_m=c.margin if margin is None else margin)
    return vision.ballistic_clearance_lines(np.array(c.lines, np.float32).reshape(-1, 4), _weapon(weapon or c.weapon), co, minimap=c.minimap, heightmap=maps(c.hm),
                                            fit_to_minimap=c.fit, viewport=c.viewport)


def _map_call(vision, maps, c, paint=True, want_bytes=True, want_margin=True, palette=PALETTE, weapon=None, seed=5):
    import squad_mortar_helper_amd as smh
    ow, oh = c.window
    base = np.random.default_rng(seed).integers(0, 256, size=(oh, ow, 4)).astype(np.uint8)
    img = base.copy() if paint else None
    co = smh.BallisticClearanceOptions(samples=c.samples, margin_m=c.margin, origin=c.origin, palette=palette)
    b, m, res = vision.ballistic_clearance_map(_options(c.viewport, c.window, c.fit), _weapon(weapon or c.weapon), co, minimap=c.minimap, heightmap=maps(c.hm),
                                               image=img, bytes=want_bytes, margin=want_margin)
    return base, img, b, m, res


# ---- per call
@pytest.mark.parametrize("case", K.line_cases(), ids=lambda c: c.name)
def test_every_line_case_on_the_per_call_path(vision, maps, case):
    recs = K.checked_lines(case)
    _same_lines(_lines_call(vision, maps, case), recs, case.name)
    if case.name == "m == margin_m":                              # ... and one ulp more blocks, at the very sample
        more = float(np.nextafter(case.margin, np.inf))
        out = _lines_call(vision, maps, case, margin=more)
        _same_lines(out, K.restate_lines(case, margin=more), "one ulp more")
        assert out[0].dir[0].arc[B.LOW].status == R.S_BLOCKED and out[0].dir[0].arc[B.LOW].n_blocked == 1
    if case.name.startswith("low blocked, high clear"):           # the answer the feature is for, on the device's own record
        out = _lines_call(vision, maps, case)
        assert [out[0].dir[0].arc[a].status for a in (0, 1)] == [R.S_CLEAR, R.S_BLOCKED] and out[0].dir[0].choice == 1 + B.HIGH


@pytest.mark.parametrize("case", K.map_cases(), ids=lambda c: c.name)
def test_every_map_case_on_the_per_call_path(vision, maps, case):
    r = K.checked_map(case)
    base, img, b, m, res = _map_call(vision, maps, case)
    _same_plane(b, r["bytes"], "class bytes", case.name)
    _same_plane(m, r["margin"], "margins", case.name)
    assert np.array_equal(img, R.paint(base.copy(), r["bytes"], PALETTE)), case.name
    assert np.array_equal(img[..., 3], base[..., 3])
    _same_summary(res, r, case.name)


def test_every_combination_of_outputs_per_call_and_the_default_palette(vision, maps):
    case = next(c for c in K.map_cases() if c.name == "country, 130 x 33, a scale per axis")
    r = K.checked_map(case)
    for paint, by, mg in itertools.product((False, True), repeat=3):
        base, img, b, m, res = _map_call(vision, maps, case, paint=paint, want_bytes=by, want_margin=mg, palette=None)
        assert (img is None, b is None, m is None) == (not paint, not by, not mg)
        if paint:
            assert np.array_equal(img, R.paint(base.copy(), r["bytes"])) and not np.array_equal(img, base), (paint, by, mg)
        if by:
            _same_plane(b, r["bytes"], "class bytes", (paint, by, mg))
        if mg:
            _same_plane(m, r["margin"], "margins", (paint, by, mg))
        _same_summary(res, r, (paint, by, mg))                     # (the summary alone included)


def test_the_default_weapon_is_tied_to_terrain_clearance(vision, maps):
    """With smhv_weapon_defaults arc[HIGH] of every line equals smhv_clearance_lines' record field for field; the map's own class equals
    smhv_clearance_map's status under 1 -> 1, 3 -> 2, 4 -> 3, and the LOS bits are identical."""
    import squad_mortar_helper_amd as smh
    n = 0
    for c in CC.line_cases():
        if not c.lines:
            continue
        co = smh.ClearanceOptions(samples=c.samples, margin_m=c.margin)
        ln = np.array(c.lines, np.float32).reshape(-1, 4)
        ref, _ = vision.clearance_lines(ln, co, minimap=c.minimap, heightmap=maps(c.hm), fit_to_minimap=c.fit, viewport=c.viewport)
        got = vision.ballistic_clearance_lines(ln, smh.Weapon(), smh.BallisticClearanceOptions(samples=c.samples, margin_m=c.margin), minimap=c.minimap,
                                               heightmap=maps(c.hm), fit_to_minimap=c.fit, viewport=c.viewport)
        for i in range(len(ln)):
            for d in (0, 1):
                a, t, g = got[i].dir[d].arc[B.HIGH], ref[i].dir[d], got[i].dir[d]
                assert g.valid == (1 if t.status else 0), (c.name, i, d)
                assert (a.status, a.first_blocked, a.n_blocked, a.min_at, g.los_blocked) == (t.status, t.first_blocked, t.n_blocked, t.min_at, t.los_blocked), (c.name, i, d)
                assert same_bits(a.min_margin, t.min_margin), (c.name, i, d, a.min_margin, t.min_margin)
                n += 1
    assert n >= 500
    to_status = np.array([0, 1, 255, 2, 3, 255, 255, 255], np.uint8)
    for c in CC.map_cases():
        co = smh.ClearanceOptions(samples=c.samples, margin_m=c.margin, origin=c.origin)
        opt = _options(c.viewport, c.window, c.fit)
        ref, _ = vision.clearance_map(opt, co, minimap=c.minimap, heightmap=maps(c.hm), image=None, bytes=True)
        got, _, _ = vision.ballistic_clearance_map(opt, smh.Weapon(), smh.BallisticClearanceOptions(samples=c.samples, margin_m=c.margin, origin=c.origin),
                                                   minimap=c.minimap, heightmap=maps(c.hm), bytes=True, margin=False)
        assert np.array_equal(to_status[got & 7], ref & 0x7F) and np.array_equal(got & 0x80, ref & 0x80), c.name


def test_every_line_is_tied_to_ballistics(vision, maps):
    """meters, alt_delta and both arcs' bal equal smhv_ballistic_lines' meters, alt_delta and status, for every line with a verdict."""
    n = 0
    for c in K.line_cases():
        if not c.lines:
            continue
        ln = np.array(c.lines, np.float32).reshape(-1, 4)
        got = _lines_call(vision, maps, c)
        sol = vision.ballistic_lines(ln, _weapon(c.weapon), mpx=None, minimap=c.minimap, heightmap=maps(c.hm), fit_to_minimap=c.fit, viewport=c.viewport)
        for i in range(len(ln)):
            for d in (0, 1):
                g, s = got[i].dir[d], sol[i].dir[d]
                if g.valid:
                    assert s.source == B.HEIGHTMAP and same_bits(g.meters, s.meters) and same_bits(g.alt_delta, s.alt_delta), (c.name, i, d)
                    assert [g.arc[a].bal for a in (0, 1)] == [s.arc[a].status for a in (0, 1)], (c.name, i, d)
                    n += 1
                else:
                    assert s.source != B.HEIGHTMAP, (c.name, i, d)
    assert n >= 100


# ---- batches
@pytest.fixture(scope="module")
def world(vision):
    """Three of the scenes of tests/minimap_scenes.py in a plain batch that has run once: ORIGIN lies in the first one's rectangle (the
    heightmap feeds it) and outside the second one's (no verdict there); the third is closed."""
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
    assert recs[0]["minimap"] is not None
    hm_data = CC.country_map()
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


def _want(world, rec, weapon, origin, window, samples, margin, fit=True):
    return R.clearance_map(weapon, _origin_of(rec, origin), window, samples, margin, _view(window), rec["minimap"], world["hm_data"], fit)


def _check_map_batch(world, b, stream, weapon, origin, window, ctx, parts=None, samples=64, margin=0.0, paint=True, by=True, mg=True, palette=PALETTE, fit=True):
    """Render (with paint), run the map in `parts` ([(first, n)]) with the outputs asked for, hold every frame against the restatement."""
    import torch
    import squad_mortar_helper_amd as smh
    ow, oh = window
    opt = _options(_view(window), window, fit)
    base = None
    if paint:
        b.render(None, ow, oh, options=opt, stream=stream)
        base = [b.read_render(f).copy() for f in range(N)]
    co = smh.BallisticClearanceOptions(samples=samples, margin_m=margin, origin=origin, paint=paint, bytes=by, margin=mg, palette=palette)
    planes = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    margins = torch.full((N, oh, ow), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for first, n in parts or [(0, N)]:
        assert b.ballistic_clearance_map(opt, _weapon(weapon), co, first=first, n=n, heightmap=world["hm"], bytes_ptr=planes[first].data_ptr() if by else None,
                                         margin_ptr=margins[first].data_ptr() if mg else None, stream=stream) == {}
    res = b.read_ballistic_clearance_map(0, N)
    planes, margins = planes.cpu().numpy(), margins.cpu().numpy()
    out = []
    for f in range(N):
        r = _want(world, world["recs"][f], weapon, origin, window, samples, margin, fit)
        if by:
            _same_plane(planes[f], r["bytes"], "class bytes", (ctx, f, world["names"][f]))
        else:
            assert (planes[f] == 0xEE).all()
        if mg:
            _same_plane(margins[f], r["margin"], "margins", (ctx, f, world["names"][f]))
        else:
            assert (margins[f] == 7.0).all()
        if paint:
            assert np.array_equal(b.read_render(f), R.paint(base[f].copy(), r["bytes"], palette)), (ctx, f, world["names"][f])
        _same_summary(res[f], r, (ctx, f, world["names"][f]))
        out.append(r)
    assert not out[2]["valid"] and bytes(res[2]) == bytes(64)      # the closed frame: no origin, a result of zeros
    return out


def _check_lines_batch(world, b, stream, weapon, ctx, parts=None, samples=64, margin=0.0):
    import squad_mortar_helper_amd as smh
    co = smh.BallisticClearanceOptions(samples=samples, margin_m=margin)
    for first, n in parts or [(0, N)]:
        b.ballistic_clearance(_weapon(weapon), co, first=first, n=n, heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, stream=stream)
    got = b.read_ballistic_clearance(0, N)
    valid = 0
    for f, rec in enumerate(world["recs"]):
        n = rec["n_lines"]
        want = R.lines(weapon, rec["lines"], samples, margin, rec["minimap"], world["hm_data"], False, LINE_VIEW)
        assert got[f].n_lines == n and tuple(got[f].reserved) == (0, 0, 0), (ctx, f)
        _same_lines(got[f].line[:n], want, (ctx, f))
        assert bytes(got[f])[16 + 192 * n:] == bytes(192 * (32 - n)), (ctx, f, "lines beyond n_lines are zero")
        valid += sum(1 for pair in want if pair[0] is not None)
    return valid


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w)
def test_a_plain_batch_of_three_frames_that_differ(vision, world, window):
    fb, s = world["fb"], world["s"]
    out = _check_map_batch(world, fb, s, K.THROWER, ORIGIN, window, "point")
    assert [r["valid"] for r in out] == [1, 1, 0] and out[0]["bytes"].any() and not out[1]["bytes"].any()
    f = K.features(out[0])
    print("features of frame 0:", f)
    assert sum(1 for v in f.values() if v[0]) >= 6                  # the batch is no batch of zeros
    out0 = _check_map_batch(world, fb, s, K.THROWER_LOW, ("p0", 0), window, "line p0", samples=65, margin=1.5)
    out1 = _check_map_batch(world, fb, s, K.ROCKET_HIGH, ("p1", 0), window, "line p1", samples=33, fit=False)
    assert [r["valid"] for r in out0] == [1, 1, 0] == [r["valid"] for r in out1] and out0[0]["origin"] != out1[0]["origin"]
    _check_map_batch(world, fb, s, K.MORTAR, ("p0", 31), window, "line 31")
    assert fb.ballistic_clearance_map_ptr() != 0


def test_in_parts_every_combination_of_outputs_and_the_lines_of_a_batch(vision, world):
    fb, s = world["fb"], world["s"]
    _check_map_batch(world, fb, s, K.THROWER, ORIGIN, WINDOWS[0], "parts", parts=[(1, 2), (0, 1)])
    _check_map_batch(world, fb, s, K.THROWER_LOW, ("p0", 0), WINDOWS[1], "parts, line", parts=[(0, 1), (1, 1), (2, 1)], samples=34)
    for paint, by, mg in itertools.product((False, True), repeat=3):
        _check_map_batch(world, fb, s, K.THROWER, ORIGIN, WINDOWS[1], ("outputs", paint, by, mg), paint=paint, by=by, mg=mg, palette=None)
    for w in (K.MORTAR, K.THROWER_LOW):
        assert _check_lines_batch(world, fb, s, w, "lines", parts=[(1, 2), (0, 1)]) >= 1
    _check_lines_batch(world, fb, s, K.THROWER, "lines, S = 66, a margin", samples=66, margin=2.5)
    assert fb.ballistic_clearance_ptr() != 0


def test_first_use_and_no_side_effects_on_the_other_families(vision, world):
    """A fresh batch: E_STATE before the family's first call; a first call over one frame leaves zeros in the rest of its slabs; planes and
    the summary need no render, PAINT needs the most recent one; and the slabs of terrain clearance and ballistics are as they were."""
    import squad_mortar_helper_amd as smh
    L = smh._lib
    d, s = world["d"], world["s"]
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"], stream=s)
    window = WINDOWS[1]
    opt = _options(_view(window), window)
    for call in (lambda: fb2.read_ballistic_clearance_map(0, 1), fb2.ballistic_clearance_map_ptr, lambda: fb2.read_ballistic_clearance(0, 1), fb2.ballistic_clearance_ptr):
        with pytest.raises(smh.VisionError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    weapon = _weapon(K.THROWER)
    # the existing families first, so that their slabs exist around the new calls
    fb2.clearance(smh.ClearanceOptions(samples=64), heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, stream=s)
    fb2.clearance_map(opt, smh.ClearanceOptions(samples=64, origin=ORIGIN, paint=False), heightmap=world["hm"], stream=s)
    fb2.ballistics(weapon, heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, stream=s)
    fb2.ballistic_map(opt, weapon, smh.BallisticOptions(origin=ORIGIN, paint=False), heightmap=world["hm"], stream=s)
    before = [bytes(fb2.read_clearance(0, N)), bytes(fb2.read_clearance_map(0, N)), bytes(fb2.read_ballistics(0, N)), bytes(fb2.read_ballistic_map(0, N)),
              bytes(fb2.read_results(0, N))]
    fb2.ballistic_clearance_map(opt, weapon, smh.BallisticClearanceOptions(origin=ORIGIN, paint=False), first=0, n=1, heightmap=world["hm"], stream=s)
    res = fb2.read_ballistic_clearance_map(0, N)
    assert bytes(res[1]) == bytes(64) and bytes(res[2]) == bytes(64)
    _same_summary(res[0], _want(world, world["recs"][0], K.THROWER, ORIGIN, window, 64, 0.0), "the summary alone, a first call over one frame")
    assert res[0].valid == 1 and sum(res[0].own) > 0
    fb2.ballistic_clearance(weapon, smh.BallisticClearanceOptions(), first=0, n=1, heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, stream=s)
    got = fb2.read_ballistic_clearance(0, N)
    row = C.sizeof(L.BallisticClearanceResult)
    assert bytes(got)[row:] == bytes(2 * row) and got[0].n_lines == world["recs"][0]["n_lines"]
    _check_map_batch(world, fb2, s, K.THROWER, ORIGIN, window, "no render", paint=False)
    after = [bytes(fb2.read_clearance(0, N)), bytes(fb2.read_clearance_map(0, N)), bytes(fb2.read_ballistics(0, N)), bytes(fb2.read_ballistic_map(0, N)),
             bytes(fb2.read_results(0, N))]
    assert before == after
    paint = smh.BallisticClearanceOptions(origin=ORIGIN, paint=True)
    with pytest.raises(smh.VisionError) as ei:
        fb2.ballistic_clearance_map(opt, weapon, paint, heightmap=world["hm"], stream=s)
    assert ei.value.code == L.E_STATE
    fb2.render(None, window[0], window[1], options=opt, stream=s)
    fb2.ballistic_clearance_map(opt, weapon, paint, heightmap=world["hm"], stream=s)
    for w, h in ((window[0] + 1, window[1]), (window[1], window[0])):
        with pytest.raises(smh.VisionError) as ei:
            fb2.ballistic_clearance_map(_options(_view(window), (w, h)), weapon, paint, heightmap=world["hm"], stream=s)
        assert ei.value.code == L.E_STATE, (w, h)
    other = (33, 17)                                               # ... which the planes alone do not mind
    made = fb2.ballistic_clearance_map(_options(_view(other), other), weapon, smh.BallisticClearanceOptions(origin=ORIGIN, paint=False, bytes=True, margin=True),
                                       first=0, n=1, heightmap=world["hm"], stream=s)
    r = R.clearance_map(K.THROWER, ORIGIN, other, 64, 0.0, _view(other), world["recs"][0]["minimap"], world["hm_data"], True)
    _same_plane(made["bytes"][0].cpu().numpy(), r["bytes"], "class bytes", "another window")
    _same_plane(made["margin"][0].cpu().numpy(), r["margin"], "margins", "another window")
    fb2.close()


def test_argument_errors_enqueue_nothing(vision, world, maps):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s = world["fb"], world["s"]
    window = WINDOWS[1]
    ow, oh = window
    opt = _options(_view(window), window)
    hm = world["hm"]._hm
    fo = L.firing_options(False, LINE_VIEW)
    fb.render(None, ow, oh, options=opt, stream=s)
    good = smh.BallisticClearanceOptions(samples=64, margin_m=1.0, origin=ORIGIN, paint=True, bytes=True, margin=True)
    weapon = _weapon(K.THROWER)
    planes_t = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    margins_t = torch.full((N, oh, ow), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fb.ballistic_clearance_map(opt, weapon, good, heightmap=world["hm"], bytes_ptr=planes_t.data_ptr(), margin_ptr=margins_t.data_ptr(), stream=s)
    fb.ballistic_clearance(weapon, good, heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, stream=s)
    images = [fb.read_render(f).copy() for f in range(N)]
    slabs = bytes(fb.read_ballistic_clearance_map(0, N)), bytes(fb.read_ballistic_clearance(0, N))
    before = planes_t.cpu().numpy().tobytes(), margins_t.cpu().numpy().tobytes()

    def arms(**kw):
        w = weapon.struct()
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    nan, inf = float("nan"), float("inf")
    bad_opt = bad_options(good.struct)
    bad_arm = [arms(size=76), arms(arc=2), arms(unit=3), arms(velocity=0.0), arms(velocity=nan), arms(gravity=-1.0), arms(gravity=inf), arms(elev_min=nan),
               arms(elev_max=inf), arms(elev_min=81.0), arms(range_min=-1.0), arms(dispersion=-0.5), arms(dispersion=nan)]
    planes = L.BallisticClearancePlanes(planes_t.data_ptr(), margins_t.data_ptr())
    pl, st, o, w = C.byref(planes), C.c_void_p(s), good.struct(), arms()
    bmap, blines = lib.smhv_batch_ballistic_clearance_map, lib.smhv_batch_ballistic_clearance
    for i, bo in enumerate(bad_opt):
        assert bmap(fb._b, 0, N, hm, C.byref(opt), C.byref(w), C.byref(bo), pl, st) == L.E_INVALID, i
        assert blines(fb._b, 0, N, hm, C.byref(fo), C.byref(w), C.byref(bo), st) == L.E_INVALID, i
    for i, bw in enumerate(bad_arm):
        assert bmap(fb._b, 0, N, hm, C.byref(opt), C.byref(bw), C.byref(o), pl, st) == L.E_INVALID, i
        assert blines(fb._b, 0, N, hm, C.byref(fo), C.byref(bw), C.byref(o), st) == L.E_INVALID, i
    assert bmap(None, 0, N, hm, C.byref(opt), C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    assert bmap(fb._b, 0, N, hm, C.byref(opt), None, C.byref(o), pl, st) == L.E_INVALID
    assert bmap(fb._b, 0, N, hm, C.byref(opt), C.byref(w), None, pl, st) == L.E_INVALID
    assert bmap(fb._b, 0, N, hm, None, C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    assert bmap(fb._b, 0, N, hm, C.byref(opt), C.byref(w), C.byref(o), None, st) == L.E_INVALID                                   # plane flags and no planes
    for p in (L.BallisticClearancePlanes(None, margins_t.data_ptr()), L.BallisticClearancePlanes(planes_t.data_ptr(), None)):    # a plane flag without its pointer
        assert bmap(fb._b, 0, N, hm, C.byref(opt), C.byref(w), C.byref(o), C.byref(p), st) == L.E_INVALID
    assert bmap(fb._b, 1, N, hm, C.byref(opt), C.byref(w), C.byref(o), pl, st) == L.E_INVALID                                     # beyond the capacity
    assert bmap(fb._b, 0, 0, hm, C.byref(opt), C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    assert blines(fb._b, 1, N, hm, C.byref(fo), C.byref(w), C.byref(o), st) == L.E_INVALID and blines(fb._b, 0, 0, hm, C.byref(fo), C.byref(w), C.byref(o), st) == L.E_INVALID
    assert blines(None, 0, N, hm, C.byref(fo), C.byref(w), C.byref(o), st) == L.E_INVALID and blines(fb._b, 0, N, hm, C.byref(fo), None, C.byref(o), st) == L.E_INVALID
    assert blines(fb._b, 0, N, hm, C.byref(fo), C.byref(w), None, st) == L.E_INVALID
    wrong_fo = L.firing_options(False, LINE_VIEW)
    wrong_fo.flags = 2
    assert blines(fb._b, 0, N, hm, C.byref(wrong_fo), C.byref(w), C.byref(o), st) == L.E_INVALID
    wrong = _options(_view(window), window)
    wrong.size = 8
    assert bmap(fb._b, 0, N, hm, C.byref(wrong), C.byref(w), C.byref(o), pl, st) == L.E_INVALID
    for ww, hh in ((0, oh), (ow, 0), (16385, oh)):
        assert bmap(fb._b, 0, N, hm, C.byref(_options(_view(window), (ww, hh))), C.byref(w), C.byref(o), pl, st) == L.E_INVALID, (ww, hh)
    assert bmap(fb._b, 0, N, hm, C.byref(_options(_view(window), (ow + 1, oh))), C.byref(w), C.byref(o), pl, st) == L.E_STATE   # a stale window
    out1 = (L.BallisticClearanceMapResult * 1)()
    assert lib.smhv_batch_read_ballistic_clearance_map(fb._b, 1, N, out1) == L.E_INVALID and lib.smhv_batch_read_ballistic_clearance_map(fb._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_read_ballistic_clearance(fb._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_ballistic_clearance_map_ptr(fb._b, None) == L.E_INVALID and lib.smhv_batch_ballistic_clearance_ptr(fb._b, None) == L.E_INVALID
    torch.cuda.synchronize()
    for f in range(N):
        assert np.array_equal(fb.read_render(f), images[f]), f
    assert (bytes(fb.read_ballistic_clearance_map(0, N)), bytes(fb.read_ballistic_clearance(0, N))) == slabs
    assert (planes_t.cpu().numpy().tobytes(), margins_t.cpu().numpy().tobytes()) == before
    # the per-call paths: the same checks, a line origin and no output besides; image, planes and result stay as they were
    img = np.full((oh, ow, 4), 77, np.uint8)
    cb = np.full((oh, ow), 0xEE, np.uint8)
    mb = np.full((oh, ow), 7.0, np.float32)
    res = L.BallisticClearanceMapResult()
    C.memset(C.byref(res), 0x5A, 64)
    args = (img.ctypes.data, cb.ctypes.data, mb.ctypes.data, C.byref(res))
    pmap, plines = lib.smhv_ballistic_clearance_map, lib.smhv_ballistic_clearance_lines
    line_origin = good.struct()
    line_origin.origin_mode = L.REACH_ORIGIN_LINE_P0
    for i, bo in enumerate(bad_opt + [line_origin]):
        assert pmap(vision._ctx, hm, C.byref(opt), C.byref(w), C.byref(bo), None, *args) == L.E_INVALID, i
    for i, bw in enumerate(bad_arm):
        assert pmap(vision._ctx, hm, C.byref(opt), C.byref(bw), C.byref(o), None, *args) == L.E_INVALID, i
    assert pmap(vision._ctx, hm, C.byref(opt), C.byref(w), C.byref(o), None, None, None, None, None) == L.E_INVALID
    assert pmap(None, hm, C.byref(opt), C.byref(w), C.byref(o), None, *args) == L.E_INVALID
    one = np.array([[1.0, 2.0, 30.0, 40.0]], np.float32)
    rec = (L.BallisticClearance * 1)()
    C.memset(rec, 0x5A, 192)
    for i, bo in enumerate(bad_opt):
        assert plines(vision._ctx, one.ctypes.data, 1, None, hm, C.byref(fo), C.byref(w), C.byref(bo), rec) == L.E_INVALID, i
    for i, bw in enumerate(bad_arm):
        assert plines(vision._ctx, one.ctypes.data, 1, None, hm, C.byref(fo), C.byref(bw), C.byref(o), rec) == L.E_INVALID, i
    assert plines(vision._ctx, None, 1, None, hm, C.byref(fo), C.byref(w), C.byref(o), rec) == L.E_INVALID
    assert plines(vision._ctx, one.ctypes.data, 1, None, hm, C.byref(fo), C.byref(w), C.byref(o), None) == L.E_INVALID
    assert (img == 77).all() and (cb == 0xEE).all() and (mb == 7.0).all() and bytes(res) == b"\x5a" * 64 and bytes(rec) == b"\x5a" * 192
    # a correct call follows, without a result, and the batch still answers
    case = next(c for c in K.map_cases() if c.name == "country, 65 x 17, a scale per axis")
    r = K.checked_map(case)
    _, _, b, m, _ = _map_call(vision, maps, case, paint=False)
    _same_plane(b, r["bytes"], "class bytes", "after the failed calls")
    _same_plane(m, r["margin"], "margins", "after the failed calls")
    _check_map_batch(world, fb, s, K.THROWER, ORIGIN, window, "after the failed calls")
