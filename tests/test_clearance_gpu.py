"""Terrain clearance on the device (smhv_clearance_lines / smhv_clearance_map / smhv_batch_clearance / smhv_batch_clearance_map), every
comparison exact: records, profiles, status bytes, summaries and painted images equal to the restatement (tests/clearance_ref.py)
bit for bit -- per call for every case, on a plain batch and on a slot of both pipeline schedules from the batch's own records."""
import ctypes as C
import struct

import numpy as np
import pytest

import clearance_cases as CC
import clearance_ref as R
import minimap_scenes as S

pytestmark = pytest.mark.gpu

PALETTE = dict(out_of_range=(250, 10, 20, 255), clear=(10, 200, 30, 90), blocked=(3, 4, 5, 131), los=(90, 0, 200, 77))
FIELDS = ("status", "first_blocked", "n_blocked", "los_blocked", "min_margin", "min_at")
WINDOW = (97, 66)                                                # two tiles across with one column in the second, five down with two rows in the last
VIEW = (0.26, 0.11, 1.25, -0.5)                                  # the 360 x 585 ROI of the scenes into that window, a scale per axis
LINE_VIEW = (1.5, 0.75, -6.0, 2.0)                               # the viewport the batch's line clearance is asked at


def _options(viewport, window, fit=True):
    import squad_mortar_helper_amd as smh
    sw, sh, tx, ty = viewport or (1.0, 1.0, 0.0, 0.0)
    vp = smh.MapViewport((0.0, 0.0, float(window[0]), float(window[1])), (sw, sh), (tx, ty))
    return smh.render_options(vp, window[0], window[1], heightmap=False, markers=True, fit_to_minimap=fit, background=(9, 8, 7, 255))


def _bits(v):
    return struct.pack("<d", v)


def _same_dir(got, want, ctx):
    g = {f: getattr(got, f) for f in FIELDS}
    assert {f: v for f, v in g.items() if f != "min_margin"} == {f: v for f, v in want.items() if f != "min_margin"} and got.reserved == 0, (ctx, g, want)
    assert _bits(g["min_margin"]) == _bits(want["min_margin"]), (ctx, g["min_margin"].hex(), float(want["min_margin"]).hex())


def _same_lines(out, prof, recs, want_prof, ctx):
    assert len(out) == len(recs)
    for i, (rec, (fwd, bck)) in enumerate(zip(out, recs)):
        _same_dir(rec.dir[0], fwd, (ctx, i, 0))
        _same_dir(rec.dir[1], bck, (ctx, i, 1))
    if want_prof is not None:
        assert prof.dtype == np.float32 and prof.shape == want_prof.shape, (ctx, prof.shape)
        assert prof.tobytes() == want_prof.tobytes(), (ctx, np.argwhere(prof != want_prof)[:4].tolist())


def _same_bytes(got, want, ctx):
    assert got.shape == want.shape and got.dtype == np.uint8, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d bytes differ" % len(bad), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // CC.TW, y // CC.TH),
                              "got", int(got[y, x]), "want", int(want[y, x])))


def _same_summary(res, r, ctx):
    want = R.summary(r)
    got = dict(valid=int(res.valid), origin=(float(res.origin[0]), float(res.origin[1])), count=[int(v) for v in res.count], los_blocked=int(res.los_blocked))
    assert got == want and res.reserved == 0, (ctx, got, want)
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


def _lines_call(vision, maps, c, samples=None, margin=None, hm="case"):
    import squad_mortar_helper_amd as smh
    co = smh.ClearanceOptions(samples=c.samples if samples is None else samples, margin_m=c.margin if margin is None else margin)
    return vision.clearance_lines(np.array(c.lines, np.float32).reshape(-1, 4), co, minimap=c.minimap, heightmap=maps(c.hm) if hm == "case" else hm,
                                  fit_to_minimap=c.fit, viewport=c.viewport, profiles=True)


def _map_call(vision, maps, c, paint=True, want_bytes=True, palette=PALETTE, samples=None, hm="case"):
    import squad_mortar_helper_amd as smh
    ow, oh = c.window
    base = np.random.default_rng(5).integers(0, 256, size=(oh, ow, 4)).astype(np.uint8)
    img = base.copy() if paint else None
    co = smh.ClearanceOptions(samples=c.samples if samples is None else samples, margin_m=c.margin, origin=c.origin, palette=palette)
    b, res = vision.clearance_map(_options(c.viewport, c.window, c.fit), co, minimap=c.minimap, heightmap=maps(c.hm) if hm == "case" else hm, image=img,
                                  bytes=want_bytes)
    return base, img, b, res


@pytest.mark.parametrize("case", CC.line_cases(), ids=lambda c: c.name)
def test_every_line_case_on_the_per_call_path(vision, maps, case):
    recs, prof = CC.checked_lines(case)
    out, got = _lines_call(vision, maps, case)
    _same_lines(out, got, recs, prof, case.name)
    if case.name == "m == margin_m":                              # ... and one ulp more blocks, at the very sample
        more = float(np.nextafter(case.margin, np.inf))
        out, got = _lines_call(vision, maps, case, margin=more)
        _same_lines(out, got, *CC.restate_lines(case, margin=more), "one ulp more")
        assert out[0].dir[0].status == R.BLOCKED


@pytest.mark.parametrize("case", CC.map_cases(), ids=lambda c: c.name)
def test_every_map_case_on_the_per_call_path(vision, maps, case):
    r = CC.checked_map(case)
    base, img, b, res = _map_call(vision, maps, case)
    _same_bytes(b, r["bytes"], case.name)
    assert np.array_equal(img, R.paint(base.copy(), r["bytes"], PALETTE)), case.name
    assert np.array_equal(img[..., 3], base[..., 3])
    _same_summary(res, r, case.name)


def test_paint_and_bytes_against_each_alone(vision, maps):
    case = next(c for c in CC.map_cases() if c.name == "window 130 x 33")
    r = CC.checked_map(case)
    base, both_img, both_b, both_res = _map_call(vision, maps, case, palette=None)
    _, img, b, res = _map_call(vision, maps, case, want_bytes=False, palette=None)
    assert b is None and np.array_equal(img, both_img) and np.array_equal(img, R.paint(base.copy(), r["bytes"])) and not np.array_equal(img, base)
    assert bytes(res) == bytes(both_res)
    _, img, b, res = _map_call(vision, maps, case, paint=False, palette=None)
    assert img is None and np.array_equal(b, both_b) and bytes(res) == bytes(both_res)
    _same_bytes(b, r["bytes"], "bytes alone")
    _same_summary(res, r, "bytes alone")


def test_without_a_heightmap_nothing_has_a_verdict(vision, maps):
    wall = next(c for c in CC.line_cases() if c.name == "wall, S = 64")
    out, prof = _lines_call(vision, maps, wall, hm=None)
    assert bytes(out) == bytes(64 * len(out)) and not prof.any()
    land = next(c for c in CC.map_cases() if c.name == "window 65 x 17")
    base, img, b, res = _map_call(vision, maps, land, hm=None)
    assert not b.any() and np.array_equal(img, base)
    assert (res.valid, tuple(res.count), res.los_blocked) == (1, (0, 0, 0), 0)   # an origin, and nothing to hold an arc against


def test_a_heightmap_switched_between_two_calls(vision, maps):
    """The same lines and the same window against one heightmap, another, and the first again: no call sees the previous one's."""
    wall = next(c for c in CC.line_cases() if c.name == "wall, S = 64")
    land = next(c for c in CC.map_cases() if c.name == "window 65 x 17")
    other = wall._replace(hm=CC.country_map())
    assert wall.hm[0].shape == other.hm[0].shape
    want = {id(c): CC.restate_lines(c) for c in (wall, other)}
    assert want[id(wall)][0] != want[id(other)][0]
    for c in (wall, other, wall):
        out, prof = _lines_call(vision, maps, c)
        _same_lines(out, prof, *want[id(c)], "switched")
    flat = land._replace(hm=CC.wall_map())
    wants = {id(c): CC.restate_map(c) for c in (land, flat)}
    assert not np.array_equal(wants[id(land)]["bytes"], wants[id(flat)]["bytes"])
    for c in (land, flat, land):
        _, _, b, res = _map_call(vision, maps, c, paint=False)
        _same_bytes(b, wants[id(c)]["bytes"], "switched")
        _same_summary(res, wants[id(c)], "switched")


def test_a_wrong_sample_count_shows(vision, maps):
    """The device at S = 64 against the restatement at S = 65, on the wall: they must differ -- the comparison can see a sample count."""
    wall = next(c for c in CC.line_cases() if c.name == "wall, S = 64")
    out, prof = _lines_call(vision, maps, wall)
    recs65, prof65 = CC.restate_lines(wall, samples=65)
    with pytest.raises(AssertionError):
        _same_lines(out, prof, recs65, prof65, "S = 64 against 65")
    _same_lines(out, prof, *CC.restate_lines(wall), "S = 64")
    land = next(c for c in CC.map_cases() if c.name == "130 x 33 panned, S = 64")
    _, _, b, _ = _map_call(vision, maps, land, paint=False)
    assert not np.array_equal(b, CC.restate_map(land, samples=65)["bytes"])
    _same_bytes(b, CC.checked_map(land)["bytes"], "S = 64")


# ---- the batch: three frames -- an open one whose record has no minimap rectangle, a closed one, an open one with its rectangle
@pytest.fixture(scope="module")
def world(vision):
    import torch
    import squad_mortar_helper_amd as smh
    frames, anchor_list, rects, names = S.make_scenes()
    order = [7, S.N_SCENES - 1, 0]
    frames = np.ascontiguousarray(frames[order])
    anchor_list = [anchor_list[i] for i in order]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb = smh.FrameBatch(vision, S.W, S.H, 3)
    fb.run(d.data_ptr(), 3, stages=stages, grayscale=False, anchors=anchors, stream=s)
    with_rects = smh.results_to_dicts(fb.read_results(0, 3))
    fb.run(d.data_ptr(), 1, stages=smh.STAGE_ALL, grayscale=False, anchors=anchors, stream=s)   # frame 0 again, without the minimap stage
    recs = smh.results_to_dicts(fb.read_results(0, 3))
    assert recs[0]["map_open"] and recs[0]["minimap"] is None and recs[0]["n_lines"] >= 1 and with_rects[0]["minimap"] is not None
    assert not recs[1]["map_open"] and recs[1]["n_lines"] == 0
    assert recs[2]["map_open"] and recs[2]["minimap"] is not None and recs[2]["n_lines"] >= 1
    hm_data = CC.country_map()
    hm = smh.Heightmap(vision, *hm_data)
    w = dict(d=d, s=s, anchors=anchors, fb=fb, recs=recs, with_rects=with_rects, stages=stages, hm=hm, hm_data=hm_data)
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


def _check_batch(world, b, stream, recs, ctx, samples=64, margin=0.0):
    """The line clearance with profiles, then the clearance map (rendered, painted, with bytes) from a point and from both ends of line
    0, every frame held against the restatement on the batch's own records -> the statuses seen."""
    import torch
    import squad_mortar_helper_amd as smh
    n = len(recs)
    seen = set()
    co = smh.ClearanceOptions(samples=samples, margin_m=margin)
    prof = torch.full((n, 32, R.PROFILE), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.clearance(co, heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, profiles_ptr=prof.data_ptr(), stream=stream)
    out = b.read_clearance(0, n)
    prof = prof.cpu().numpy()
    assert b.clearance_ptr() != 0
    for f, rec in enumerate(recs):
        want, wprof = R.lines(rec["lines"], samples, margin, rec["minimap"], world["hm_data"], False, LINE_VIEW)
        assert out[f].n_lines == rec["n_lines"] and out[f].reserved == 0, (ctx, f)
        _same_lines(out[f].line[:rec["n_lines"]], prof[f, :rec["n_lines"]], want, wprof, (ctx, f))
        assert bytes(out[f])[8 + 64 * rec["n_lines"]:] == bytes(64 * (32 - rec["n_lines"])) and not prof[f, rec["n_lines"]:].any(), (ctx, f)
        seen |= set(d["status"] for pair in want for d in pair)
    ow, oh = WINDOW
    opt = _options(VIEW, WINDOW)
    for origin in ((150.0, 260.0), ("p0", 0), ("p1", 0)):
        b.render(None, ow, oh, options=opt, stream=stream)
        base = [b.read_render(f).copy() for f in range(n)]
        mo = smh.ClearanceOptions(samples=samples, margin_m=margin, origin=origin, paint=True, bytes=True, palette=PALETTE)
        got = torch.full((n, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        b.clearance_map(opt, mo, heightmap=world["hm"], bytes_ptr=got.data_ptr(), stream=stream)
        res = b.read_clearance_map(0, n)
        got = got.cpu().numpy()
        for f, rec in enumerate(recs):
            r = R.clearance_map(_origin_of(rec, origin), WINDOW, samples, margin, VIEW, rec["minimap"], world["hm_data"], True)
            _same_bytes(got[f], r["bytes"], (ctx, origin, f))
            assert np.array_equal(b.read_render(f), R.paint(base[f].copy(), r["bytes"], PALETTE)), (ctx, origin, f)
            _same_summary(res[f], r, (ctx, origin, f))
            seen |= set(int(v) & 0x7F for v in np.unique(r["bytes"]))
        assert bytes(res[1]) == bytes(32) and not got[1].any()      # the closed frame: no origin, a result of zeros
    assert b.clearance_map_ptr() != 0
    return seen


def test_a_plain_batch_whose_frames_differ(vision, world):
    seen = _check_batch(world, world["fb"], world["s"], world["recs"], "plain")
    assert {R.NONE, R.CLEAR} <= seen and len(seen) >= 3, seen       # the batch is no batch of zeros
    _check_batch(world, world["fb"], world["s"], world["recs"], "plain, S = 65, a margin", samples=65, margin=12.5)


def test_a_slot_of_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, 3, depth=3, search=search)
        slot = p.submit(world["d"].data_ptr(), 3, stages=world["stages"], grayscale=False, anchors=world["anchors"])
        p.wait()
        recs = smh.results_to_dicts(p.slots[slot].read_results(0, 3))
        assert [r["n_lines"] for r in recs] == [r["n_lines"] for r in world["with_rects"]] and [r["minimap"] for r in recs] == [r["minimap"] for r in world["with_rects"]]
        seen = _check_batch(world, p.slots[slot], p.stream_of(slot), recs, search)
        assert {R.NONE, R.CLEAR} <= seen, (search, seen)
        p.close()


def test_refused_arguments_enqueue_nothing(vision, world, maps):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s, recs = world["fb"], world["s"], world["recs"]
    ow, oh = WINDOW
    opt = _options(VIEW, WINDOW)
    hm = world["hm"]._hm
    fo = L.firing_options(False, LINE_VIEW)
    fb.render(None, ow, oh, options=opt, stream=s)
    good = smh.ClearanceOptions(samples=64, origin=(150.0, 260.0), paint=True, bytes=True)
    got = torch.full((3, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    prof = torch.full((3, 32, R.PROFILE), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fb.clearance_map(opt, good, heightmap=world["hm"], bytes_ptr=got.data_ptr(), stream=s)
    fb.clearance(good, heightmap=world["hm"], fit_to_minimap=False, viewport=LINE_VIEW, profiles_ptr=prof.data_ptr(), stream=s)
    images = [fb.read_render(f).copy() for f in range(3)]
    slabs = bytes(fb.read_clearance(0, 3)), bytes(fb.read_clearance_map(0, 3))
    before = got.cpu().numpy().copy(), prof.cpu().numpy().copy()

    def options(**kw):
        o = good.struct()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    bad = [options(size=60), options(size=68), options(size=0), options(flags=4), options(flags=0x80000003), options(samples=0), options(samples=257),
           options(samples=0xFFFFFFFF), options(margin_m=-1.0), options(margin_m=-1e-300), options(margin_m=float("nan")), options(margin_m=float("inf"))]
    bad_map = [options(origin_mode=3), options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=32), options(origin_mode=L.REACH_ORIGIN_LINE_P1, line=0xFFFFFFFF)]
    db, dp, st = C.c_void_p(got.data_ptr()), C.c_void_p(prof.data_ptr()), C.c_void_p(s)
    o = options()
    for i, w in enumerate(bad):
        assert lib.smhv_batch_clearance(fb._b, 0, 3, hm, C.byref(fo), C.byref(w), dp, st) == L.E_INVALID, i
    for i, w in enumerate(bad + bad_map):
        assert lib.smhv_batch_clearance_map(fb._b, 0, 3, hm, C.byref(opt), C.byref(w), db, st) == L.E_INVALID, i
    assert lib.smhv_batch_clearance(None, 0, 3, hm, C.byref(fo), C.byref(o), dp, st) == L.E_INVALID
    assert lib.smhv_batch_clearance(fb._b, 0, 3, hm, C.byref(fo), None, dp, st) == L.E_INVALID
    assert lib.smhv_batch_clearance(fb._b, 1, 3, hm, C.byref(fo), C.byref(o), dp, st) == L.E_INVALID               # beyond the capacity
    assert lib.smhv_batch_clearance(fb._b, 0, 0, hm, C.byref(fo), C.byref(o), dp, st) == L.E_INVALID
    wrong = L.firing_options(False, LINE_VIEW)
    wrong.flags = 2
    assert lib.smhv_batch_clearance(fb._b, 0, 3, hm, C.byref(wrong), C.byref(o), dp, st) == L.E_INVALID
    assert lib.smhv_batch_clearance_map(None, 0, 3, hm, C.byref(opt), C.byref(o), db, st) == L.E_INVALID
    assert lib.smhv_batch_clearance_map(fb._b, 0, 3, hm, C.byref(opt), None, db, st) == L.E_INVALID
    assert lib.smhv_batch_clearance_map(fb._b, 0, 3, hm, None, C.byref(o), db, st) == L.E_INVALID
    assert lib.smhv_batch_clearance_map(fb._b, 0, 3, hm, C.byref(opt), C.byref(o), None, st) == L.E_INVALID       # BYTES and no memory
    assert lib.smhv_batch_clearance_map(fb._b, 1, 3, hm, C.byref(opt), C.byref(o), db, st) == L.E_INVALID
    assert lib.smhv_batch_clearance_map(fb._b, 0, 0, hm, C.byref(opt), C.byref(o), db, st) == L.E_INVALID
    for w, h in ((0, oh), (ow, 0), (16385, oh)):
        assert lib.smhv_batch_clearance_map(fb._b, 0, 3, hm, C.byref(_options(VIEW, (w, h))), C.byref(o), db, st) == L.E_INVALID, (w, h)
    assert lib.smhv_batch_clearance_map(fb._b, 0, 3, hm, C.byref(_options(VIEW, (ow + 1, oh))), C.byref(o), db, st) == L.E_STATE   # a stale window
    assert lib.smhv_batch_read_clearance(fb._b, 1, 3, (L.ClearanceResult * 3)()) == L.E_INVALID
    assert lib.smhv_batch_read_clearance(fb._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_read_clearance_map(fb._b, 1, 3, (L.ClearanceMapResult * 3)()) == L.E_INVALID
    assert lib.smhv_batch_clearance_ptr(fb._b, None) == L.E_INVALID and lib.smhv_batch_clearance_map_ptr(fb._b, None) == L.E_INVALID
    torch.cuda.synchronize()
    for f in range(3):
        assert np.array_equal(fb.read_render(f), images[f]), f
    assert (bytes(fb.read_clearance(0, 3)), bytes(fb.read_clearance_map(0, 3))) == slabs
    assert np.array_equal(got.cpu().numpy(), before[0]) and np.array_equal(prof.cpu().numpy(), before[1])
    # a batch that has computed neither has no slab to read
    fb2 = smh.FrameBatch(vision, S.W, S.H, 3)
    for call in (lambda: fb2.read_clearance(0, 1), fb2.clearance_ptr, lambda: fb2.read_clearance_map(0, 1), fb2.clearance_map_ptr):
        with pytest.raises(smh.VisionError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    with pytest.raises(smh.VisionError) as ei:                     # PAINT before any render
        fb2.clearance_map(opt, smh.ClearanceOptions(origin=(150.0, 260.0)), heightmap=world["hm"], stream=s)
    assert ei.value.code == L.E_STATE
    fb2.close()
    # the per-call paths: the same checks, a line origin and two null outputs besides; what the caller passed stays as it was
    img = np.full((oh, ow, 4), 77, np.uint8)
    cb = np.full((oh, ow), 0xEE, np.uint8)
    res = L.ClearanceMapResult()
    C.memset(C.byref(res), 0x5A, 32)
    args = (img.ctypes.data, cb.ctypes.data, C.byref(res))
    for i, w in enumerate(bad + bad_map + [options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=0)]):
        assert lib.smhv_clearance_map(vision._ctx, hm, C.byref(opt), C.byref(w), None, *args) == L.E_INVALID, i
    assert lib.smhv_clearance_map(vision._ctx, hm, C.byref(opt), C.byref(o), None, None, None, C.byref(res)) == L.E_INVALID
    assert lib.smhv_clearance_map(vision._ctx, hm, C.byref(opt), None, None, *args) == L.E_INVALID
    assert lib.smhv_clearance_map(vision._ctx, hm, None, C.byref(o), None, *args) == L.E_INVALID
    assert lib.smhv_clearance_map(None, hm, C.byref(opt), C.byref(o), None, *args) == L.E_INVALID
    assert (img == 77).all() and (cb == 0xEE).all() and bytes(res) == b"\x5a" * 32
    lines = np.array([[20.0, 64.0, 120.0, 64.0]], np.float32)
    out = (L.Clearance * 1)()
    C.memset(out, 0x5A, 64)
    pr = np.full((1, R.PROFILE), -1.0, np.float32)
    for i, w in enumerate(bad):
        assert lib.smhv_clearance_lines(vision._ctx, lines.ctypes.data, 1, None, hm, C.byref(fo), C.byref(w), out, pr.ctypes.data) == L.E_INVALID, i
    assert lib.smhv_clearance_lines(vision._ctx, lines.ctypes.data, 1, None, hm, C.byref(fo), None, out, pr.ctypes.data) == L.E_INVALID
    assert lib.smhv_clearance_lines(vision._ctx, None, 1, None, hm, C.byref(fo), C.byref(o), out, pr.ctypes.data) == L.E_INVALID
    assert lib.smhv_clearance_lines(vision._ctx, lines.ctypes.data, 1, None, hm, C.byref(fo), C.byref(o), None, pr.ctypes.data) == L.E_INVALID
    assert lib.smhv_clearance_lines(None, lines.ctypes.data, 1, None, hm, C.byref(fo), C.byref(o), out, pr.ctypes.data) == L.E_INVALID
    assert bytes(out) == b"\x5a" * 64 and (pr == -1.0).all()
    # correct calls follow, and the batch still answers
    wall = next(c for c in CC.line_cases() if c.name == "wall, S = 64")
    got_lines, got_prof = _lines_call(vision, maps, wall)
    _same_lines(got_lines, got_prof, *CC.checked_lines(wall), "after the failed calls")
    _check_batch(world, fb, s, recs, "after the failed calls")
