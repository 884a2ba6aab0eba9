"""The reach map on the device (smhv_batch_reach / smhv_reach_map), every comparison exact: class bytes, painted image and summary
equal to the restatement (tests/reach_ref.py) byte for byte, per call, on a plain batch, on a slot of both pipeline schedules and in
parts; and the class bytes tied to smhv_firing_solutions of the same lines."""
import ctypes as C

import numpy as np
import pytest

import minimap_scenes as S
import reach_cases as RC
import reach_ref as R
import test_reach_host as TH

pytestmark = pytest.mark.gpu

N = S.N_SCENES
WINDOW = (97, 66)                                                # two tiles across with one column in the second, five down with two rows in the last
VIEW = (0.26, 0.11, 1.25, -0.5)                                  # the 360 x 585 ROI of the scenes into that window, a scale per axis
RING = 100.0
PALETTE = dict(out_of_range=(250, 10, 20, 255), ring=(3, 4, 5, 131), band=[(10 + 30 * k, 255 - 20 * k, 7 * k, 40 + 25 * k) for k in range(8)])


def _options(viewport, window, fit=True):
    import squad_mortar_helper_amd as smh
    sw, sh, tx, ty = viewport or (1.0, 1.0, 0.0, 0.0)
    vp = smh.MapViewport((0.0, 0.0, float(window[0]), float(window[1])), (sw, sh), (tx, ty))
    return smh.render_options(vp, window[0], window[1], heightmap=False, markers=True, fit_to_minimap=fit, background=(9, 8, 7, 255))


def _summary(res):
    return dict(valid=int(res.valid), source_mask=int(res.source_mask), origin=(float(res.origin[0]), float(res.origin[1])), count=[int(v) for v in res.count],
                ring=int(res.ring))


def _same_classes(got, want, ctx):
    assert got.shape == want.shape and got.dtype == np.uint8, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d class bytes differ" % len(bad), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // RC.TW, y // RC.TH),
                              "got", int(got[y, x]), "want", int(want[y, x])))


def _same_summary(res, r, ctx):
    want = R.summary(r)
    got = _summary(res)
    assert got == want and tuple(res.reserved) == (0, 0), (ctx, got, want)
    # (the origin compared as bits too: -0.0 and NaN do not slip through ==)
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


def _per_call(vision, maps, c, paint=True, classes=True, palette=None, seed=5):
    import squad_mortar_helper_amd as smh
    ow, oh = c.window
    opt = _options(c.viewport, c.window, c.fit)
    base = np.random.default_rng(seed).integers(0, 256, size=(oh, ow, 4)).astype(np.uint8)
    img = base.copy() if paint else None
    ro = smh.ReachOptions(origin=c.origin, ring_m=c.ring_m, palette=palette)
    cls, res = vision.reach_map(opt, ro, mpx=c.mpx, minimap=c.minimap, heightmap=maps(c.hm), image=img, classes=classes)
    return base, img, cls, res


@pytest.mark.parametrize("case", RC.all_cases(), ids=lambda c: c.name)
def test_every_case_on_the_per_call_path(vision, maps, case):
    r = RC.checked(case)
    base, img, cls, res = _per_call(vision, maps, case, palette=PALETTE)
    _same_classes(cls, r["classes"], case.name)
    assert np.array_equal(img, R.paint(base.copy(), r["classes"], PALETTE)), case.name
    assert np.array_equal(img[..., 3], base[..., 3])
    _same_summary(res, r, case.name)


def test_either_output_alone_and_the_default_palette(vision, maps):
    case = next(c for c in RC.all_cases() if c.name == "seam")
    r = RC.checked(case)
    base, img, cls, res = _per_call(vision, maps, case, classes=False)
    assert cls is None and np.array_equal(img, R.paint(base.copy(), r["classes"])) and not np.array_equal(img, base)
    _same_summary(res, r, "paint alone")
    base, img, cls, res = _per_call(vision, maps, case, paint=False)
    assert img is None
    _same_classes(cls, r["classes"], "classes alone")
    _same_summary(res, r, "classes alone")


def test_the_class_bytes_agree_with_smhv_firing_solutions(vision, maps):
    """For 2400 sampled pixels that cover every class: smhv_firing_solutions of the line (o, t) says NaN exactly where the class is 1,
    source NONE exactly where it is 0, and elsewhere floor((mils[0] - 800) / 100), clamped to 0 .. 7, is k.  Samples within 1e-6 of a
    band edge are left out (the device's atan may differ from libm's by ulps): at most 1 % of them."""
    total = skipped = 0
    seen = set()
    for c, r, pts in TH.cross_samples():
        _, _, cls, _ = _per_call(vision, maps, c, paint=False)
        _same_classes(cls, r["classes"], c.name)
        dev = dict(r, classes=cls)                                 # the DEVICE's bytes are what is held against the firing solutions

        def solve(lines, c=c):
            f = vision.firing_solutions(np.array(lines, np.float32).reshape(-1, 4), mpx=c.mpx, minimap=c.minimap, heightmap=maps(c.hm),
                                        fit_to_minimap=c.fit, viewport=c.viewport)
            return [(float(v["mils"][0]), int(v["source"])) for v in f]
        n, k, classes = TH.cross_check(c, dev, pts, solve)
        total, skipped, seen = total + n, skipped + k, seen | classes
    assert total >= 2000 and skipped <= total // 100 and seen == set(range(10)), (total, skipped, seen)


@pytest.fixture(scope="module")
def world(vision):
    """The scenes of tests/minimap_scenes.py with the closed frame moved between open ones, in a plain batch that has run once."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, anchor_list, rects, names = S.make_scenes()
    order = [0, 1, N - 1] + list(range(2, N - 1))                   # the closed scene becomes frame 2
    frames = np.ascontiguousarray(frames[order])
    anchor_list, names = [anchor_list[i] for i in order], [names[i] for i in order]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    assert not recs[2]["map_open"] and all(recs[f]["map_open"] and recs[f]["n_lines"] >= 1 for f in range(N) if f != 2)
    assert any(r["minimap"] is not None for r in recs) and any(r["mpx"] is not None for r in recs)
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


def _want(world, rec, origin, fit, ring_m):
    return R.reach(_origin_of(rec, origin), WINDOW, VIEW, rec["minimap"], rec["mpx"], world["hm_data"], fit, ring_m)


def _check_batch(world, b, stream, origin, ctx, parts=None, fit=True, ring_m=RING, palette=None):
    """Render, read the images, run the reach map (in `parts`: [(first, n)]) with both outputs, hold every frame against the restatement
    -> the restatements."""
    import torch
    import squad_mortar_helper_amd as smh
    ow, oh = WINDOW
    opt = _options(VIEW, WINDOW, fit)
    b.render(None, ow, oh, options=opt, stream=stream)
    base = [b.read_render(f).copy() for f in range(N)]
    ro = smh.ReachOptions(origin=origin, ring_m=ring_m, paint=True, classes=True, palette=palette)
    cls = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for first, n in parts or [(0, N)]:
        b.reach(opt, ro, first=first, n=n, heightmap=world["hm"], classes_ptr=cls[first].data_ptr(), stream=stream)
    res = b.read_reach(0, N)
    cls = cls.cpu().numpy()
    out = []
    for f in range(N):
        r = _want(world, world["recs"][f], origin, fit, ring_m)
        _same_classes(cls[f], r["classes"], (ctx, f, world["names"][f]))
        assert np.array_equal(b.read_render(f), R.paint(base[f].copy(), r["classes"], palette)), (ctx, f, world["names"][f])
        _same_summary(res[f], r, (ctx, f, world["names"][f]))
        out.append(r)
    assert not out[2]["valid"] and bytes(res[2]) == bytes(64)      # the closed frame: no origin, a result of zeros
    return out


def _line_index(recs):
    """A line index some open frames have and, where the scenes' line counts differ, others have not."""
    counts = [r["n_lines"] for r in recs if r["map_open"]]
    return min(counts) if min(counts) < max(counts) else 0


def test_a_plain_batch_whose_frames_differ(vision, world):
    fb, s, recs = world["fb"], world["s"], world["recs"]
    out = _check_batch(world, fb, s, (150.0, 260.0), "point", palette=PALETTE)
    assert sum(r["valid"] for r in out) == N - 1
    masks = set(R.summary(r)["source_mask"] for r in out if r["valid"])
    assert any(m & (1 << R.HEIGHTMAP) for m in masks) and any(m & (1 << R.SCALES) for m in masks), masks
    assert any((r["classes"] & R.RING).any() for r in out) and len(set(int(v) for r in out for v in np.unique(r["classes"] & 0x7F))) >= 3
    line = _line_index(recs)
    out0 = _check_batch(world, fb, s, ("p0", line), "line p0")
    out1 = _check_batch(world, fb, s, ("p1", line), "line p1", fit=False, ring_m=0.0)
    have = [r["map_open"] and r["n_lines"] > line for r in recs]
    assert [bool(r["valid"]) for r in out0] == have == [bool(r["valid"]) for r in out1] and any(have)
    assert any(a["origin"] != b["origin"] for a, b in zip(out0, out1) if a["valid"])
    # a line no frame has: nothing anywhere
    none = _check_batch(world, fb, s, ("p0", 31), "line 31")
    assert not any(r["valid"] for r in none) or max(r["n_lines"] for r in recs) == 32
    assert fb.reach_ptr() != 0


def test_in_parts(vision, world):
    fb, s = world["fb"], world["s"]
    _check_batch(world, fb, s, (150.0, 260.0), "parts", parts=[(4, N - 4), (0, 4)])
    _check_batch(world, fb, s, ("p0", 0), "parts, line", parts=[(0, 1), (1, 1), (2, N - 2)], ring_m=10.0)


def test_a_slot_of_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, N, depth=3, search=search)
        slot = p.submit(world["d"].data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"])
        p.wait()
        recs = smh.results_to_dicts(p.slots[slot].read_results(0, N))
        assert [r["n_lines"] for r in recs] == [r["n_lines"] for r in world["recs"]]
        out = _check_batch(world, p.slots[slot], p.stream_of(slot), ("p1", 0), search)
        assert sum(r["valid"] for r in out) == N - 1
        p.close()


def test_classes_without_any_render_and_paint_needs_the_window(vision, world):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    d, s = world["d"], world["s"]
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"], stream=s)
    opt = _options(VIEW, WINDOW)
    with pytest.raises(smh.VisionError) as ei:
        fb2.read_reach(0, 1)
    assert ei.value.code == L.E_STATE
    with pytest.raises(smh.VisionError) as ei:
        fb2.reach_ptr()
    assert ei.value.code == L.E_STATE
    cls = fb2.reach(opt, smh.ReachOptions(origin=(150.0, 260.0), ring_m=RING, paint=False, classes=True), heightmap=world["hm"], stream=s)
    res = fb2.read_reach(0, N)
    for f in range(N):
        r = _want(world, world["recs"][f], (150.0, 260.0), True, RING)
        _same_classes(cls[f].cpu().numpy(), r["classes"], ("no render", f))
        _same_summary(res[f], r, ("no render", f))
    # the summary alone
    fb2.reach(opt, smh.ReachOptions(origin=(150.0, 260.0), ring_m=RING, paint=False, classes=False), first=1, n=1, heightmap=world["hm"], stream=s)
    _same_summary(fb2.read_reach(1, 1)[0], _want(world, world["recs"][1], (150.0, 260.0), True, RING), "summary alone")
    # PAINT before any render, and at a window that is not the most recent render's
    paint = smh.ReachOptions(origin=(150.0, 260.0), paint=True)
    with pytest.raises(smh.VisionError) as ei:
        fb2.reach(opt, paint, heightmap=world["hm"], stream=s)
    assert ei.value.code == L.E_STATE
    fb2.render(None, WINDOW[0], WINDOW[1], options=opt, stream=s)
    fb2.reach(opt, paint, heightmap=world["hm"], stream=s)
    for w, h in ((WINDOW[0] + 1, WINDOW[1]), (WINDOW[0], WINDOW[1] - 1), (WINDOW[1], WINDOW[0])):
        with pytest.raises(smh.VisionError) as ei:
            fb2.reach(_options(VIEW, (w, h)), paint, heightmap=world["hm"], stream=s)
        assert ei.value.code == L.E_STATE, (w, h)
    # ... which CLASSES alone does not mind
    other = (33, 17)
    cls = fb2.reach(_options(VIEW, other), smh.ReachOptions(origin=(150.0, 260.0), paint=False, classes=True), first=3, n=1, heightmap=world["hm"], stream=s)
    r = R.reach((150.0, 260.0), other, VIEW, world["recs"][3]["minimap"], world["recs"][3]["mpx"], world["hm_data"], True, 0.0)
    _same_classes(cls[0].cpu().numpy(), r["classes"], "another window")
    torch.cuda.synchronize()
    fb2.close()


def test_argument_errors_enqueue_nothing(vision, world, maps):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, s = world["fb"], world["s"]
    ow, oh = WINDOW
    opt = _options(VIEW, WINDOW)
    hm = world["hm"]._hm
    fb.render(None, ow, oh, options=opt, stream=s)
    good = smh.ReachOptions(origin=(150.0, 260.0), ring_m=RING, paint=True, classes=True)
    cls = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fb.reach(opt, good, heightmap=world["hm"], classes_ptr=cls.data_ptr(), stream=s)
    images = [fb.read_render(f).copy() for f in range(N)]
    slab = bytes(fb.read_reach(0, N))
    before = cls.cpu().numpy().copy()

    def options(**kw):
        o = good.struct()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    bad = [options(size=76), options(size=84), options(size=0), options(flags=4), options(flags=0x80000003), options(origin_mode=3),
           options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=32), options(origin_mode=L.REACH_ORIGIN_LINE_P1, line=0xFFFFFFFF),
           options(ring_m=-1.0), options(ring_m=float("nan")), options(ring_m=float("inf"))]
    dc, st = C.c_void_p(cls.data_ptr()), C.c_void_p(s)
    for i, o in enumerate(bad):
        assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(opt), C.byref(o), dc, st) == L.E_INVALID, i
    o = options()
    assert lib.smhv_batch_reach(None, 0, N, hm, C.byref(opt), C.byref(o), dc, st) == L.E_INVALID
    assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(opt), None, dc, st) == L.E_INVALID
    assert lib.smhv_batch_reach(fb._b, 0, N, hm, None, C.byref(o), dc, st) == L.E_INVALID
    assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(opt), C.byref(o), None, st) == L.E_INVALID          # CLASSES and no memory
    assert lib.smhv_batch_reach(fb._b, 1, N, hm, C.byref(opt), C.byref(o), dc, st) == L.E_INVALID            # beyond the capacity
    assert lib.smhv_batch_reach(fb._b, 0, 0, hm, C.byref(opt), C.byref(o), dc, st) == L.E_INVALID
    wrong = _options(VIEW, WINDOW)
    wrong.size = 8
    assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(wrong), C.byref(o), dc, st) == L.E_INVALID
    wrong = _options(VIEW, WINDOW)
    wrong.flags = 0x40
    assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(wrong), C.byref(o), dc, st) == L.E_INVALID
    for w, h in ((0, oh), (ow, 0), (16385, oh)):
        assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(_options(VIEW, (w, h))), C.byref(o), dc, st) == L.E_INVALID, (w, h)
    assert lib.smhv_batch_reach(fb._b, 0, N, hm, C.byref(_options(VIEW, (ow + 1, oh))), C.byref(o), dc, st) == L.E_STATE          # a stale window
    out1 = (L.ReachResult * 1)()
    assert lib.smhv_batch_read_reach(fb._b, 1, N, out1) == L.E_INVALID
    assert lib.smhv_batch_read_reach(fb._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_reach_ptr(fb._b, None) == L.E_INVALID
    torch.cuda.synchronize()
    for f in range(N):
        assert np.array_equal(fb.read_render(f), images[f]), f
    assert bytes(fb.read_reach(0, N)) == slab and np.array_equal(cls.cpu().numpy(), before)
    # the per-call path: the same checks, a line origin and two null outputs besides; image, classes and result stay as they were
    img = np.full((oh, ow, 4), 77, np.uint8)
    cb = np.full((oh, ow), 0xEE, np.uint8)
    res = L.ReachResult()
    C.memset(C.byref(res), 0x5A, 64)
    args = (img.ctypes.data, cb.ctypes.data, C.byref(res))
    for i, wrong in enumerate(bad + [options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=0)]):
        assert lib.smhv_reach_map(vision._ctx, hm, C.byref(opt), C.byref(wrong), None, None, *args) == L.E_INVALID, i
    assert lib.smhv_reach_map(vision._ctx, hm, C.byref(opt), C.byref(o), None, None, None, None, C.byref(res)) == L.E_INVALID
    assert lib.smhv_reach_map(vision._ctx, hm, C.byref(opt), None, None, None, *args) == L.E_INVALID
    assert lib.smhv_reach_map(vision._ctx, hm, None, C.byref(o), None, None, *args) == L.E_INVALID
    assert lib.smhv_reach_map(None, hm, C.byref(opt), C.byref(o), None, None, *args) == L.E_INVALID
    assert (img == 77).all() and (cb == 0xEE).all() and bytes(res) == b"\x5a" * 64
    # a correct call follows, without a result
    mpx = C.c_double(21.0)
    assert lib.smhv_reach_map(vision._ctx, hm, C.byref(opt), C.byref(o), C.byref(mpx), None, img.ctypes.data, cb.ctypes.data, None) == 0
    r = R.reach((150.0, 260.0), WINDOW, VIEW, None, 21.0, world["hm_data"], True, RING)
    _same_classes(cb, r["classes"], "after the failed calls")
    assert np.array_equal(img, R.paint(np.full((oh, ow, 4), 77, np.uint8), r["classes"]))
    _check_batch(world, fb, s, (150.0, 260.0), "after the failed calls")
