"""The terrain relief on the device (smhv_batch_relief / smhv_relief_map), every comparison exact: flag bytes, shades, heights, painted
image and summary equal to the restatement (tests/relief_ref.py) byte for byte and bit for bit -- per call for every case of
tests/relief_cases.py, on a plain batch in every form of the kernel, on a slot of both pipeline schedules and in parts; and the
heights tied to smhv_firing_solutions of the same points."""
import ctypes as C
import struct

import numpy as np
import pytest

import firing_ref as FR
import minimap_scenes as S
import relief_cases as RC
import relief_ref as R

pytestmark = pytest.mark.gpu

N = 4                                                            # frames of the batches: scenes 0, 7, the closed one, 1
SCENES = (0, 7, S.N_SCENES - 1, 1)
CLOSED = 2
WINDOW = (97, 66)                                                # two tiles across with one column in the second, five down with two rows in the last
VIEW = (0.26, 0.11, 1.25, -0.5)                                  # the 360 x 585 ROI of the scenes into that window, a scale per axis
OPT = R.options(interval_m=5.0, major_every=3, contour=(250, 10, 20, 140), major=(3, 4, 5, 231), shade_weight=77)


def _options(viewport, window, fit=True):
    import squad_mortar_helper_amd as smh
    sw, sh, tx, ty = viewport or (1.0, 1.0, 0.0, 0.0)
    vp = smh.MapViewport((0.0, 0.0, float(window[0]), float(window[1])), (sw, sh), (tx, ty))
    return smh.render_options(vp, window[0], window[1], heightmap=False, markers=True, fit_to_minimap=fit, background=(9, 8, 7, 255))


def _relief_options(opt, **kw):
    import squad_mortar_helper_amd as smh
    return smh.ReliefOptions(**dict(opt, **kw))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_plane(got, want, what, ctx):
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, what, got.shape, want.shape, got.dtype)
    a, b = (_bits(got), _bits(want)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d %s differ" % (len(bad), what), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // RC.TW, y // RC.TH),
                              "got", got[y, x], "want", want[y, x]))


def _same_summary(res, r, ctx):
    want = R.summary(r)
    got = dict(valid=int(res.valid), n_height=int(res.n_height), n_contour=int(res.n_contour), n_major=int(res.n_major), z_min=float(res.z_min),
               z_max=float(res.z_max))
    assert got == want and tuple(res.reserved) == (0, 0, 0, 0), (ctx, got, want)
    # (as bits too: -0.0 does not slip through ==)
    assert struct.pack("<dd", res.z_min, res.z_max) == struct.pack("<dd", want["z_min"], want["z_max"]), (ctx, got, want)


@pytest.fixture(scope="module")
def maps(vision):
    """The cases' heightmaps on the device, one copy each."""
    import squad_mortar_helper_amd as smh
    made = {}

    def get(hm):
        if id(hm[0]) not in made:
            made[id(hm[0])] = smh.Heightmap(vision, hm[0], hm[1], hm[2])
        return made[id(hm[0])]
    yield get
    for h in made.values():
        h.close()


def _per_call(vision, maps, c, paint=True, seed=5, **kw):
    ow, oh = c.window
    opt = _options(c.viewport, c.window, c.fit)
    base = np.random.default_rng(seed).integers(0, 256, size=(oh, ow, 4)).astype(np.uint8)
    img = base.copy() if paint else None
    fb, sh, hs, res = vision.relief_map(opt, _relief_options(c.opt), minimap=c.minimap, heightmap=maps(c.hm), image=img, **kw)
    return base, img, fb, sh, hs, res


@pytest.mark.parametrize("case", RC.all_cases(), ids=lambda c: c.name)
def test_every_case_on_the_per_call_path(vision, maps, case):
    r = RC.checked(case)
    base, img, fb, sh, hs, res = _per_call(vision, maps, case)
    _same_plane(fb, r["bytes"], "flag bytes", case.name)
    _same_plane(hs, r["heights"], "heights", case.name)
    _same_plane(sh, r["shades"], "shades", case.name)
    assert np.array_equal(img, R.paint(base.copy(), r, case.opt)), case.name
    assert np.array_equal(img[..., 3], base[..., 3])
    if case.name == "all weights 0":
        assert np.array_equal(img, base)
    _same_summary(res, r, case.name)


def test_each_output_alone(vision, maps):
    case = next(c for c in RC.all_cases() if c.name == "window 65 x 17")
    r = RC.checked(case)
    base, img, fb, sh, hs, res = _per_call(vision, maps, case, bytes=False, shades=False, heights=False)
    assert fb is None and sh is None and hs is None and np.array_equal(img, R.paint(base.copy(), r, case.opt)) and not np.array_equal(img, base)
    _same_summary(res, r, "paint alone")
    for which in ("bytes", "shades", "heights"):
        kw = dict(bytes=False, shades=False, heights=False)
        kw[which] = True
        _, img, fb, sh, hs, res = _per_call(vision, maps, case, paint=False, **kw)
        got = dict(bytes=fb, shades=sh, heights=hs)
        assert img is None and [k for k, v in got.items() if v is not None] == [which]
        _same_plane(got[which], r[which], which, which + " alone")
        _same_summary(res, r, which + " alone")
    # PAINT with a shade weight of 0 and no SHADES plane: the shade is not computed, and nothing shows it
    o = dict(case.opt, shade_weight=0)
    opt = _options(case.viewport, case.window, case.fit)
    img = base.copy()
    fb, _, _, res = vision.relief_map(opt, _relief_options(o), minimap=case.minimap, heightmap=maps(case.hm), image=img, shades=False, heights=False)
    _same_plane(fb, r["bytes"], "flag bytes", "no shade")
    assert np.array_equal(img, R.paint(base.copy(), r, o))


@pytest.mark.parametrize("name", ["integer coordinates, random", "magnified 8 x, nearest"])
def test_the_heights_are_the_firing_solutions(vision, maps, name):
    """Every pixel of the window against smhv_firing_solutions of the line from the pixel over texel (0, 0), which is 0, to it: its
    alt_delta is the height -- at integer coordinates for the bilinear rule, everywhere with NEAREST -- bit for bit."""
    case = next(c for c in RC.all_cases() if c.name == name)
    assert case.hm[0][0, 0] == 0
    r = RC.checked(case)
    ow, oh = case.window
    sw, sh, tx, ty = case.viewport or (1.0, 1.0, 0.0, 0.0)
    y, x = np.mgrid[0:oh, 0:ow]
    # the map-ROI point whose translation is the pixel's centre, exactly: (X + 0.5 - tx) / sw with sw = 1 and tx = 0 or 0.5
    ex, ey = (x + 0.5 - tx) / sw, (y + 0.5 - ty) / sh
    lines = np.stack([np.full(x.shape, ex[0, 0]), np.full(x.shape, ey[0, 0]), ex, ey], axis=-1).astype(np.float32).reshape(-1, 4)
    f = vision.firing_solutions(lines, minimap=case.minimap, heightmap=maps(case.hm), fit_to_minimap=case.fit, viewport=case.viewport)
    assert (f["source"] == FR.HEIGHTMAP).all()
    alt = np.ascontiguousarray(f["alt_delta"]).reshape(oh, ow)
    assert np.array_equal(alt.view(np.uint64), np.ascontiguousarray(r["z"]).view(np.uint64))
    _, _, _, _, hs, res = _per_call(vision, maps, case, paint=False, bytes=False, shades=False)
    _same_plane(hs, alt.astype(np.float32), "heights", name)
    assert struct.pack("<dd", res.z_min, res.z_max) == struct.pack("<dd", alt.min(), alt.max())


@pytest.fixture(scope="module")
def world(vision):
    """Four scenes of tests/minimap_scenes.py, the closed one among them, in a plain batch that has run once with the minimap stage and
    in another that has run without it: its frames have no minimap rectangle."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, anchor_list, rects, names = S.make_scenes()
    frames = np.ascontiguousarray(frames[list(SCENES)])
    anchor_list, names = [anchor_list[i] for i in SCENES], [names[i] for i in SCENES]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors(anchor_list)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    assert [r["map_open"] for r in recs] == [f != CLOSED for f in range(N)] and all(recs[f]["minimap"] is not None for f in range(N) if f != CLOSED)
    bare = smh.FrameBatch(vision, S.W, S.H, N)
    bare.run(d.data_ptr(), N, stages=smh.STAGE_ALL, grayscale=False, anchors=anchors, stream=s)
    bare_recs = smh.results_to_dicts(bare.read_results(0, N))
    assert all(r["minimap"] is None for r in bare_recs) and bare_recs[0]["map_open"]
    hm_data = RC.pyramid()
    hm = smh.Heightmap(vision, *hm_data)
    w = dict(d=d, s=s, anchors=anchors, names=names, fb=fb, recs=recs, bare=bare, bare_recs=bare_recs, stages=stages, hm=hm, hm_data=hm_data)
    yield w
    hm.close()
    bare.close()
    fb.close()


def _want(world, rec, opt, fit=True, window=WINDOW):
    return R.relief(window, VIEW, rec["minimap"] if rec["map_open"] else None, world["hm_data"], fit, opt)


def _check_batch(world, b, recs, stream, ctx, opt=OPT, parts=None, fit=True, paint=True, planes=True):
    """Render, read the images, run the relief (in `parts`: [(first, n)]), hold every frame against the restatement -> the restatements."""
    import torch
    ow, oh = WINDOW
    ropt = _options(VIEW, WINDOW, fit)
    b.render(None, ow, oh, options=ropt, stream=stream)
    base = [b.read_render(f).copy() for f in range(N)]
    ro = _relief_options(opt, paint=paint, bytes=planes, shades=planes, heights=planes)
    fbytes = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    shades = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    heights = torch.full((N, oh, ow), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for first, n in parts or [(0, N)]:
        kw = dict(bytes_ptr=fbytes[first].data_ptr(), shades_ptr=shades[first].data_ptr(), heights_ptr=heights[first].data_ptr()) if planes else {}
        assert b.relief(ropt, ro, first=first, n=n, heightmap=world["hm"], stream=stream, **kw) == {}
    res = b.read_relief(0, N)
    fbytes, shades, heights = fbytes.cpu().numpy(), shades.cpu().numpy(), heights.cpu().numpy()
    out = []
    for f in range(N):
        r = _want(world, recs[f], opt, fit)
        where = (ctx, f, world["names"][f])
        if planes:
            _same_plane(fbytes[f], r["bytes"], "flag bytes", where)
            _same_plane(heights[f], r["heights"], "heights", where)
            _same_plane(shades[f], r["shades"], "shades", where)
        else:
            assert (fbytes[f] == 0xEE).all() and (shades[f] == 0xEE).all() and (heights[f] == -7.0).all(), where
        assert np.array_equal(b.read_render(f), R.paint(base[f].copy(), r, opt) if paint else base[f]), where
        _same_summary(res[f], r, where)
        if not r["valid"]:
            assert bytes(res[f]) == bytes(48) and np.array_equal(b.read_render(f), base[f]), where
        out.append(r)
    return out


def test_a_plain_batch_in_every_form(vision, world):
    fb, s, recs = world["fb"], world["s"], world["recs"]
    out = _check_batch(world, fb, recs, s, "paint and planes")
    assert [r["valid"] for r in out] == [1, 1, 0, 1]
    assert all(RC._counts(r)[2] >= 10 for r in out if r["valid"]) and len(set(int(v) for r in out for v in np.unique(r["shades"]))) >= 10
    assert len(set(R.summary(r)["n_height"] for r in out)) >= 3      # the frames differ
    _check_batch(world, fb, recs, s, "paint alone", planes=False)
    _check_batch(world, fb, recs, s, "planes alone", paint=False)
    _check_batch(world, fb, recs, s, "the summary alone", paint=False, planes=False)
    _check_batch(world, fb, recs, s, "nearest, bounds offset", opt=dict(OPT, nearest=True, interval_m=20.0), fit=False)
    assert fb.relief_ptr() != 0


def test_frames_without_a_minimap_rectangle_and_a_range(vision, world):
    out = _check_batch(world, world["bare"], world["bare_recs"], world["s"], "no rectangle")
    assert not any(r["valid"] for r in out)
    _check_batch(world, world["fb"], world["recs"], world["s"], "parts", parts=[(3, 1), (0, 3)])
    _check_batch(world, world["fb"], world["recs"], world["s"], "parts of one", parts=[(0, 1), (1, 1), (2, 2)], opt=dict(OPT, interval_m=0.0))
    # a range first > 0 alone: the frames before it keep what they had
    import torch
    fb, s = world["fb"], world["s"]
    ropt = _options(VIEW, WINDOW)
    before = bytes(fb.read_relief(0, 1))
    got = fb.relief(ropt, _relief_options(dict(OPT, base_m=1.0), paint=False, bytes=True), first=1, n=2, heightmap=world["hm"], stream=s)
    assert sorted(got) == ["bytes"] and tuple(got["bytes"].shape) == (2, WINDOW[1], WINDOW[0])
    torch.cuda.synchronize()
    r = _want(world, world["recs"][1], dict(OPT, base_m=1.0))
    _same_plane(got["bytes"][0].cpu().numpy(), r["bytes"], "flag bytes", "first = 1")
    assert not got["bytes"][1].any() and bytes(fb.read_relief(0, 1)) == before
    _same_summary(fb.read_relief(1, 1)[0], r, "first = 1")


def test_a_slot_of_both_pipeline_schedules(vision, world):
    import squad_mortar_helper_amd as smh
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, S.W, S.H, N, depth=3, search=search)
        slot = p.submit(world["d"].data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"])
        p.wait()
        recs = smh.results_to_dicts(p.slots[slot].read_results(0, N))
        assert [r["minimap"] for r in recs] == [r["minimap"] for r in world["recs"]]
        out = _check_batch(world, p.slots[slot], recs, p.stream_of(slot), search)
        assert sum(r["valid"] for r in out) == N - 1
        p.close()


def test_weights_of_zero_leave_the_render_as_it_is(vision, world):
    fb, s = world["fb"], world["s"]
    ow, oh = WINDOW
    ropt = _options(VIEW, WINDOW)
    fb.render(None, ow, oh, options=ropt, stream=s)
    alone = [fb.read_render(f).copy() for f in range(N)]
    zero = dict(OPT, contour=(1, 2, 3, 0), major=(4, 5, 6, 0), shade_weight=0)
    fb.render(None, ow, oh, options=ropt, stream=s)
    fb.relief(ropt, _relief_options(zero), heightmap=world["hm"], stream=s)
    res = fb.read_relief(0, N)
    for f in range(N):
        assert np.array_equal(fb.read_render(f), alone[f]), f
        _same_summary(res[f], _want(world, world["recs"][f], zero), f)
    assert res[0].n_contour > 0


def test_paint_needs_the_most_recent_render_and_argument_errors_enqueue_nothing(vision, world):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    d, s = world["d"], world["s"]
    ow, oh = WINDOW
    ropt = _options(VIEW, WINDOW)
    hm = world["hm"]._hm
    fb2 = smh.FrameBatch(vision, S.W, S.H, N)
    fb2.run(d.data_ptr(), N, stages=world["stages"], grayscale=False, anchors=world["anchors"], stream=s)
    for call in (lambda: fb2.read_relief(0, 1), fb2.relief_ptr, lambda: fb2.relief(ropt, _relief_options(OPT), heightmap=world["hm"], stream=s)):
        with pytest.raises(smh.VisionError) as ei:                  # no relief yet; PAINT before any render
            call()
        assert ei.value.code == L.E_STATE
    fb2.relief(ropt, _relief_options(OPT, paint=False), first=1, n=1, heightmap=world["hm"], stream=s)      # the summary alone needs no render
    _same_summary(fb2.read_relief(1, 1)[0], _want(world, world["recs"][1], OPT), "no render")
    fb2.render(None, ow, oh, options=ropt, stream=s)
    fb2.relief(ropt, _relief_options(OPT), heightmap=world["hm"], stream=s)
    for w, h in ((ow + 1, oh), (ow, oh - 1), (oh, ow)):
        with pytest.raises(smh.VisionError) as ei:
            fb2.relief(_options(VIEW, (w, h)), _relief_options(OPT), heightmap=world["hm"], stream=s)
        assert ei.value.code == L.E_STATE, (w, h)
    other = (33, 17)                                               # ... which the planes alone do not mind
    got = fb2.relief(_options(VIEW, other), _relief_options(OPT, paint=False, heights=True), first=3, n=1, heightmap=world["hm"], stream=s)
    _same_plane(got["heights"][0].cpu().numpy(), _want(world, world["recs"][3], OPT, window=other)["heights"], "heights", "another window")
    # what is refused, and that it leaves the images, the slab and the planes as they were
    good = _relief_options(OPT, bytes=True, shades=True, heights=True)
    planes = [torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda"),
              torch.full((N, oh, ow), -7.0, dtype=torch.float32, device="cuda")]
    torch.cuda.synchronize()
    fb2.render(None, ow, oh, options=ropt, stream=s)
    fb2.relief(ropt, good, heightmap=world["hm"], bytes_ptr=planes[0].data_ptr(), shades_ptr=planes[1].data_ptr(), heights_ptr=planes[2].data_ptr(), stream=s)
    images = [fb2.read_render(f).copy() for f in range(N)]
    slab = bytes(fb2.read_relief(0, N))
    before = [p.cpu().numpy().copy() for p in planes]

    def options(**kw):
        o = good.struct()
        for k, v in kw.items():
            if k == "light":
                for i in range(3):
                    o.light[i] = v[i]
            else:
                setattr(o, k, v)
        return o
    nan, inf = float("nan"), float("inf")
    bad = [options(size=76), options(size=84), options(size=0), options(flags=32), options(flags=0x8000000F), options(interval_m=-1.0), options(interval_m=nan),
           options(interval_m=inf), options(base_m=nan), options(base_m=-inf), options(exaggeration=inf), options(exaggeration=nan),
           options(light=(nan, 0.0, 1.0)), options(light=(0.0, inf, 1.0)), options(light=(0.0, 0.0, -inf)), options(shade_weight=256),
           options(shade_weight=0xFFFFFFFF)]
    pl = L.ReliefPlanes(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr())
    st = C.c_void_p(s)
    for i, o in enumerate(bad):
        assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(ropt), C.byref(o), C.byref(pl), st) == L.E_INVALID, i
    o = options()
    assert lib.smhv_batch_relief(None, 0, N, hm, C.byref(ropt), C.byref(o), C.byref(pl), st) == L.E_INVALID
    assert lib.smhv_batch_relief(fb2._b, 0, N, None, C.byref(ropt), C.byref(o), C.byref(pl), st) == L.E_INVALID       # relief without terrain
    assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(ropt), None, C.byref(pl), st) == L.E_INVALID
    assert lib.smhv_batch_relief(fb2._b, 0, N, hm, None, C.byref(o), C.byref(pl), st) == L.E_INVALID
    assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(ropt), C.byref(o), None, st) == L.E_INVALID                # plane flags and no planes
    for k in range(3):                                             # a plane flag with a null pointer
        ptrs = [planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr()]
        ptrs[k] = None
        assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(ropt), C.byref(o), C.byref(L.ReliefPlanes(*ptrs)), st) == L.E_INVALID, k
    assert lib.smhv_batch_relief(fb2._b, 1, N, hm, C.byref(ropt), C.byref(o), C.byref(pl), st) == L.E_INVALID         # beyond the capacity
    assert lib.smhv_batch_relief(fb2._b, 0, 0, hm, C.byref(ropt), C.byref(o), C.byref(pl), st) == L.E_INVALID
    wrong = _options(VIEW, WINDOW)
    wrong.size = 8
    assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(wrong), C.byref(o), C.byref(pl), st) == L.E_INVALID
    wrong = _options(VIEW, WINDOW)
    wrong.flags = 0x40
    assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(wrong), C.byref(o), C.byref(pl), st) == L.E_INVALID
    for w, h in ((0, oh), (ow, 0), (16385, oh)):
        assert lib.smhv_batch_relief(fb2._b, 0, N, hm, C.byref(_options(VIEW, (w, h))), C.byref(o), C.byref(pl), st) == L.E_INVALID, (w, h)
    out1 = (L.ReliefResult * 1)()
    assert lib.smhv_batch_read_relief(fb2._b, 1, N, out1) == L.E_INVALID
    assert lib.smhv_batch_read_relief(fb2._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_relief_ptr(fb2._b, None) == L.E_INVALID
    torch.cuda.synchronize()
    for f in range(N):
        assert np.array_equal(fb2.read_render(f), images[f]), f
    assert bytes(fb2.read_relief(0, N)) == slab and all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(planes, before))
    # the per-call path: the same checks, and no output at all; image, planes and result stay as they were
    img = np.full((oh, ow, 4), 77, np.uint8)
    pb, ps, ph = np.full((oh, ow), 0xEE, np.uint8), np.full((oh, ow), 0xEE, np.uint8), np.full((oh, ow), -7.0, np.float32)
    res = L.ReliefResult()
    C.memset(C.byref(res), 0x5A, 48)
    mm = (C.c_uint32 * 4)(*world["recs"][0]["minimap"])
    args = (img.ctypes.data, pb.ctypes.data, ps.ctypes.data, ph.ctypes.data, C.byref(res))
    for i, wrong in enumerate(bad):
        assert lib.smhv_relief_map(vision._ctx, hm, C.byref(ropt), C.byref(wrong), mm, *args) == L.E_INVALID, i
    assert lib.smhv_relief_map(vision._ctx, hm, C.byref(ropt), C.byref(o), mm, None, None, None, None, None) == L.E_INVALID
    assert lib.smhv_relief_map(vision._ctx, None, C.byref(ropt), C.byref(o), mm, *args) == L.E_INVALID
    assert lib.smhv_relief_map(vision._ctx, hm, C.byref(ropt), None, mm, *args) == L.E_INVALID
    assert lib.smhv_relief_map(vision._ctx, hm, None, C.byref(o), mm, *args) == L.E_INVALID
    assert lib.smhv_relief_map(None, hm, C.byref(ropt), C.byref(o), mm, *args) == L.E_INVALID
    assert (img == 77).all() and (pb == 0xEE).all() and (ps == 0xEE).all() and (ph == -7.0).all() and bytes(res) == b"\x5a" * 48
    # a correct call follows, the result alone
    assert lib.smhv_relief_map(vision._ctx, hm, C.byref(ropt), C.byref(o), mm, None, None, None, None, C.byref(res)) == 0
    _same_summary(res, _want(world, world["recs"][0], OPT), "after the failed calls")
    torch.cuda.synchronize()
    fb2.close()
