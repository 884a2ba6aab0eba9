"""The map grid on the device (smhv_batch_grid / smhv_grid_map / smhv_batch_grid_refs / smhv_grid_refs), every comparison exact: flag
bytes, cell words, painted image, summary and references equal to the restatement (tests/grid_ref.py) byte for byte, word for word
and bit for bit -- per call for every case of tests/grid_cases.py, on a plain batch in every form of the kernel and on both sources,
in parts, on a slot of both pipeline schedules; the references tied to the cell words of the same points."""
import ctypes as C
import struct

import numpy as np
import pytest

import grid_cases as GC
import grid_ref as G
import minimap_scenes as S

pytestmark = pytest.mark.gpu

N = 4                                                            # frames of the batches: scenes 0, 7, the closed one, 1
SCENES = (0, 7, S.N_SCENES - 1, 1)
CLOSED = 2
WINDOW = GC.WINDOW
VIEW = (0.26, 0.11, 1.25, -0.5)                                  # the 360 x 585 ROI of the scenes into that window, a scale per axis
HM = (700, 480, ((7, -5), (0, 0)))                               # the map's size in metres and its bounds: cells of 8 to 16 pixels with OPT
OPT = G.options(cell_m=150.0, levels=2, origin_m=(-20.0, 35.0), min_px=1.0, label_min_px=5.0, line=GC.LINE, label=GC.LABEL)
OPT_SCALES = G.options(cell_m=150.0, levels=1, min_px=2.0, label_min_px=5.0, line=GC.LINE, label=GC.LABEL)


def _options(viewport, window, fit=True):
    import squad_mortar_helper_amd as smh
    sw, sh, tx, ty = viewport or (1.0, 1.0, 0.0, 0.0)
    vp = smh.MapViewport((0.0, 0.0, float(window[0]), float(window[1])), (sw, sh), (tx, ty))
    return smh.render_options(vp, window[0], window[1], heightmap=False, markers=True, fit_to_minimap=fit, background=(9, 8, 7, 255))


def _grid_options(opt, **kw):
    import squad_mortar_helper_amd as smh
    return smh.GridOptions(**dict(opt, **kw))


def _same_plane(got, want, what, ctx):
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x = (int(v) for v in bad[0])
        raise AssertionError((ctx, "%d %s differ" % (len(bad), what), "first (y, x)", bad[:4].tolist(), "tile (x, y)", (x // GC.TW, y // GC.TH),
                              "got", hex(int(got[y, x])), "want", hex(int(want[y, x]))))


def _same_summary(res, r, ctx):
    want = G.summary(r)
    got = dict(valid=int(res.valid), source=int(res.source), drawn_levels=int(res.drawn_levels), n_cell=int(res.n_cell), n_line=tuple(res.n_line),
               n_label=int(res.n_label), col_first=int(res.col_first), col_last=int(res.col_last), row_first=int(res.row_first), row_last=int(res.row_last))
    assert got == want and tuple(res.reserved) == (0, 0, 0), (ctx, got, want)


def _ref_bytes(p):
    return struct.pack("<ddII3BBI16s", p["x_m"], p["y_m"], p["col"], p["row1"], *p["digit"], p["valid"], 0, p["text"])


def _same_refs(got, want, ctx):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert bytes(g) == _ref_bytes(w), (ctx, i, bytes(g).hex(), w)


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


def _per_call(vision, maps, c, paint=True, seed=5, **kw):
    ow, oh = c.window
    opt = _options(c.viewport, c.window, c.fit)
    base = np.random.default_rng(seed).integers(0, 256, size=(oh, ow, 4)).astype(np.uint8)
    img = base.copy() if paint else None
    fb, cw, res = vision.grid_map(opt, _grid_options(c.opt), mpx=c.mpx, minimap=c.minimap, heightmap=maps(c.hm), image=img, **kw)
    return base, img, fb, cw, res


@pytest.mark.parametrize("case", GC.all_cases(), ids=lambda c: c.name)
def test_every_case_on_the_per_call_path(vision, maps, case):
    r, (source, refs) = GC.checked(case)
    base, img, fb, cw, res = _per_call(vision, maps, case)
    _same_plane(fb, r["bytes"], "flag bytes", case.name)
    _same_plane(cw, r["cells"], "cell words", case.name)
    assert np.array_equal(img, G.paint(base.copy(), r, case.opt)), case.name
    assert np.array_equal(img[..., 3], base[..., 3])
    _same_summary(res, r, case.name)
    got = vision.grid_refs(case.lines, _options(case.viewport, case.window, case.fit), _grid_options(case.opt), mpx=case.mpx, minimap=case.minimap,
                           heightmap=maps(case.hm))
    _same_refs(got, refs, case.name)


def test_each_output_alone_and_weights_of_zero(vision, maps):
    case = next(c for c in GC.all_cases() if c.name == "cell 300, levels 3")
    r, _ = GC.checked(case)
    base, img, fb, cw, res = _per_call(vision, maps, case, bytes=False, cells=False)
    assert fb is None and cw is None and np.array_equal(img, G.paint(base.copy(), r, case.opt)) and not np.array_equal(img, base)
    _same_summary(res, r, "paint alone")
    for which in ("bytes", "cells"):
        kw = dict(bytes=False, cells=False)
        kw[which] = True
        _, img, fb, cw, res = _per_call(vision, maps, case, paint=False, **kw)
        got = dict(bytes=fb, cells=cw)
        assert img is None and [k for k, v in got.items() if v is not None] == [which]
        _same_plane(got[which], r[which], which, which + " alone")
        _same_summary(res, r, which + " alone")
    # line weights of 0 leave the pixels as they are; a label weight of 0 draws no label and sets no LABEL bit
    zero = dict(case.opt, line=tuple((1, 2, 3, 0) for _ in range(4)), label=(4, 5, 6, 0))
    rz = GC.restate(case, **zero)
    assert not rz["lit"].any() and r["lit"].any() and np.array_equal(rz["level"], r["level"])
    img = base.copy()
    fb, cw, res = vision.grid_map(_options(case.viewport, case.window, case.fit), _grid_options(zero), minimap=case.minimap, heightmap=maps(case.hm), image=img)
    assert np.array_equal(img, base)
    _same_plane(fb, rz["bytes"], "flag bytes", "weights of 0")
    _same_summary(res, rz, "weights of 0")


def test_the_reference_of_a_pixel_centre_is_the_pixel_cell_word(vision, maps):
    """Every pixel of a window through smhv_grid_refs as the point at its centre: col, row1 and the digits are the cell word's, valid is
    HAS_CELL -- the two kernels run one rule."""
    for name in ("cell 300, levels 3", "the origin inside the window", "bounds offset, a non-square heightmap"):
        case = next(c for c in GC.all_cases() if c.name == name)
        assert case.viewport is None                                # the map-ROI point X + 0.5 translates to the pixel's centre exactly
        ow, oh = case.window
        opt = _options(case.viewport, case.window, case.fit)
        fb, cw, _ = vision.grid_map(opt, _grid_options(case.opt), minimap=case.minimap, heightmap=maps(case.hm))
        y, x = np.mgrid[0:oh, 0:ow]
        pts = np.stack([x + 0.5, y + 0.5], axis=-1).astype(np.float32).reshape(-1, 2)
        lines = np.concatenate([pts, pts[::-1]], axis=1)              # line i: pixel i and pixel n - 1 - i
        refs = vision.grid_refs(lines, opt, _grid_options(case.opt), minimap=case.minimap, heightmap=maps(case.hm))
        raw = np.frombuffer(refs, np.uint8).reshape(-1, 2, 48)
        for end, order in ((0, slice(None)), (1, slice(None, None, -1))):
            rec = np.ascontiguousarray(raw[:, end][order])
            col, row1 = rec[:, 16:20].copy().view(np.uint32)[:, 0], rec[:, 20:24].copy().view(np.uint32)[:, 0]
            d = rec[:, 24:27].astype(np.uint32)
            word = col | row1 << 10 | d[:, 0] << 20 | d[:, 1] << 24 | d[:, 2] << 28
            assert np.array_equal(word.reshape(oh, ow), cw), (name, end)
            assert np.array_equal(rec[:, 27].reshape(oh, ow), fb & G.HAS_CELL), (name, end)
        assert (fb & G.HAS_CELL).any()


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
    assert all(recs[f]["mpx"] is not None and recs[f]["n_lines"] >= 1 for f in range(N) if f != CLOSED)
    bare = smh.FrameBatch(vision, S.W, S.H, N)
    bare.run(d.data_ptr(), N, stages=smh.STAGE_ALL, grayscale=False, anchors=anchors, stream=s)
    bare_recs = smh.results_to_dicts(bare.read_results(0, N))
    assert all(r["minimap"] is None for r in bare_recs) and bare_recs[0]["map_open"]
    hm_data = GC.heightmap(*HM)
    hm = smh.Heightmap(vision, *hm_data)
    w = dict(d=d, s=s, anchors=anchors, names=names, fb=fb, recs=recs, bare=bare, bare_recs=bare_recs, stages=stages, hm=hm, hm_data=hm_data)
    yield w
    hm.close()
    bare.close()
    fb.close()


def _want(world, rec, opt, fit=True, window=WINDOW, scales=False):
    mm = rec["minimap"] if rec["map_open"] else None
    return G.grid(window, VIEW, mm, None if scales else world["hm_data"], fit, rec["mpx"] if scales else None, opt)


def _want_refs(world, rec, opt, fit=True, scales=False):
    mm = rec["minimap"] if rec["map_open"] else None
    return G.line_refs(rec["lines"], VIEW, mm, None if scales else world["hm_data"], fit, rec["mpx"] if scales else None, opt)


def _check_batch(world, b, recs, stream, ctx, opt=OPT, parts=None, fit=True, paint=True, planes=True, scales=False):
    """Render, read the images, run the grid (in `parts`: [(first, n)]) and the references, hold every frame against the restatement."""
    import torch
    ow, oh = WINDOW
    ropt = _options(VIEW, WINDOW, fit)
    hm = None if scales else world["hm"]
    b.render(None, ow, oh, options=ropt, stream=stream)
    base = [b.read_render(f).copy() for f in range(N)]
    go = _grid_options(opt, paint=paint, bytes=planes, cells=planes)
    fbytes = torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    cells = torch.full((N, oh, ow), -0x11111112, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for first, n in parts or [(0, N)]:
        kw = dict(bytes_ptr=fbytes[first].data_ptr(), cells_ptr=cells[first].data_ptr()) if planes else {}
        assert b.grid(ropt, go, first=first, n=n, heightmap=hm, stream=stream, **kw) == {}
        b.grid_refs(ropt, go, first=first, n=n, heightmap=hm, stream=stream)
    res = b.read_grid(0, N)
    refs = b.read_grid_refs(0, N)
    fbytes, cells = fbytes.cpu().numpy(), cells.cpu().numpy().view(np.uint32)
    out = []
    for f in range(N):
        r = _want(world, recs[f], opt, fit, scales=scales)
        where = (ctx, f, world["names"][f])
        if planes:
            _same_plane(fbytes[f], r["bytes"], "flag bytes", where)
            _same_plane(cells[f], r["cells"], "cell words", where)
        else:
            assert (fbytes[f] == 0xEE).all() and (cells[f] == 0xEEEEEEEE).all(), where
        img = b.read_render(f)
        assert np.array_equal(img, G.paint(base[f].copy(), r, opt) if paint else base[f]), where
        assert np.array_equal(img[..., 3], base[f][..., 3]) and (not paint or not r["valid"] or not np.array_equal(img, base[f])), where
        _same_summary(res[f], r, where)
        if not r["valid"]:
            assert bytes(res[f]) == bytes(64) and np.array_equal(b.read_render(f), base[f]), where
        source, want = _want_refs(world, recs[f], opt, fit, scales=scales)
        n_lines = recs[f]["n_lines"]
        raw = bytes(refs[f])
        assert struct.unpack("<4I", raw[:16]) == (n_lines, source, 0, 0), where
        _same_refs([raw[16 + 48 * i:64 + 48 * i] for i in range(2 * n_lines)], want, where)
        assert raw[16 + 96 * n_lines:] == bytes(3072 - 96 * n_lines), where
        out.append(r)
    return out


def test_a_plain_batch_in_every_form_and_on_both_sources(vision, world):
    fb, s, recs = world["fb"], world["s"], world["recs"]
    out = _check_batch(world, fb, recs, s, "paint and planes")
    assert [r["valid"] for r in out] == [1, 1, 0, 1]
    sums = [G.summary(r) for r in out if r["valid"]]
    assert all(t["n_cell"] > 500 and t["n_line"][0] > 50 and t["n_line"][1] > 50 and t["n_label"] > 20 and t["drawn_levels"] >= 2 for t in sums), sums
    assert len(set(t["n_cell"] for t in sums)) == 3                 # the frames differ
    _check_batch(world, fb, recs, s, "paint alone", planes=False)
    _check_batch(world, fb, recs, s, "planes alone", paint=False)
    _check_batch(world, fb, recs, s, "the summary alone", paint=False, planes=False)
    _check_batch(world, fb, recs, s, "bounds offset, three levels", opt=dict(OPT, levels=3, min_px=0.0), fit=False)
    out = _check_batch(world, fb, recs, s, "the scales branch", opt=OPT_SCALES, scales=True)
    sums = [G.summary(r) for r in out if r["valid"]]
    assert len(sums) == 3 and all(t["source"] == G.SCALES and t["n_cell"] > 500 and t["n_line"][0] > 50 and t["drawn_levels"] >= 1 for t in sums), sums
    assert fb.grid_ptr() != 0 and fb.grid_refs_ptr() != 0


def test_frames_without_a_minimap_rectangle_and_a_range(vision, world):
    out = _check_batch(world, world["bare"], world["bare_recs"], world["s"], "no rectangle")
    assert not any(r["valid"] for r in out)
    _check_batch(world, world["fb"], world["recs"], world["s"], "parts", parts=[(3, 1), (0, 3)])
    _check_batch(world, world["fb"], world["recs"], world["s"], "parts of one", parts=[(0, 1), (1, 1), (2, 2)], opt=dict(OPT, levels=0))
    # a range first > 0 alone: the frames before it keep what they had
    import torch
    fb, s = world["fb"], world["s"]
    ropt = _options(VIEW, WINDOW)
    before, before_refs = bytes(fb.read_grid(0, 1)), bytes(fb.read_grid_refs(0, 1))
    o = dict(OPT, cell_m=90.0)
    got = fb.grid(ropt, _grid_options(o, paint=False, cells=True), first=1, n=2, heightmap=world["hm"], stream=s)
    fb.grid_refs(ropt, _grid_options(o), first=1, n=2, heightmap=world["hm"], stream=s)
    assert sorted(got) == ["cells"] and tuple(got["cells"].shape) == (2, WINDOW[1], WINDOW[0])
    torch.cuda.synchronize()
    r = _want(world, world["recs"][1], o)
    _same_plane(got["cells"][0].cpu().numpy().view(np.uint32), r["cells"], "cell words", "first = 1")
    assert not got["cells"][1].any() and bytes(fb.read_grid(0, 1)) == before and bytes(fb.read_grid_refs(0, 1)) == before_refs
    _same_summary(fb.read_grid(1, 1)[0], r, "first = 1")


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
        _check_batch(world, p.slots[slot], recs, p.stream_of(slot), search + ", scales", opt=OPT_SCALES, scales=True)
        p.close()


def test_a_grid_call_first_on_a_fresh_batch_and_argument_errors_enqueue_nothing(vision, world):
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
    for call in (lambda: fb2.read_grid(0, 1), fb2.grid_ptr, lambda: fb2.read_grid_refs(0, 1), fb2.grid_refs_ptr,
                 lambda: fb2.grid(ropt, _grid_options(OPT), heightmap=world["hm"], stream=s)):
        with pytest.raises(smh.VisionError) as ei:                  # no grid yet; PAINT before any render
            call()
        assert ei.value.code == L.E_STATE
    # the first calls of a fresh batch, over one frame: the rest of both slabs is zero
    fb2.grid(ropt, _grid_options(OPT, paint=False), first=1, n=1, heightmap=world["hm"], stream=s)
    fb2.grid_refs(ropt, _grid_options(OPT), first=1, n=1, heightmap=world["hm"], stream=s)
    _same_summary(fb2.read_grid(1, 1)[0], _want(world, world["recs"][1], OPT), "no render")
    slab, rslab = bytes(fb2.read_grid(0, N)), bytes(fb2.read_grid_refs(0, N))
    assert slab[:64] == bytes(64) and slab[128:] == bytes(128) and slab[64:128] != bytes(64)
    assert rslab[:3088] == bytes(3088) and rslab[2 * 3088:] == bytes(2 * 3088) and rslab[3088:2 * 3088] != bytes(3088)
    fb2.render(None, ow, oh, options=ropt, stream=s)
    fb2.grid(ropt, _grid_options(OPT), heightmap=world["hm"], stream=s)
    for w, h in ((ow + 1, oh), (ow, oh - 1), (oh, ow)):
        with pytest.raises(smh.VisionError) as ei:
            fb2.grid(_options(VIEW, (w, h)), _grid_options(OPT), heightmap=world["hm"], stream=s)
        assert ei.value.code == L.E_STATE, (w, h)
    other = (33, 17)                                               # ... which the planes alone do not mind
    got = fb2.grid(_options(VIEW, other), _grid_options(OPT, paint=False, bytes=True), first=3, n=1, heightmap=world["hm"], stream=s)
    _same_plane(got["bytes"][0].cpu().numpy(), _want(world, world["recs"][3], OPT, window=other)["bytes"], "flag bytes", "another window")
    # what is refused, and that it leaves the images, the slabs and the planes as they were
    good = _grid_options(OPT, bytes=True, cells=True)
    planes = [torch.full((N, oh, ow), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((N, oh, ow), -7, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    fb2.render(None, ow, oh, options=ropt, stream=s)
    fb2.grid(ropt, good, heightmap=world["hm"], bytes_ptr=planes[0].data_ptr(), cells_ptr=planes[1].data_ptr(), stream=s)
    fb2.grid_refs(ropt, good, heightmap=world["hm"], stream=s)
    images = [fb2.read_render(f).copy() for f in range(N)]
    slab, rslab = bytes(fb2.read_grid(0, N)), bytes(fb2.read_grid_refs(0, N))
    before = [p.cpu().numpy().copy() for p in planes]

    def options(**kw):
        o = good.struct()
        for k, v in kw.items():
            if k == "origin_m":
                o.origin_m[0], o.origin_m[1] = v
            else:
                setattr(o, k, v)
        return o
    nan, inf = float("nan"), float("inf")
    bad = [options(size=76), options(size=84), options(size=0), options(flags=8), options(flags=0x80000007), options(cell_m=0.0), options(cell_m=-300.0),
           options(cell_m=nan), options(cell_m=inf), options(levels=4), options(levels=0xFFFFFFFF), options(origin_m=(nan, 0.0)), options(origin_m=(0.0, -inf)),
           options(min_px=-1.0), options(min_px=nan), options(min_px=inf), options(label_min_px=nan), options(label_min_px=-inf)]
    pl = L.GridPlanes(planes[0].data_ptr(), planes[1].data_ptr())
    st = C.c_void_p(s)

    def both(b, first, n, h, ro, o, p):
        """smhv_batch_grid and smhv_batch_grid_refs refuse the same arguments"""
        rc = lib.smhv_batch_grid(b, first, n, h, ro, o, p, st)
        assert lib.smhv_batch_grid_refs(b, first, n, h, ro, o, st) == rc
        return rc
    for i, o in enumerate(bad):
        assert both(fb2._b, 0, N, hm, C.byref(ropt), C.byref(o), C.byref(pl)) == L.E_INVALID, i
    o = options()
    assert both(None, 0, N, hm, C.byref(ropt), C.byref(o), C.byref(pl)) == L.E_INVALID
    assert both(fb2._b, 0, N, hm, C.byref(ropt), None, C.byref(pl)) == L.E_INVALID
    assert both(fb2._b, 0, N, hm, None, C.byref(o), C.byref(pl)) == L.E_INVALID
    assert lib.smhv_batch_grid(fb2._b, 0, N, hm, C.byref(ropt), C.byref(o), None, st) == L.E_INVALID                  # plane flags and no planes
    for k in range(2):                                             # a plane flag with a null pointer
        ptrs = [planes[0].data_ptr(), planes[1].data_ptr()]
        ptrs[k] = None
        assert lib.smhv_batch_grid(fb2._b, 0, N, hm, C.byref(ropt), C.byref(o), C.byref(L.GridPlanes(*ptrs)), st) == L.E_INVALID, k
    assert both(fb2._b, 1, N, hm, C.byref(ropt), C.byref(o), C.byref(pl)) == L.E_INVALID                              # beyond the capacity
    assert both(fb2._b, 0, 0, hm, C.byref(ropt), C.byref(o), C.byref(pl)) == L.E_INVALID
    wrong = _options(VIEW, WINDOW)
    wrong.size = 8
    assert both(fb2._b, 0, N, hm, C.byref(wrong), C.byref(o), C.byref(pl)) == L.E_INVALID
    wrong = _options(VIEW, WINDOW)
    wrong.flags = 0x40
    assert both(fb2._b, 0, N, hm, C.byref(wrong), C.byref(o), C.byref(pl)) == L.E_INVALID
    for w, h in ((0, oh), (ow, 0), (16385, oh)):
        assert both(fb2._b, 0, N, hm, C.byref(_options(VIEW, (w, h))), C.byref(o), C.byref(pl)) == L.E_INVALID, (w, h)
    out1 = (L.GridResult * 1)()
    assert lib.smhv_batch_read_grid(fb2._b, 1, N, out1) == L.E_INVALID and lib.smhv_batch_read_grid(fb2._b, 0, 1, None) == L.E_INVALID
    assert lib.smhv_batch_grid_ptr(fb2._b, None) == L.E_INVALID and lib.smhv_batch_grid_refs_ptr(fb2._b, None) == L.E_INVALID
    assert lib.smhv_batch_read_grid_refs(fb2._b, 1, N, (L.GridRefsResult * 1)()) == L.E_INVALID
    torch.cuda.synchronize()
    for f in range(N):
        assert np.array_equal(fb2.read_render(f), images[f]), f
    assert bytes(fb2.read_grid(0, N)) == slab and bytes(fb2.read_grid_refs(0, N)) == rslab
    assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(planes, before))
    # the per-call paths: the same checks, and no output at all; image, planes, result and references stay as they were
    img = np.full((oh, ow, 4), 77, np.uint8)
    pb, pc = np.full((oh, ow), 0xEE, np.uint8), np.full((oh, ow), 0xEEEEEEEE, np.uint32)
    res = L.GridResult()
    C.memset(C.byref(res), 0x5A, 64)
    refs = (L.GridRef * 2)()
    C.memset(refs, 0x5A, 96)
    mm = (C.c_uint32 * 4)(*world["recs"][0]["minimap"])
    line = (C.c_float * 4)(10.0, 20.0, 30.0, 40.0)
    args = (img.ctypes.data, pb.ctypes.data, pc.ctypes.data, C.byref(res))
    for i, wrong in enumerate(bad):
        assert lib.smhv_grid_map(vision._ctx, hm, C.byref(ropt), C.byref(wrong), None, mm, *args) == L.E_INVALID, i
        assert lib.smhv_grid_refs(vision._ctx, line, 1, None, mm, hm, C.byref(ropt), C.byref(wrong), refs) == L.E_INVALID, i
    assert lib.smhv_grid_map(vision._ctx, hm, C.byref(ropt), C.byref(o), None, mm, None, None, None, None) == L.E_INVALID
    assert lib.smhv_grid_map(vision._ctx, hm, C.byref(ropt), None, None, mm, *args) == L.E_INVALID
    assert lib.smhv_grid_map(vision._ctx, hm, None, C.byref(o), None, mm, *args) == L.E_INVALID
    assert lib.smhv_grid_map(None, hm, C.byref(ropt), C.byref(o), None, mm, *args) == L.E_INVALID
    assert lib.smhv_grid_refs(vision._ctx, None, 1, None, mm, hm, C.byref(ropt), C.byref(o), refs) == L.E_INVALID
    assert lib.smhv_grid_refs(vision._ctx, line, 1, None, mm, hm, C.byref(ropt), C.byref(o), None) == L.E_INVALID
    assert lib.smhv_grid_refs(vision._ctx, line, 1, None, mm, hm, None, C.byref(o), refs) == L.E_INVALID
    assert lib.smhv_grid_refs(vision._ctx, None, 0, None, mm, hm, C.byref(ropt), C.byref(o), None) == 0               # no line: nothing to do
    assert (img == 77).all() and (pb == 0xEE).all() and (pc == 0xEEEEEEEE).all() and bytes(res) == b"\x5a" * 64 and bytes(refs) == b"\x5a" * 96
    # a correct call follows, the result alone
    assert lib.smhv_grid_map(vision._ctx, hm, C.byref(ropt), C.byref(o), None, mm, None, None, None, C.byref(res)) == 0
    _same_summary(res, _want(world, world["recs"][0], OPT), "after the failed calls")
    torch.cuda.synchronize()
    fb2.close()
