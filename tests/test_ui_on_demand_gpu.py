"""The grey ui_map as a luma plane, its RGBA slab made on demand (include/smh_vision_hip.h, smhv_batch_device_ptrs; k_ui_expand): a grey
batch run writes one luma byte per pixel, and d_ui is made from the plane when one of its readers asks.  Colour runs, overlay runs and
the runs of a batch whose caller holds d_ui write RGBA directly, and a frame a run finds closed keeps its older image in whichever
form holds it -- a byte per frame on the device says which.

The sizes of tests/test_mask_on_demand_gpu.py (m_xoff 3, a wave edge at column 255, 257 quads, 58-row bands, the tile-major path), each
through the fused pass (all stages) and the plain pass (markers + ui_map).  Everything byte for byte against the oracle's ui_map (grey)
and ui_colour."""
import ctypes as C

import numpy as np
import pytest

import geometry_sweep_cases as G

pytestmark = pytest.mark.gpu

SIZES = [(347, 363), (343, 361), (568, 361), (1336, 361), (1097, 1184), (1118, 1182)]
CASES = [next(c for c in G.CASES if (c.W, c.H) == s) for s in SIZES]
KINDS = {"fused": 0xF, "plain": 0x3}                                  # k_map_brq_pass (all stages) / k_map_pass (markers + ui_map)
OPEN_A, CLOSED, OPEN_B = 0, 1, 2                                       # make_frames: an open frame, a closed one, another open one
A8 = [OPEN_A, OPEN_B] * 4
B4 = [OPEN_B, CLOSED, OPEN_B, OPEN_A]                                  # differs from A8 in every frame it writes; frame 1 is closed
BG = (0, 0, 0, 255)


@pytest.fixture(scope="module", params=CASES, ids=["%dx%d" % s for s in SIZES])
def world(request, vision):
    import torch
    c = request.param
    frames, infos, refs = G.oracle_of(c)
    assert refs[OPEN_A]["map_open"] and refs[OPEN_B]["map_open"] and not refs[CLOSED]["map_open"]
    # the references tell the cases apart only if the oracle's own images differ where the cases need them to
    assert not np.array_equal(refs[OPEN_A]["ui_map"], refs[OPEN_B]["ui_map"])
    for i in (OPEN_A, OPEN_B):
        g, col = refs[i]["ui_map"], refs[i]["ui_colour"]
        assert g.shape == (c.rh, c.rw, 4) and col.shape == g.shape and not np.array_equal(g, col)
        assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2]) and (g[..., 3] == 255).all()   # (l,l,l,255)
    assert not np.array_equal(refs[OPEN_A]["ui_colour"], refs[OPEN_B]["ui_colour"])
    w = dict(c=c, refs=refs, d=torch.from_numpy(frames).cuda(), per=[(i["scales_start_y"], i["anchors"]) for i in infos],
             s=torch.cuda.current_stream().cuda_stream)
    yield w
    w.clear()
    torch.cuda.empty_cache()


@pytest.fixture(params=sorted(KINDS))
def kind(request):
    return request.param


def _args(w, order, kind, extra_stages=0):
    import torch
    import squad_mortar_helper_amd as smh
    d = w["d"][torch.tensor(order, device="cuda")].contiguous()
    anchors = smh.make_anchors([w["per"][i] for i in order])
    torch.cuda.synchronize()
    return d, dict(stages=KINDS[kind] | extra_stages, max_gap=G.MAX_GAP, anchors=anchors if KINDS[kind] & 0x8 else None)


def _run(fb, w, order, kind, gray=True, extra_stages=0):
    d, kw = _args(w, order, kind, extra_stages)
    fb.run(d.data_ptr(), len(order), stream=w["s"], grayscale=gray, **kw)
    return d                                                           # (the caller keeps the frames alive until it has read)


def _ui(fb, f):
    import squad_mortar_helper_amd as smh
    return fb.read_image(smh._lib.IMAGE_UI_MAP, f)


def _want(refs, src, gray=True):
    return refs[src]["ui_map" if gray else "ui_colour"]


def test_ui_against_the_oracle(vision, world, kind):
    """After a lazy grey run the ui_map read is the oracle's for every open frame and a second read returns the same bytes.  The two
    tall sizes also with as many frames as give the launch its full-height bands."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    runs = [[OPEN_A, CLOSED, OPEN_B]]
    if c.rh >= 900:
        runs.append([OPEN_A, CLOSED, OPEN_B] * 11)
    for order in runs:
        n = len(order)
        fb = smh.FrameBatch(vision, c.W, c.H, n)
        try:
            assert fb.ui_state() == (0, False)
            d = _run(fb, world, order, kind)
            assert fb.ui_state() == (n, False)
            for f in sorted({0, 2, n - 3, n - 1}):
                got = _ui(fb, f)
                assert fb.ui_state() == (0, False)
                assert np.array_equal(got, _want(refs, order[f])), (c, kind, n, f)
                assert np.array_equal(_ui(fb, f), got), (c, kind, n, f, "second read")
            assert not np.any(_ui(fb, 1)), (c, kind, n, "a closed frame of a fresh batch: the zeros of its creation")
            del d
        finally:
            fb.close()


@pytest.mark.parametrize("read_between", [False, True], ids=["no_read_between", "read_between"])
def test_closed_frames_and_the_high_water_mark(vision, world, kind, read_between):
    """Run A over 8 frames, run B over the first 4 with frame 1 closed, read all 8: frames 0, 2, 3 show B, frame 1 still A, 4-7 A."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    fb = smh.FrameBatch(vision, c.W, c.H, 8)
    try:
        da = _run(fb, world, A8, kind)
        assert fb.ui_state() == (8, False)
        if read_between:
            assert np.array_equal(_ui(fb, 7), _want(refs, A8[7]))
            assert fb.ui_state() == (0, False)
        db = _run(fb, world, B4, kind)
        assert fb.ui_state() == (4 if read_between else 8, False)
        recs = smh.results_to_dicts(fb.read_results(0, 4))
        assert [r["map_open"] for r in recs] == [1, 0, 1, 1]
        for f in range(8):
            src = B4[f] if f < 4 and B4[f] != CLOSED else A8[f]
            assert np.array_equal(_ui(fb, f), _want(refs, src)), (c, kind, read_between, f)
        assert fb.ui_state() == (0, False)
        del da, db
    finally:
        fb.close()


def test_mixed_forms_per_frame(vision, world, kind):
    """A frame's newest image is in whichever form its last open run wrote: colour then grey with frame 1 closed -- frame 1 still reads
    colour; grey then colour with frame 1 closed, nothing read in between -- frame 1 reads the older grey image.  A frame no run has
    written reads zeros, alpha included."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    first, second = [OPEN_A, OPEN_B, OPEN_A], [OPEN_B, CLOSED, OPEN_B]
    for gray1 in (False, True):
        fb = smh.FrameBatch(vision, c.W, c.H, 4)
        try:
            d1 = _run(fb, world, first, kind, gray=gray1)
            assert fb.ui_state() == ((3, False) if gray1 else (0, False))
            d2 = _run(fb, world, second, kind, gray=not gray1)
            assert fb.ui_state() == (3, False)                         # (the mark of whichever run was grey: only flagged frames expand)
            for f in (1, 0, 2):
                want = _want(refs, first[1], gray1) if f == 1 else _want(refs, second[f], not gray1)
                assert np.array_equal(_ui(fb, f), want), (c, kind, gray1, f)
            assert fb.ui_state() == (0, False)
            assert not np.any(_ui(fb, 3)), (c, kind, gray1, "never written")
            del d1, d2
        finally:
            fb.close()


def test_asking_for_d_ui_switches_the_batch_to_eager(vision, world, kind):
    """smhv_batch_device_ptrs with a non-NULL d_ui: the slab is up to date when it returns, and every later grey run's RGBA is in memory
    when its stream gets there -- a plain device-to-host copy of the whole slab on the run's stream, no library call in between, equal
    to the slab of a lazy batch with the same history once that has been materialised, padded columns included.  A batch asked for its
    records only stays lazy."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    fb = smh.FrameBatch(vision, c.W, c.H, 3)
    lazy = smh.FrameBatch(vision, c.W, c.H, 3)
    try:
        ly = fb.layout
        nb = int(ly.ui_stride) * 3
        assert int(ly.ui_stride) == int(ly.ui_pitch) * c.rh

        def copy_out(ptr):
            host = np.empty(nb, np.uint8)
            assert hip.hipMemcpyAsync(host.ctypes.data, C.c_void_p(ptr), nb, 2, C.c_void_p(world["s"])) == 0   # hipMemcpyDeviceToHost
            assert hip.hipStreamSynchronize(C.c_void_p(world["s"])) == 0
            return host.reshape(3, c.rh, int(ly.ui_pitch))

        def roi(slab, f):
            return slab[f, :, int(ly.ui_offset):int(ly.ui_offset) + 4 * c.rw].reshape(c.rh, c.rw, 4)
        order1, order2 = [OPEN_A, CLOSED, OPEN_B], [OPEN_B, OPEN_A, OPEN_A]
        d1 = _run(fb, world, order1, kind)
        ptrs = fb.device_ptrs()
        assert ptrs["results"] and ptrs["bits"] and fb.ui_state() == (3, False)       # the mapping has not asked for d_ui
        ui_ptr = ptrs["ui"]
        assert ui_ptr and fb.ui_state() == (0, True) and ptrs["ui"] == ui_ptr
        got = copy_out(ui_ptr)
        for f in (0, 2):
            assert np.array_equal(roi(got, f), _want(refs, order1[f])), (c, kind, "at the switch", f)
        assert not np.any(got[1]), (c, kind, "the closed frame at the switch")
        d2, kw = _args(world, order2, kind)
        fb.run(d2.data_ptr(), 3, stream=world["s"], **kw)
        got = copy_out(ui_ptr)                                          # <- nothing of the library between the run and the copy
        assert fb.ui_state() == (0, True)
        for f in range(3):
            assert np.array_equal(roi(got, f), _want(refs, order2[f])), (c, kind, "eager run", f)
        # the lazy batch: its records' pointer, the same two runs -- never eager, the slab owed until somebody asks
        assert lazy.device_ptrs()["results"]
        d3 = _run(lazy, world, order1, kind)
        d4 = _run(lazy, world, order2, kind)
        assert lazy.ui_state() == (3, False)
        lazy_ptr = lazy.device_ptrs()["ui"]                             # (materialises what the lazy runs owe, then hands the slab out)
        assert lazy.ui_state() == (0, True)
        want = copy_out(lazy_ptr)
        assert np.array_equal(got, want), (c, kind, "whole slab, padded columns included", np.argwhere(got != want)[:4])
        del d1, d2, d3, d4
    finally:
        fb.close()
        lazy.close()


def _render_ui(b, first, n, stream):
    import squad_mortar_helper_amd as smh
    import render_ref as RR
    rw, rh = b.roi[2], b.roi[3]
    quad, scale, top_left = RR.identity(rw, rh)
    b.render(smh.MapViewport(quad, scale, top_left), rw, rh, first=first, n=n, background=BG, stream=stream)


def _feed_ui(b, feed, n, stream):
    b.feed(feed, first=0, n=n, stream=stream)
    return [(int(f), int(k), int(crc), bytes(data)) for f, k, crc, data in feed.read()[1]]


def _feed_capacity(n, rw, rh):
    import web_ref as W
    return 6 + n * (32 + W.slot(10 + rw * rh * 4) + W.slot(7 + 16 * 32))   # (every frame's UpdateState, Map and Markers at their largest)


def test_readers_on_other_streams(vision, world, kind):
    """The map view at the identity viewport on stream X and the feed on stream Y, back to back on a batch whose slab is owed: the
    first expands on its stream, the second waits for that expansion on its own.  Both are what an eager batch gives."""
    import torch
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    fb = smh.FrameBatch(vision, c.W, c.H, 8)
    eager = smh.FrameBatch(vision, c.W, c.H, 8)
    feed = smh.WebFeed(vision, _feed_capacity(8, c.rw, c.rh), 8)
    sx, sy = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        assert eager.device_ptrs()["ui"] and eager.ui_state() == (0, True)
        de = _run(eager, world, A8, kind)
        _render_ui(eager, 0, 8, world["s"])
        want_render = [eager.read_render(f).copy() for f in range(8)]
        want_feed = _feed_ui(eager, feed, 8, world["s"])
        assert eager.ui_state() == (0, True)
        payload = _want(refs, A8[0]).tobytes()
        assert any(payload in m[3] for m in want_feed), (c, kind, "the feed's Map against the oracle")
        for first in ("render", "feed"):
            d2 = _run(fb, world, B4 + B4, kind)                          # other content in between, so that a stale slab would show
            for f in range(8):
                _ui(fb, f)
            d3 = _run(fb, world, A8, kind)
            torch.cuda.synchronize()                                   # the run is complete: X and Y are ordered behind it
            assert fb.ui_state() == (8, False)
            feed.reset()
            if first == "render":
                _render_ui(fb, 0, 8, sx.cuda_stream)
                fb.feed(feed, first=0, n=8, stream=sy.cuda_stream)
            else:
                fb.feed(feed, first=0, n=8, stream=sy.cuda_stream)
                _render_ui(fb, 0, 8, sx.cuda_stream)
            assert fb.ui_state() == (0, False)
            got_feed = [(int(f), int(k), int(crc), bytes(data)) for f, k, crc, data in feed.read()[1]]
            assert got_feed == want_feed, (c, kind, first, "feed")
            for f in range(8):
                assert np.array_equal(fb.read_render(f), want_render[f]), (c, kind, first, "render", f)
            del d2, d3
        del de
    finally:
        feed.close()
        fb.close()
        eager.close()


@pytest.mark.parametrize("depth", [2, 12])
def test_pipeline(vision, world, kind, depth):
    """A pipeline of 3-frame submissions, grey: the ui_map read from the last slot is the oracle's, and an earlier slot still holds its own."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    orders = [[OPEN_A, CLOSED, OPEN_B], [OPEN_B, OPEN_A, CLOSED], [OPEN_B, OPEN_B, OPEN_A]]
    pipe = smh.Pipeline(vision, c.W, c.H, 3, depth)
    try:
        kept, slots = [], []
        for order in orders:
            d, kw = _args(world, order, kind)
            kept.append(d)
            slots.append(pipe.submit(d.data_ptr(), 3, **kw))
        assert len(set(slots)) == min(depth, 3)
        for k in (2, 1):
            pipe.wait(slots[k])
            b = pipe.slots[slots[k]]
            assert b.ui_state() == (3, False)
            for f in range(3):
                if orders[k][f] != CLOSED:
                    assert np.array_equal(_ui(b, f), _want(refs, orders[k][f])), (c, kind, depth, k, f)
            assert b.ui_state() == (0, False)
        pipe.wait()
        del kept
    finally:
        pipe.close()


def test_overlay_stage_on_a_lazy_batch(vision, world, kind):
    """A run with the overlay stage reads the ui_map inside the run: it writes RGBA itself, behind the expansion of what earlier grey
    runs owe the slab.  The overlay is the restatement's over the oracle's grey ui_map and what an eager batch gives; the frame the
    run finds closed keeps the earlier run's image."""
    import firing_ref as R
    import overlay_ref as O
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    data = np.random.default_rng(11).integers(0, 65536, size=(97, 131), dtype=np.uint16)
    bounds = ((-7, 5), (0, 0))
    hm = smh.Heightmap(vision, data, bounds, (1.0, 1.0, 1.0))
    cm = R.color_map(data)
    extra = smh.STAGE_MINIMAP | smh.STAGE_HEIGHTMAP_OVERLAY
    first, second = [OPEN_B, OPEN_A, OPEN_A], [OPEN_A, CLOSED, OPEN_B]
    fb = smh.FrameBatch(vision, c.W, c.H, 3)
    eager = smh.FrameBatch(vision, c.W, c.H, 3)
    try:
        assert eager.device_ptrs()["ui"]
        got = {}
        for name, b in (("lazy", fb), ("eager", eager)):
            b.set_firing(hm, fit_to_minimap=True)
            d1 = _run(b, world, first, kind)
            assert b.ui_state() == ((3, False) if name == "lazy" else (0, True))
            d2 = _run(b, world, second, kind, extra_stages=extra)
            assert b.ui_state()[0] == 0                                # the overlay run owes nothing: the slab is RGBA
            recs = smh.results_to_dicts(b.read_results(0, 3))
            assert [r["map_open"] for r in recs] == [1, 0, 1]
            got[name] = [b.read_overlay(f).copy() for f in range(3)]
            for f in (0, 2):
                want = O.overlay(_want(refs, second[f]), recs[f]["minimap"], cm, bounds[0][0], bounds[0][1], True)
                assert np.array_equal(got[name][f], want), (c, kind, name, f)
                assert np.array_equal(_ui(b, f), _want(refs, second[f])), (c, kind, name, f)
            assert np.array_equal(_ui(b, 1), _want(refs, first[1])), (c, kind, name, "the closed frame keeps the earlier run's image")
            del d1, d2
        for f in range(3):
            assert np.array_equal(got["lazy"][f], got["eager"][f]), (c, kind, f)
    finally:
        fb.close()
        eager.close()
        hm.close()
