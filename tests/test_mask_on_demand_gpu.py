"""The marker mask as bytes, made on demand (include/smh_vision_hip.h, smhv_batch_device_ptrs; k_mask_expand): the streaming passes of
a batch run write the bit rows (and the tile-major mask) only, and the byte form comes from the bit rows when one of its readers asks.

Sizes from tests/geometry_sweep_cases.py where the expansion can go wrong -- rw 33 at m_xoff 3 (a second word column of one pixel),
rw 31, m_quads 65 (a wave edge at column 255) and 257, rh 901 (58-row bands, bit rows only) and rh 900 (the tile-major path) -- each
through the fused pass (all stages) and the plain pass (markers + ui_map).  Everything byte for byte against the oracle's mask."""
import ctypes as C

import numpy as np
import pytest

import geometry_sweep_cases as G
import web_views_ref as V

pytestmark = pytest.mark.gpu

SIZES = [(347, 363), (343, 361), (568, 361), (1336, 361), (1097, 1184), (1118, 1182)]
CASES = [next(c for c in G.CASES if (c.W, c.H) == s) for s in SIZES]
KINDS = {"fused": 0xF, "plain": 0x3}                                  # k_map_brq_pass (all stages) / k_map_pass (markers + ui_map)
OPEN_A, CLOSED, OPEN_B = 0, 1, 2                                       # make_frames: an open frame, a closed one, another open one
A8 = [OPEN_A, OPEN_B] * 4
B4 = [OPEN_B, OPEN_A] * 2
BG = (0, 0, 0, 255)


@pytest.fixture(scope="module", params=CASES, ids=["%dx%d" % s for s in SIZES])
def world(request, vision):
    import torch
    c = request.param
    frames, infos, refs = G.oracle_of(c)
    assert refs[OPEN_A]["map_open"] and refs[OPEN_B]["map_open"] and not refs[CLOSED]["map_open"]
    assert not np.array_equal(refs[OPEN_A]["lsd"], refs[OPEN_B]["lsd"]) and (refs[OPEN_A]["lsd"] == 255).sum() >= 50
    w = dict(c=c, refs=refs, d=torch.from_numpy(frames).cuda(), per=[(i["scales_start_y"], i["anchors"]) for i in infos],
             s=torch.cuda.current_stream().cuda_stream)
    yield w
    w.clear()
    torch.cuda.empty_cache()


@pytest.fixture(params=sorted(KINDS))
def kind(request):
    return request.param


def _pick(w, order):
    """(device frames, anchors) of the case's frames in `order`."""
    import torch
    import squad_mortar_helper_amd as smh
    return w["d"][torch.tensor(order, device="cuda")].contiguous(), smh.make_anchors([w["per"][i] for i in order])


def _args(w, order, kind):
    import torch
    d, anchors = _pick(w, order)
    torch.cuda.synchronize()
    return d, dict(stages=KINDS[kind], max_gap=G.MAX_GAP, anchors=anchors if KINDS[kind] & 0x8 else None)


def _run(fb, w, order, kind):
    d, kw = _args(w, order, kind)
    fb.run(d.data_ptr(), len(order), stream=w["s"], **kw)
    return d                                                           # (the caller keeps the frames alive until it has read)


def _mask(fb, f):
    import squad_mortar_helper_amd as smh
    return fb.read_image(smh._lib.VIEW_LSD_INPUT, f)


def _expand(fb, f):
    """The frame's bit rows as the batch holds them, expanded on the host: byte x = 0xFF where bit x + bits_xoff is set."""
    _, _, bits, xoff = fb.tile_mask(f)
    x = np.arange(fb.roi[2]) + xoff
    return (((bits[:, x >> 5] >> (x & 31).astype(np.uint32)) & 1) * 255).astype(np.uint8)


def test_mask_against_the_oracle(vision, world, kind):
    """After a lazy run the mask read is the oracle's for every open frame, a second read returns the same bytes, and the bit rows
    expand to the same image.  The two tall sizes also with as many frames as give the launch its full-height bands (58 / 62 rows
    without the tile-major mask at rh 901, 24 rows with it at rh 900)."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    runs = [[OPEN_A, CLOSED, OPEN_B]]
    if c.rh >= 900:
        runs.append([OPEN_A, CLOSED, OPEN_B] * 11)
    for order in runs:
        n = len(order)
        fb = smh.FrameBatch(vision, c.W, c.H, n)
        try:
            assert fb.mask_state() == (0, False)
            d = _run(fb, world, order, kind)
            assert fb.mask_state() == (n, False)
            for f in sorted({0, 2, n - 3, n - 1}):
                want = refs[order[f]]["lsd"]
                got = _mask(fb, f)
                assert fb.mask_state() == (0, False)
                assert np.array_equal(got, want), (c, kind, n, f)
                assert np.array_equal(_mask(fb, f), got), (c, kind, n, f, "second read")
                assert np.array_equal(_expand(fb, f), want), (c, kind, n, f, "bit rows")
            del d
        finally:
            fb.close()


@pytest.mark.parametrize("read_between", [False, True], ids=["no_read_between", "read_between"])
def test_high_water_mark(vision, world, kind, read_between):
    """Run A over 8 frames, run B over the first 4 with other content, read all 8: frames 0-3 show B, frames 4-7 A."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    fb = smh.FrameBatch(vision, c.W, c.H, 8)
    try:
        da = _run(fb, world, A8, kind)
        assert fb.mask_state() == (8, False)
        if read_between:
            assert np.array_equal(_mask(fb, 7), refs[A8[7]]["lsd"])
            assert fb.mask_state() == (0, False)
        db = _run(fb, world, B4, kind)
        assert fb.mask_state() == (4 if read_between else 8, False)
        for f in range(8):
            want = refs[B4[f] if f < 4 else A8[f]]["lsd"]
            assert np.array_equal(_mask(fb, f), want), (c, kind, read_between, f)
        assert fb.mask_state() == (0, False)
        del da, db
    finally:
        fb.close()


def test_closed_frames_keep_the_older_mask(vision, world, kind):
    """A frame whose button is closed, after a run in which it was open: the passes skip it (aux.open == 0), so its bit rows stay
    the earlier run's -- and so did the bytes the passes' epilogues used to write beside them, which is what a read returned
    before the byte form was made on demand.  The mask read is that earlier run's, and the expansion of the frame's current bit rows."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    fb = smh.FrameBatch(vision, c.W, c.H, 3)
    try:
        d1 = _run(fb, world, [OPEN_A, OPEN_B, OPEN_A], kind)
        d2 = _run(fb, world, [OPEN_B, CLOSED, CLOSED], kind)
        recs = smh.results_to_dicts(fb.read_results(0, 3))
        assert [r["map_open"] for r in recs] == [1, 0, 0]
        for f, src in ((0, OPEN_B), (1, OPEN_B), (2, OPEN_A)):
            got = _mask(fb, f)
            assert np.array_equal(got, refs[src]["lsd"]), (c, kind, f)
            assert np.array_equal(got, _expand(fb, f)), (c, kind, f)
        del d1, d2
    finally:
        fb.close()


def test_asking_for_d_mask_switches_the_batch_to_eager(vision, world, kind):
    """smhv_batch_device_ptrs with a non-NULL d_mask: the bytes of the runs so far are there when it returns, and every later run's are
    in memory when its stream gets there -- a plain device-to-host copy on the run's stream, no library call in between.  A batch
    asked for its records only stays lazy."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    fb = smh.FrameBatch(vision, c.W, c.H, 3)
    lazy = smh.FrameBatch(vision, c.W, c.H, 3)
    try:
        ly = fb.layout
        nb = int(ly.mask_stride) * 3
        host = np.empty(nb, np.uint8)

        def copy_out():
            assert hip.hipMemcpyAsync(host.ctypes.data, C.c_void_p(mask_ptr), nb, 2, C.c_void_p(world["s"])) == 0   # hipMemcpyDeviceToHost
            assert hip.hipStreamSynchronize(C.c_void_p(world["s"])) == 0
            img = host.reshape(3, c.rh, int(ly.mask_pitch))
            return img[:, :, int(ly.mask_offset):int(ly.mask_offset) + c.rw]
        order1, order2 = [OPEN_A, CLOSED, OPEN_B], [OPEN_B, OPEN_A, OPEN_A]
        d1 = _run(fb, world, order1, kind)
        ptrs = fb.device_ptrs()
        assert ptrs["results"] and ptrs["bits"] and fb.mask_state() == (3, False)     # the mapping has not asked for d_mask
        mask_ptr = ptrs["mask"]
        assert mask_ptr and fb.mask_state() == (0, True) and ptrs["mask"] == mask_ptr
        got = copy_out()
        for f in (0, 2):
            assert np.array_equal(got[f], refs[order1[f]]["lsd"]), (c, kind, "at the switch", f)
        d2, kw = _args(world, order2, kind)
        fb.run(d2.data_ptr(), 3, stream=world["s"], **kw)
        got = copy_out()                                                # <- nothing of the library between the run and the copy
        assert fb.mask_state() == (0, True)
        for f in range(3):
            assert np.array_equal(got[f], refs[order2[f]]["lsd"]), (c, kind, "eager run", f)
        # the other batch: its records' pointer, a run, the same again -- never eager, the bytes owed until somebody reads them
        assert lazy.device_ptrs()["results"]
        d3 = _run(lazy, world, order2, kind)
        assert sorted(lazy.device_ptrs()) == sorted(("results", "ui", "mask", "ocr", "scales", "bits")) and lazy.device_ptrs()["ui"]
        assert lazy.mask_state() == (3, False)
        assert np.array_equal(_mask(lazy, 1), refs[order2[1]]["lsd"]) and lazy.mask_state() == (0, False)
        del d1, d2, d3
    finally:
        fb.close()
        lazy.close()


def _render_mask(b, first, n, stream):
    import squad_mortar_helper_amd as smh
    import render_ref as RR
    rw, rh = b.roi[2], b.roi[3]
    quad, scale, top_left = RR.identity(rw, rh)
    b.render(smh.MapViewport(quad, scale, top_left), rw, rh, first=first, n=n, background=BG, stream=stream,
             layers=smh.RenderLayers((), map_source=smh._lib.VIEW_LSD_INPUT))


def _feed_mask(b, feed, n, stream):
    import squad_mortar_helper_amd as smh
    b.feed(feed, first=0, n=n, stream=stream, map_source=smh._lib.VIEW_LSD_INPUT)
    return [(int(f), int(k), int(crc), bytes(data)) for f, k, crc, data in feed.read()[1]]


def _feed_capacity(n, rw, rh):
    import web_ref as W
    return 6 + n * (32 + W.slot(10 + rw * rh * 4) + W.slot(7 + 16 * 32))   # (every frame's UpdateState, Map and Markers at their largest)


@pytest.mark.parametrize("search,depth", [("frame", 3), ("batch", 2)], ids=["frame_granular_depth3", "batch_granular_depth2"])
def test_pipeline_slots(vision, world, kind, search, depth):
    """Seven submissions of 8 frames, so that the slots come round: the mask read from each slot after wait(slot) is that of a plain batch
    given the same runs as the slot (and the oracle's).  Then, on slots whose mask nobody has read since their last submission: the map
    view with the mask as the map and the feed of the mask view are what a plain batch gives whose mask was read first -- the
    expansion is ordered ahead of both on a fresh slot."""
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    orders = [A8, B4 + B4, [OPEN_A, CLOSED] * 4, A8[::-1], B4 + A8[:4], [CLOSED, OPEN_B] * 4, A8]
    plains = [smh.FrameBatch(vision, c.W, c.H, 8) for _ in range(depth)]   # one per slot, run over what the slot is given: the same history
    pipe = smh.Pipeline(vision, c.W, c.H, 8, depth, search=search)
    feed = smh.WebFeed(vision, _feed_capacity(8, c.rw, c.rh), 8)
    try:
        kept, slot_of, last = [], [], {}
        for k, order in enumerate(orders):
            d, kw = _args(world, order, kind)
            kept.append(d)
            slot = pipe.submit(d.data_ptr(), 8, **kw)
            slot_of.append(slot)
            last[slot] = k
            plain = plains[slot]
            kept.append(_run(plain, world, order, kind))
            if k < 4:                                                  # read while the pipeline is young: every slot once, and one again
                pipe.wait(slot)
                for f in range(8):
                    want = _mask(plain, f)
                    assert np.array_equal(_mask(pipe.slots[slot], f), want), (c, kind, search, k, f)
                    if refs[order[f]]["map_open"]:
                        assert np.array_equal(want, refs[order[f]]["lsd"]), (c, kind, search, k, f)
        assert slot_of == [k % depth for k in range(7)]
        # two slots nobody has looked at since their last submission: the render on one, the feed on the other
        fresh = sorted(last, key=last.get)[-2:]
        for slot, what in zip(fresh, ("render", "feed")):
            order = orders[last[slot]]
            pipe.wait(slot)
            b = pipe.slots[slot]
            assert b.mask_state()[0] == 8
            plain = plains[slot]
            for f in range(8):
                _mask(plain, f)                                        # the plain batch's bytes are there before its render / feed
            st = pipe.stream_of(slot)
            if what == "render":
                _render_mask(plain, 0, 8, world["s"])
                want = [plain.read_render(f).copy() for f in range(8)]
                _render_mask(b, 0, 8, st)
                for f in range(8):
                    got = b.read_render(f)
                    assert np.array_equal(got, want[f]), (c, kind, search, "render", f)
                    if refs[order[f]]["map_open"]:
                        assert np.array_equal(got, V.gray(refs[order[f]]["lsd"])), (c, kind, search, "render against the oracle", f)
            else:
                feed.reset()
                want = _feed_mask(plain, feed, 8, world["s"])
                feed.reset()
                got = _feed_mask(b, feed, 8, st)
                assert got == want and len(got) >= 8, (c, kind, search, "feed")
                payload = V.gray(refs[order[0]]["lsd"]).tobytes()
                assert refs[order[0]]["map_open"] and any(payload in m[3] for m in got), (c, kind, search, "feed against the oracle")
            assert b.mask_state()[0] == 0
        pipe.wait()
    finally:
        feed.close()
        pipe.close()
        for plain in plains:
            plain.close()
        del kept


def test_two_consumers_on_two_streams(vision, world, kind):
    """The map view on stream X and the feed on stream Y, back to back on a batch whose bytes are owed: the first expands on its
    stream, the second waits for that expansion on its own.  Both are what they are on a batch whose mask was read first."""
    import torch
    import squad_mortar_helper_amd as smh
    c, refs = world["c"], world["refs"]
    fb = smh.FrameBatch(vision, c.W, c.H, 8)
    feed = smh.WebFeed(vision, _feed_capacity(8, c.rw, c.rh), 8)
    sx, sy = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        d = _run(fb, world, A8, kind)
        for f in range(8):
            _mask(fb, f)
        _render_mask(fb, 0, 8, world["s"])
        want_render = [fb.read_render(f).copy() for f in range(8)]
        want_feed = _feed_mask(fb, feed, 8, world["s"])
        assert np.array_equal(want_render[1], V.gray(refs[A8[1]]["lsd"]))
        for first in ("render", "feed"):
            d2 = _run(fb, world, B4 + B4, kind)                          # other content in between, so that stale bytes would show
            for f in range(8):
                _mask(fb, f)
            d3 = _run(fb, world, A8, kind)
            torch.cuda.synchronize()                                   # the run is complete: X and Y are ordered behind it
            assert fb.mask_state() == (8, False)
            feed.reset()
            if first == "render":
                _render_mask(fb, 0, 8, sx.cuda_stream)
                fb.feed(feed, first=0, n=8, stream=sy.cuda_stream, map_source=smh._lib.VIEW_LSD_INPUT)
            else:
                fb.feed(feed, first=0, n=8, stream=sy.cuda_stream, map_source=smh._lib.VIEW_LSD_INPUT)
                _render_mask(fb, 0, 8, sx.cuda_stream)
            assert fb.mask_state() == (0, False)
            got_feed = [(int(f), int(k), int(crc), bytes(data)) for f, k, crc, data in feed.read()[1]]
            assert got_feed == want_feed, (c, kind, first, "feed")
            for f in range(8):
                assert np.array_equal(fb.read_render(f), want_render[f]), (c, kind, first, "render", f)
            del d2, d3
        del d
    finally:
        feed.close()
        fb.close()
