"""A debug view as the remote-viewer feed's Map (smhv_batch_feed_view / smhv_feed_frame_view), byte for byte against the restatement
(tests/web_views_ref.py over tests/web_ref.py: numpy, struct.pack and zlib.crc32), no tolerance and no excluded cases: every view
at frame sizes whose quarter starts at every column residue and has every width residue, at every split of the rows over the
waves and in both forms of a plane's CRC; one changed source pixel; the rule, its state and a switch of the source; the capacity
measured with the source's size; the state and argument errors; the identity with smhv_batch_feed; both pipeline schedules; the
per-call path against smhv_get_debug_view; and that feeding moves nothing else."""
import zlib

import numpy as np
import pytest

import render_geometry_cases as G
import render_ref as RR
import web_ref as W
import web_views_ref as V
from fixtures import MANIFEST, load_fixture
from test_firing_gpu import _frames_with_minimaps
from test_web_gpu import SEQ, _same

pytestmark = pytest.mark.gpu

BG = G.BG


def _planes(fb, f):
    """What the views of frame f are made from, as the batch holds them."""
    from squad_mortar_helper_amd import _lib as L
    return dict(ui=fb.read_image(L.IMAGE_UI_MAP, f), mask=fb.read_image(L.VIEW_LSD_INPUT, f), ocr=fb.read_image(L.VIEW_OCR_INPUT, f),
                scales=fb.read_image(L.VIEW_FIND_SCALES_INPUT, f))


def _ref_frames(fb, first, n, which, planes=None):
    """The restatement's input for frames [first, first + n) under a source: the records, and the source's (w, h, bytes)."""
    out = []
    for i, r in enumerate(fb.read_results(first, n)):
        vb = None
        if r.map_open:
            p = planes[first + i] if planes is not None else _planes(fb, first + i)
            vb = (p["ui"].shape[1], p["ui"].shape[0], p["ui"].tobytes()) if which == V.VIEW_NONE else V.view_bytes(which, **p)
        lines = np.array([[l.x0, l.y0, l.x1, l.y1] for l in r.lines[:r.n_lines]], np.float32).reshape(-1, 4)
        out.append((bool(r.map_open), int(r.status), vb, lines, bool(r.has_mpx), float(r.mpx), bool(r.has_minimap), tuple(r.minimap)))
    return out


def _full(N, w, h):
    return 6 + N * (32 + W.slot(10 + w * h * 4) + W.slot(7 + 16 * 32))


def _frame_for(Wd, Ht):
    """A synthetic frame with a small block of near-white, equal-channel pixels in the bottom right quadrant, above the scale bars
    (the synthetic frames hold no text: without it the OCR input is all 255) -> (frame, anchors entry, scales start row)."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    x, y, rw, rh = smh.map_bounds(Wd, Ht)
    frame, info = synth.make_frame(Wd, Ht, frame_idx=31 + Wd)
    qw, qh = rw // 2, rh // 2
    assert info["scales_start_y"] > 12 and qw >= 12
    frame[y + qh + 4:y + qh + 10, x + qw + 2:x + qw + 9, :3] = 210
    return frame, (info["scales_start_y"], info["anchors"]), info["scales_start_y"]


def _oracle_planes(frame, start_y):
    from oracle import oracle as o
    c = o.crop_to_map(frame, grayscale=False)
    assert c is not None
    iso = o.isolate_map_markers(c["cropped_map"])
    return dict(ui=c["ui_map"], iso=iso, mask=o.mask_marker_lines(iso), ocr=o.ocr_preprocess(c["cropped_brq"]), scales=o.find_scales_preprocess(c["cropped_brq"], start_y))


def _run(vision, Wd, Ht, frames, anchor_list):
    import torch
    import squad_mortar_helper_amd as smh
    N = len(frames)
    d = torch.from_numpy(np.stack(frames)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, Wd, Ht, N)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL, grayscale=False, anchors=smh.make_anchors(anchor_list), stream=s)
    return fb, d, s


def _payloads(msgs):
    return {f: data[10:] for f, kind, _, data in msgs if kind == W.MAP}


@pytest.mark.parametrize("size", V.SIZES)
def test_every_view_at_the_shapes_that_can_break_it(vision, size):
    """Frames: the base, the base again, the base with one marker-coloured pixel in the quarter.  Per view and split of the rows:
    every open frame's entry CRC is zlib's of the view, every Map payload is the view, header, entries and layout are the
    restatement's; a plane's CRC in both of its forms; once per view the payload is what the layers call renders from that source
    at the identity viewport of the view's size."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    L = smh._lib
    lib = L.load()
    Wd, Ht = size
    x, y, rw, rh = smh.map_bounds(Wd, Ht)
    k = V.SIZES.index(size)
    assert ((x + rw // 2) % 4, rw // 2) == (V.Q_XOFF[k], V.BRQ_W[k])            # the coverage this size was chosen for
    if k == 0:
        V.check_coverage(smh.map_bounds)
    base, anchors, start_y = _frame_for(Wd, Ht)
    # what keeps the comparison honest, on the oracle's images of the base frame
    op = _oracle_planes(base, start_y)
    assert (op["mask"] == 255).sum() >= 100 and op["iso"].any(axis=2).sum() >= 100 and (op["ocr"] != 255).sum() >= 20, size
    below = op["scales"][start_y:]
    assert (below == 0).any() and (below == 255).any(), size
    third = base.copy()
    third[y + rh // 2 + rh // 4, x + rw // 2 + rw // 4, :3] = np.array(synth.TEAM_RGB[0], np.uint8)[::-1]
    fb, d, s = _run(vision, Wd, Ht, [base, base.copy(), third], [anchors] * 3)
    N = 3
    feed = smh.WebFeed(vision, _full(N, rw, rh), N)
    try:
        planes = [_planes(fb, f) for f in range(N)]
        # the batch holds what the oracle computes (the scales image from its start row on)
        assert np.array_equal(planes[0]["ui"], op["ui"]) and np.array_equal(planes[0]["mask"], op["mask"]) and np.array_equal(planes[0]["ocr"], op["ocr"])
        assert np.array_equal(planes[0]["scales"][start_y:], below)
        for which in V.VIEWS:
            ref = _ref_frames(fb, 0, N, which, planes)
            want = W.feed(ref)
            vw, vh = V.view_size(which, rw, rh)
            assert all(r[2][:2] == (vw, vh) for r in ref)
            gray = which in (V.VIEW_OCR_INPUT, V.VIEW_FIND_SCALES_INPUT, V.VIEW_LSD_INPUT)
            for form in ((0, 4) if gray else (0,)):
                L.check(lib.smhv_debug_feed_gray_form(form))
                for rows in V.FEED_ROWS:
                    L.check(lib.smhv_debug_feed_rows(rows))
                    feed.reset()
                    fb.feed(feed, stream=s, map_source=which)
                    h, msgs = _same(feed, want, (size, which, form, rows))
                    crcs = {e.frame: e.crc for e in feed.entries}
                    assert crcs == {f: zlib.crc32(ref[f][2][2]) for f in range(N)}, (size, which, form, rows)
                    pay = _payloads(msgs)
                    assert 0 in pay and 1 not in pay and all(pay[f] == ref[f][2][2] for f in pay), (size, which, form, rows, sorted(pay))
            # the header's second identity: the layers call with this source, the identity viewport at the view's size, nothing else
            ident = G.View(*RR.identity(vw, vh))
            fb.render(smh.MapViewport(ident.quad, ident.scale, ident.top_left), vw, vh, background=BG, stream=s, layers=smh.RenderLayers((), map_source=which))
            for f in range(N):
                assert fb.read_render(f).tobytes() == ref[f][2][2], (size, which, "render", f)
    finally:
        L.check(lib.smhv_debug_feed_rows(0))
        L.check(lib.smhv_debug_feed_gray_form(0))
        feed.close()
        fb.close()


def test_a_plane_wider_than_64_groups(vision):
    """2560 x 1440: the mask's rows hold 83 16-byte groups, so a lane has two per row and the general kernel hashes the plane."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    L = smh._lib
    Wd, Ht = 2560, 1440
    x, y, rw, rh = smh.map_bounds(Wd, Ht)
    assert (rw + x % 4 + 15) // 16 > 64
    frame, info = synth.make_frame(Wd, Ht, frame_idx=77)
    fb, d, s = _run(vision, Wd, Ht, [frame], [(info["scales_start_y"], info["anchors"])])
    feed = smh.WebFeed(vision, _full(1, rw, rh), 1)
    try:
        planes = [_planes(fb, 0)]
        assert (planes[0]["mask"] == 255).sum() >= 100
        for which in (V.VIEW_LSD_INPUT, V.VIEW_LSD_PREPROCESS):
            ref = _ref_frames(fb, 0, 1, which, planes)
            for rows in (0, 3):
                L.check(L.load().smhv_debug_feed_rows(rows))
                feed.reset()
                fb.feed(feed, stream=s, map_source=which)
                _, msgs = _same(feed, W.feed(ref), (which, rows))
                assert feed.entries[0].crc == zlib.crc32(ref[0][2][2]) and _payloads(msgs)[0] == ref[0][2][2]
    finally:
        L.check(L.load().smhv_debug_feed_rows(0))
        feed.close()
        fb.close()


def _spots(which, rw, rh, start_y):
    """The changed source pixels in ROI coordinates: the view's first and last pixel, a row's end, the next row's start, the middle
    (the scales image from its start row on)."""
    if which in (V.VIEW_LSD_PREPROCESS, V.VIEW_LSD_INPUT):
        return [(0, 0), (rh - 1, rw - 1), (0, rw - 1), (1, 0), (rh // 2, rw // 2)]
    qw, qh = rw // 2, rh // 2
    y0 = start_y if which == V.VIEW_FIND_SCALES_INPUT else 0
    return [(rh // 2 + py, rw // 2 + px) for py, px in ((y0, 0), (qh - 1, qw - 1), (y0, qw - 1), (y0 + 1, 0), ((y0 + qh) // 2, qw // 2))]


@pytest.mark.parametrize("which", V.VIEWS)
@pytest.mark.parametrize("size", [(451, 360), (1920, 1080)])
def test_one_changed_pixel(vision, size, which):
    """base, five copies with one changed source pixel each, the base again, and the base with a non-marker pixel outside the
    quarter recoloured to another non-marker colour: every copy changes the view and sends a Map; the last frame changes the
    ui_map and not the view, so it sends a Map under VIEW_NONE and none under the view."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    Wd, Ht = size
    x, y, rw, rh = smh.map_bounds(Wd, Ht)
    base, anchors, start_y = _frame_for(Wd, Ht)
    frames = [base]
    for (py, px) in _spots(which, rw, rh, start_y):
        f = base.copy()
        old = f[y + py, x + px, :3].copy()
        if which in (V.VIEW_LSD_PREPROCESS, V.VIEW_LSD_INPUT):
            f[y + py, x + px, :3] = np.array(synth.TEAM_RGB[0], np.uint8)[::-1]   # a marker pixel: kept by the isolation, set in the mask
        elif which == V.VIEW_OCR_INPUT:
            f[y + py, x + px, :3] = 230                                          # near white with equal channels: text
        elif which == V.VIEW_FIND_SCALES_INPUT:
            f[y + py, x + px, :3] = 0 if old.any() else 255                      # luma zero <-> non-zero
        else:
            f[y + py, x + px, :3] = 255 - old
        frames.append(f)
    frames.append(base.copy())
    special = base.copy()
    assert rw // 2 > 3 and rh // 2 > 3
    special[y + 2, x + 3, :3] = (70, 80, 90)                                     # terrain to terrain, in the top left quarter
    frames.append(special)
    N = len(frames)
    fb, d, s = _run(vision, Wd, Ht, frames, [anchors] * N)
    feed = smh.WebFeed(vision, _full(N, rw, rh), N)
    try:
        planes = [_planes(fb, f) for f in range(N)]
        ref = _ref_frames(fb, 0, N, which, planes)
        none = _ref_frames(fb, 0, N, V.VIEW_NONE, planes)
        views = [r[2][2] for r in ref]
        assert all(views[k] != views[0] for k in range(1, 6)) and len(set(views[:6])) == 6, (size, which)   # every copy changes the view
        assert views[6] == views[0] and views[7] == views[0] and none[7][2][2] != none[6][2][2], (size, which)
        want, want_none = W.feed(ref), W.feed(none)
        sent = lambda w: [f for f, kind, _, _ in w["messages"] if kind == W.MAP]
        assert sent(want) == [0, 1, 2, 3, 4, 5, 6] and sent(want_none) == list(range(N))
        fb.feed(feed, stream=s, map_source=which)
        _, msgs = _same(feed, want, (size, which))
        assert sorted(_payloads(msgs)) == [0, 1, 2, 3, 4, 5, 6]
        feed.reset()
        fb.feed(feed, stream=s)
        _, msgs = _same(feed, want_none, (size, "ui_map"))
        assert sorted(_payloads(msgs)) == list(range(N))
    finally:
        feed.close()
        fb.close()


@pytest.fixture(scope="module")
def scene(vision):
    """The sequence scene of tests/test_web_gpu.py: one 1080p batch in the order of SEQ, run once in colour with every stage."""
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    L = smh._lib
    src, src_anchors = _frames_with_minimaps(4, 2100)
    x, y, rw, rh = smh.map_bounds(1920, 1080)
    a2 = src[0].copy()
    a2[y + 5, x + 5, :3] = np.array(synth.TEAM_RGB[1], np.uint8)[::-1]            # A': one more marker pixel -- the mask changes too
    plain, pinfo = synth.make_frame(1920, 1080, frame_idx=2190, n_lines=0)
    plain_anchors = smh.make_anchors([(pinfo["scales_start_y"], pinfo["anchors"])])[0]
    pick = {"A": (src[0], src_anchors[0]), "B": (src[1], src_anchors[1]), "closed": (src[3], src_anchors[3]), "A'": (a2, src_anchors[0]), "plain": (plain, plain_anchors)}
    N = len(SEQ)
    frames = np.stack([pick[k][0] for k in SEQ])
    anchors = (L.Anchors * N)()
    for i, k in enumerate(SEQ):
        anchors[i] = pick[k][1]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    fb.run(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors, stream=s)
    planes = [_planes(fb, f) for f in range(N)]
    refs = {which: _ref_frames(fb, 0, N, which, planes) for which in (V.VIEW_NONE, V.VIEW_LSD_INPUT, V.VIEW_CROPPED_BRQ)}
    assert [f[0] for f in refs[V.VIEW_NONE]] == [k != "closed" for k in SEQ]
    sc = dict(fb=fb, N=N, refs=refs, s=s, d=d, rw=rw, rh=rh, anchors=anchors, stages=stages, full=_full(N, rw, rh))
    yield sc
    fb.close()


def test_rule_state_reset_snapshot_and_switching(vision, scene):
    import squad_mortar_helper_amd as smh
    fb, N, s = scene["fb"], scene["N"], scene["s"]
    lsd, none = scene["refs"][V.VIEW_LSD_INPUT], scene["refs"][V.VIEW_NONE]
    LSD = V.VIEW_LSD_INPUT
    whole = W.feed(lsd)
    sent = [f for f, k, _, _ in whole["messages"] if k == W.MAP]
    assert sent == [0, 4, 5, 6, 9, 10] and [f for f in range(N) if lsd[f][0] and f not in sent] == [1, 3, 7]   # six Maps sent, three suppressed
    feed = smh.WebFeed(vision, scene["full"], N)
    fb.feed(feed, stream=s, map_source=LSD)
    h, _ = _same(feed, whole, "sequence")
    assert h.n_maps == 6 and h.frames_done == N and h.last_crc == zlib.crc32(lsd[10][2][2])
    # sub-ranges chain through the stored CRC on the device
    feed.reset()
    stored, got = None, []
    for first, n in ((0, 3), (3, 4), (7, N - 7)):
        fb.feed(feed, first=first, n=n, stream=s, map_source=LSD)
        part = W.feed(lsd[first:first + n], stored=stored, first=first)
        _, msgs = _same(feed, part, ("part", first))
        stored = part["stored"]
        got += msgs
    assert got == whole["messages"] and stored == whole["stored"]
    # NONE -> LSD_INPUT -> LSD_INPUT -> NONE on frames 0, 1 (A A): one stored CRC whatever the source
    feed.reset()
    stored, maps = None, []
    for which, ref in ((V.VIEW_NONE, none), (LSD, lsd), (LSD, lsd), (V.VIEW_NONE, none)):
        fb.feed(feed, first=0, n=2, stream=s, map_source=which)
        part = W.feed(ref[:2], stored=stored)
        h, _ = _same(feed, part, ("switch", which, len(maps)))
        stored = part["stored"]
        assert (h.has_last_crc, h.last_crc) == (1, stored)
        maps.append(part["n_maps"])
    assert maps == [1, 1, 0, 1]                                                   # the second LSD_INPUT call sends no Map for the unchanged frame
    # reset: the view is sent again; a snapshot with a view neither uses nor changes the stored CRC
    feed.reset()
    fb.feed(feed, first=0, n=2, stream=s, map_source=LSD)
    first_call = W.feed(lsd[:2])
    _same(feed, first_call, "after reset")
    for f, kinds in ((0, [W.MAP, W.UPDATE_STATE, W.MARKERS]), (10, [W.MAP, W.UPDATE_STATE])):
        snap = W.feed(lsd[f:f + 1], stored=first_call["stored"], snapshot=True, first=f)
        assert [k for _, k, _, _ in snap["messages"]] == kinds
        fb.feed(feed, first=f, n=1, snapshot=True, stream=s, map_source=LSD)
        _same(feed, snap, ("snapshot", f), stored_after=first_call["stored"])
    fb.feed(feed, snapshot=True, stream=s, map_source=LSD)
    _same(feed, W.feed(lsd, stored=first_call["stored"], snapshot=True), "snapshot of the batch", stored_after=first_call["stored"])
    fb.feed(feed, first=0, n=5, stream=s, map_source=LSD)
    _same(feed, W.feed(lsd[:5], stored=first_call["stored"]), "after the snapshots")
    feed.close()


def test_capacity_is_measured_with_the_source(vision, scene):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    fb, N, s, rw, rh = scene["fb"], scene["N"], scene["s"], scene["rw"], scene["rh"]
    brq, none = scene["refs"][V.VIEW_CROPPED_BRQ], scene["refs"][V.VIEW_NONE]
    BRQ = V.VIEW_CROPPED_BRQ
    cap = V.worst_case(BRQ, rw, rh)
    assert cap < V.worst_case(V.VIEW_NONE, rw, rh)
    feed = smh.WebFeed(vision, cap, N)
    fb.feed(feed, stream=s, map_source=BRQ)                                        # the quarter's worst case is enough for the quarter
    h, _ = _same(feed, W.feed(brq, capacity=cap), "the quarter's worst case")
    assert h.frames_done >= 1
    before = feed.read()
    with pytest.raises(smh.VisionError) as ei:                                    # ... and not for the ui_map, nor for a view of the map's size
        fb.feed(feed, stream=s)
    assert ei.value.code == L.E_INVALID
    with pytest.raises(smh.VisionError) as ei:
        fb.feed(feed, stream=s, map_source=V.VIEW_LSD_INPUT)
    assert ei.value.code == L.E_INVALID
    after = feed.read()
    assert bytes(after[0]) == bytes(before[0]) and after[1] == before[1]
    feed.close()
    small = smh.WebFeed(vision, cap - 1, N)
    with pytest.raises(smh.VisionError) as ei:
        fb.feed(small, first=0, n=1, stream=s, map_source=BRQ)
    assert ei.value.code == L.E_INVALID
    small.close()
    # the capacity cut and the continuation with a view
    first0, end0 = 4, 10                                                          # B A A' A' closed B: A' differs from A outside the quarter only
    uncapped = W.feed(brq[first0:end0], first=first0)
    assert uncapped["n_maps"] == 3 and W.feed(none[first0:end0], first=first0)["n_maps"] == 4
    two = [e for e in uncapped["entries"] if e[0] <= 5]
    cap = two[-1][4] + two[-1][2]
    feed = smh.WebFeed(vision, cap, N)
    first, stored, got, rounds = first0, None, [], 0
    while first < end0:
        fb.feed(feed, first=first, n=end0 - first, stream=s, map_source=BRQ)
        part = W.feed(brq[first:end0], stored=stored, capacity=cap, first=first)
        assert part["frames_done"] >= 1
        h, msgs = _same(feed, part, ("capped", first))
        assert h.bytes_used <= cap
        got += msgs
        first, stored, rounds = first + h.frames_done, part["stored"], rounds + 1
    assert got == uncapped["messages"] and stored == uncapped["stored"] and rounds >= 2
    feed.close()
    feed = smh.WebFeed(vision, cap - 1, N)                                        # one byte short of two Maps
    fb.feed(feed, first=first0, n=end0 - first0, stream=s, map_source=BRQ)
    h, _ = _same(feed, W.feed(brq[first0:end0], capacity=cap - 1, first=first0), "one byte short")
    assert h.frames_done == 1 and h.n_maps == 1
    feed.close()


def test_state_and_argument_errors_change_nothing(vision, scene):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    N, s, d, rw, rh = scene["N"], scene["s"], scene["d"], scene["rw"], scene["rh"]
    feed = smh.WebFeed(vision, scene["full"], N)
    scene["fb"].feed(feed, first=0, n=3, stream=s, map_source=V.VIEW_LSD_INPUT)
    content = feed.read()
    stored = (content[0].has_last_crc, content[0].last_crc)

    def unchanged(ctx):
        again = feed.read()
        assert bytes(again[0]) == bytes(content[0]) and again[1] == content[1], ctx
        assert (again[0].has_last_crc, again[0].last_crc) == stored, ctx

    fb2 = smh.FrameBatch(vision, 1920, 1080, N)
    for which in (V.VIEW_NONE,) + V.VIEWS:                                        # no run at all: no ui_map
        assert lib.smhv_batch_feed_view(fb2._b, feed._f, 0, N, 0, which, s) == L.E_STATE, which
    fb2.run(d.data_ptr(), N, stages=smh.STAGE_UI_MAP | smh.STAGE_MINIMAP, grayscale=True, anchors=None, stream=s)
    for which in V.VIEWS:                                                         # a grayscale ui_map, and no OCR / SCALES / MARKERS stage
        assert lib.smhv_batch_feed_view(fb2._b, feed._f, 0, N, 0, which, s) == L.E_STATE, which
    unchanged("after the state errors")
    fb2.run(d.data_ptr(), N, stages=smh.STAGE_ALL, grayscale=False, anchors=None, stream=s)
    assert lib.smhv_batch_feed_view(fb2._b, feed._f, 0, N, 0, V.VIEW_FIND_SCALES_INPUT, s) == L.E_STATE   # the SCALES stage without anchors
    for which in (6, 100, 0xFFFFFFFF):                                            # an unknown source
        assert lib.smhv_batch_feed_view(fb2._b, feed._f, 0, N, 0, which, s) == L.E_INVALID, which
        assert lib.smhv_batch_feed_view(scene["fb"]._b, feed._f, 0, N, 0, which, s) == L.E_INVALID, which
    for args in ((0, 0, 0), (1, N, 0), (N, 1, 0), (0, N, 2)):
        assert lib.smhv_batch_feed_view(scene["fb"]._b, feed._f, args[0], args[1], args[2], V.VIEW_LSD_INPUT, s) == L.E_INVALID, args
    unchanged("after the argument errors")
    # ... and the colour run made the other four available: a correct call follows
    planes = [_planes(fb2, f) for f in range(3)]
    fb2.feed(feed, first=0, n=3, stream=s, map_source=V.VIEW_LSD_PREPROCESS)
    _same(feed, W.feed(_ref_frames(fb2, 0, 3, V.VIEW_LSD_PREPROCESS, planes), stored=content[0].last_crc), "after the failed calls")
    fb2.close()
    feed.close()


def test_view_none_is_smhv_batch_feed(vision, scene):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    fb, N, s = scene["fb"], scene["N"], scene["s"]
    a, b = smh.WebFeed(vision, scene["full"], N), smh.WebFeed(vision, scene["full"], N)
    for flags in (0, L.FEED_SNAPSHOT):
        L.check(lib.smhv_batch_feed(fb._b, a._f, 0, N, flags, s))
        L.check(lib.smhv_batch_feed_view(fb._b, b._f, 0, N, flags, L.VIEW_NONE, s))
        ha, ma = a.read()
        ea = [(e.offset, e.length, e.frame, e.kind, e.crc) for e in a.entries]
        hb, mb = b.read()
        eb = [(e.offset, e.length, e.frame, e.kind, e.crc) for e in b.entries]
        assert bytes(ha) == bytes(hb) and ea == eb and ma == mb and ha.n_maps >= 6, flags
        assert ma == W.feed(scene["refs"][V.VIEW_NONE], snapshot=bool(flags))["messages"]
    a.close()
    b.close()


def test_a_view_from_the_slots_of_both_pipeline_schedules(vision, scene):
    import squad_mortar_helper_amd as smh
    N, d, anchors = scene["N"], scene["d"], scene["anchors"]
    want = W.feed(scene["refs"][V.VIEW_LSD_INPUT])["messages"]
    want_brq = W.feed(scene["refs"][V.VIEW_CROPPED_BRQ])["messages"]
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=4, search=search)
        feed = smh.WebFeed(vision, scene["full"], N)
        slots = [p.submit(d.data_ptr(), N, stages=scene["stages"], grayscale=False, anchors=anchors) for _ in range(2)]
        p.wait()
        for k, sl in enumerate(slots):
            for which, w in ((V.VIEW_LSD_INPUT, want), (V.VIEW_CROPPED_BRQ, want_brq)):
                feed.reset()
                p.slots[sl].feed(feed, stream=p.stream_of(sl), map_source=which)
                h, msgs = feed.read()
                assert msgs == w and h.frames_done == N, (search, k, which)
        feed.close()
        p.close()


def test_per_call_path_against_get_debug_view(vision):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    stems = ("full_1024x768_png", "full_1280x1024_png", "point_intersect_png")
    cap = max(W.worst_case(MANIFEST[st]["map_rect"][2], MANIFEST[st]["map_rect"][3]) for st in stems)
    feed = smh.WebFeed(vision, cap, 1)
    stored, sizes = None, set()
    for k, stem in enumerate(stems):
        frame, e, _ = load_fixture(stem)
        vision.load_frame(frame)
        r = vision.crop_to_map(grayscale=bool(k % 2))
        assert r is not None, stem
        rect = vision.find_minimap()
        vision.isolate_map_markers()
        vision.mask_marker_lines()
        lines = vision.find_marker_lines(15)
        vision.ocr_preprocess()
        mpx = None if k == 0 else 0.5 + k
        for which in V.VIEWS:
            img = vision.get_debug_view(which)
            h, w = img.shape[:2]
            sizes.add((w * h) % 1024)
            fr = [(True, 0, (w, h, img.tobytes()), lines, mpx is not None, mpx or 0.0, rect is not None, rect or (0, 0, 0, 0))]
            want = W.feed(fr, stored=stored)
            vision.feed_frame(feed, lines, mpx=mpx, minimap=rect, map_source=which)
            _, msgs = _same(feed, want, (stem, which))
            if want["n_maps"]:
                (f, kind, crc, data), = [m for m in msgs if m[1] == W.MAP]
                assert data[10:] == img.tobytes() and crc == zlib.crc32(img.tobytes()), (stem, which)
            stored = want["stored"]
            if which == V.VIEW_LSD_INPUT:                                         # the same view again: no Map; as a snapshot: the Map first
                vision.feed_frame(feed, lines, mpx=mpx, minimap=rect, map_source=which)
                again = W.feed(fr, stored=stored)
                assert again["n_maps"] == 0
                _same(feed, again, (stem, which, "again"))
                vision.feed_frame(feed, lines, mpx=mpx, minimap=rect, map_source=which, snapshot=True)
                _same(feed, W.feed(fr, stored=stored, snapshot=True), (stem, which, "snapshot"), stored_after=stored)
            assert np.array_equal(vision.get_debug_view(which), img), (stem, which)   # the call leaves the trait path's state alone
        ui = vision.ui_map(copy=True)                                             # ... and the ui_map follows on the same feed
        fr = [(True, 0, (ui.shape[1], ui.shape[0], ui.tobytes()), lines, mpx is not None, mpx or 0.0, rect is not None, rect or (0, 0, 0, 0))]
        want = W.feed(fr, stored=stored)
        vision.feed_frame(feed, lines, mpx=mpx, minimap=rect)
        _same(feed, want, (stem, "ui_map"))
        stored = want["stored"]
    assert len(sizes) >= 4 and 0 not in sizes                                     # images that end inside a row of the CRC's description
    before = feed.read()
    with pytest.raises(smh.VisionError) as ei:
        vision.feed_frame(feed, lines, map_source=6)
    assert ei.value.code == L.E_INVALID
    small = smh.WebFeed(vision, V.worst_case(V.VIEW_CROPPED_BRQ, w * 2, h * 2), 1)
    vision.feed_frame(small, lines, map_source=V.VIEW_CROPPED_BRQ)
    with pytest.raises(smh.VisionError) as ei:
        vision.feed_frame(small, lines, map_source=V.VIEW_LSD_INPUT)
    assert ei.value.code == L.E_INVALID
    small.close()
    after = feed.read()
    assert bytes(after[0]) == bytes(before[0]) and after[1] == before[1]
    feed.close()


def _state(fb, N):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    w, h = fb.render_size()
    return (bytes(fb.read_results(0, N)),
            [bytes(fb.read_image(k, f).tobytes()) for f in range(N) for k in (L.IMAGE_UI_MAP, L.VIEW_LSD_INPUT, L.VIEW_OCR_INPUT, L.VIEW_FIND_SCALES_INPUT)],
            [bytes(fb.read_render(f).tobytes()) for f in range(N)] if w and h else [])


def test_nothing_else_moves(vision, scene):
    import squad_mortar_helper_amd as smh
    fb, N, s, rw, rh = scene["fb"], scene["N"], scene["s"], scene["rw"], scene["rh"]
    ident = G.View(*RR.identity(rw // 4, rh // 4))
    fb.render(smh.MapViewport(ident.quad, ident.scale, ident.top_left), rw // 4, rh // 4, background=BG, stream=s)
    before = _state(fb, N)
    assert len(before[2]) == N
    feed = smh.WebFeed(vision, scene["full"], N)
    for which in V.VIEWS:
        fb.feed(feed, stream=s, map_source=which)
        fb.feed(feed, first=2, n=5, snapshot=True, stream=s, map_source=which)
    feed.read()
    assert _state(fb, N) == before
    feed.close()
