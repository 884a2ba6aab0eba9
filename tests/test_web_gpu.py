"""The remote-viewer feed on the device, byte for byte against the restatement (tests/web_ref.py: struct.pack and zlib.crc32), no
tolerance and no excluded cases: the CRC over the pitched ui slab at three frame sizes, the "changed since the last texture" rule,
its state across calls, the capacity cut, the slots of both pipeline schedules, the per-call path on the golden fixtures, and
that feeding moves nothing else."""
import zlib

import numpy as np
import pytest

import web_ref as W
from fixtures import MANIFEST, OPEN_STEMS, load_fixture
from test_firing_gpu import _frames_with_minimaps

pytestmark = pytest.mark.gpu

SEQ = "A A closed A B A A' A' closed B plain".split()


def _ref_frames(fb, first, n):
    """The restatement's input for frames [first, first + n): the records and ui_maps as the batch holds them."""
    import squad_mortar_helper_amd as smh
    _, _, rw, rh = fb.roi
    out = []
    for i, r in enumerate(fb.read_results(first, n)):
        ui = (rw, rh, fb.read_image(smh._lib.IMAGE_UI_MAP, first + i).tobytes()) if r.map_open else None
        lines = np.array([[l.x0, l.y0, l.x1, l.y1] for l in r.lines[:r.n_lines]], np.float32).reshape(-1, 4)
        out.append((bool(r.map_open), int(r.status), ui, lines, bool(r.has_mpx), float(r.mpx), bool(r.has_minimap), tuple(r.minimap)))
    return out


def _same(feed, want, ctx, stored_after=None):
    """The feed's last call == the restatement's result: header, entries (frame, kind, length, crc, offset), messages, layout."""
    h, msgs = feed.read()
    assert (h.n_entries, h.frames_done, h.n_maps, h.bytes_used) == (len(want["entries"]), want["frames_done"], want["n_maps"], want["bytes_used"]), ctx
    stored = want["stored"] if stored_after is None else stored_after
    assert (h.has_last_crc, h.last_crc) == ((1, stored) if stored is not None else (0, 0)), ctx
    got = [(e.frame, e.kind, e.length, e.crc, e.offset) for e in feed.entries]
    assert got == want["entries"], (ctx, got[:6], want["entries"][:6])
    assert len(msgs) == len(want["messages"]), ctx
    for k, (g, w) in enumerate(zip(msgs, want["messages"])):
        if g != w:
            bad = [i for i in range(min(len(g[3]), len(w[3]))) if g[3][i] != w[3][i]][:4]
            raise AssertionError((ctx, "message", k, g[:3], w[:3], len(g[3]), len(w[3]), bad))
    # every message at an offset = 6 (mod 16), none overlapping, bytes_used the end of the last
    offs = [(e.offset, e.length) for e in feed.entries]
    assert all(o % 16 == 6 for o, _ in offs) and all(offs[i][0] + offs[i][1] <= offs[i + 1][0] for i in range(len(offs) - 1)), ctx
    assert not offs or (offs[0][0] == 6 and h.bytes_used == offs[-1][0] + offs[-1][1]), ctx
    return h, msgs


@pytest.fixture(scope="module")
def scene(vision):
    """One 1080p batch in the order of SEQ -- A and B have a minimap rectangle and marker lines (the rectangle covers their scale
    bars: no m/px), A' is A with one map pixel changed, `plain` a frame with scale labels and without marker lines -- run once with
    every stage whose output the last test watches, and its restatement inputs."""
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    L = smh._lib
    src, src_anchors = _frames_with_minimaps(4, 2100)                             # 0, 1: open, with a rectangle, a line and labels; 3: closed
    x, y, rw, rh = smh.map_bounds(1920, 1080)
    a2 = src[0].copy()
    a2[y + 5, x + 5, :3] = 200                                                    # outside the rectangle (its edges lie at 10 or more)
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
    hm = smh.Heightmap(vision, np.random.default_rng(3).integers(0, 65536, size=(96, 128), dtype=np.uint16), ((4, -3), (0, 0)), (1.0, 1.0, 20.0))
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    fresh = smh.WebFeed(vision, W.worst_case(rw, rh), N)
    with pytest.raises(smh.VisionError) as ei:                                    # no run of the batch has produced a ui_map
        fb.feed(fresh, stream=s)
    assert ei.value.code == L.E_STATE
    fresh.close()
    fb.set_firing(hm)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_HEIGHTMAP_OVERLAY, grayscale=False, anchors=anchors, stream=s)
    ref = _ref_frames(fb, 0, N)
    assert [f[0] for f in ref] == [k != "closed" for k in SEQ]
    assert len(ref[0][3]) >= 1 and ref[0][6] and not ref[0][4] and len(ref[10][3]) == 0 and ref[10][4]   # bounds without a ratio; a ratio without lines
    sc = dict(fb=fb, N=N, ref=ref, s=s, d=d, rw=rw, rh=rh, frames=frames, anchors=anchors, full=6 + N * (32 + W.slot(10 + rw * rh * 4) + W.slot(7 + 16 * 32)))
    yield sc
    fb.close()
    hm.close()


@pytest.mark.parametrize("size", [(1024, 768), (1280, 1024), (1920, 1080)])
def test_crc_of_the_pitched_ui_slab(vision, size):
    """Every open frame's entry carries zlib.crc32 of its ui_map, in grayscale and in colour, at every split of the rows over the
    waves; one changed pixel -- the first, the last, the ends and starts of rows, the middle -- sends a Map, a change outside the
    ROI and the button does not."""
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    L = smh._lib
    Wd, Ht = size
    x, y, rw, rh = smh.map_bounds(Wd, Ht)
    assert x % 4 != 0                                                             # the rows are only 4-byte aligned in the slab
    base, info = synth.make_frame(Wd, Ht, frame_idx=31 + Wd)
    spots = [(0, 0), (rh - 1, rw - 1), (0, rw - 1), (1, 0), (rh // 2, rw // 2), (rh - 2, rw - 1)]
    frames = [base, base.copy()]
    frames[1][0, 0, :3] = (1, 2, 3)                                               # outside the ROI and the button
    bx, by, _, _ = smh.button_bounds(Wd, Ht)
    assert x > 0 and y > 0 and bx > 0 and by > 0
    for (py, px) in spots:
        f = base.copy()
        f[y + py, x + px, :3] = 255 - f[y + py, x + px, :3]                       # terrain is 60 .. 140: the luma changes too
        frames.append(f)
    N = len(frames)
    d = torch.from_numpy(np.stack(frames)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, Wd, Ht, N)
    feed = smh.WebFeed(vision, 6 + N * (32 + W.slot(10 + rw * rh * 4) + W.slot(7 + 16 * 32)), N)
    try:
        for gray in (True, False):
            fb.run(d.data_ptr(), N, stages=smh.STAGE_MARKERS | smh.STAGE_UI_MAP, grayscale=gray, stream=s)
            uis = [fb.read_image(L.IMAGE_UI_MAP, f) for f in range(N)]
            assert np.array_equal(uis[1], uis[0])
            for k, (py, px) in enumerate(spots):
                diff = np.argwhere(np.any(uis[2 + k] != uis[0], axis=2))
                assert diff.tolist() == [[py, px]], (gray, k)                     # exactly one ui pixel differs, the named one
            want = W.feed(_ref_frames(fb, 0, N))
            for rows in (0, 1, 3, 8, 64):
                L.check(L.load().smhv_debug_feed_rows(rows))
                feed.reset()
                fb.feed(feed, stream=s)
                h, msgs = _same(feed, want, (size, gray, rows))
                crcs = {e.frame: e.crc for e in feed.entries}
                assert crcs == {f: zlib.crc32(uis[f].tobytes()) for f in range(N)}, (size, gray, rows)
                maps = [f for f, kind, _, _ in msgs if kind == W.MAP]
                assert maps == [0] + list(range(2, N)), (size, gray, rows, maps)  # frame 1 sends none, every one-pixel copy does
    finally:
        L.check(L.load().smhv_debug_feed_rows(0))
        feed.close()
        fb.close()


def test_sequence_rule(vision, scene):
    import squad_mortar_helper_amd as smh
    fb, N, ref, s = scene["fb"], scene["N"], scene["ref"], scene["s"]
    want = W.feed(ref)
    sent = [f for f, k, _, _ in want["messages"] if k == W.MAP]
    assert sent == [0, 4, 5, 6, 9, 10] and [f for f in range(N) if ref[f][0] and f not in sent] == [1, 3, 7]   # six Maps sent, three suppressed
    feed = smh.WebFeed(vision, scene["full"], N)
    fb.feed(feed, stream=s)
    h, msgs = _same(feed, want, "sequence")
    assert [(f, k) for f, k, _, _ in msgs][:5] == [(0, W.UPDATE_STATE), (0, W.MAP), (0, W.MARKERS), (1, W.UPDATE_STATE), (1, W.MARKERS)]
    assert h.n_maps == 6 and h.frames_done == N and h.last_crc == zlib.crc32(ref[10][2][2])
    hp, ep, bp = feed.ptrs()
    assert hp and ep and bp and bp % 16 == 0
    feed.close()


def test_state_across_calls_reset_and_snapshot(vision, scene):
    import squad_mortar_helper_amd as smh
    fb, N, ref, s = scene["fb"], scene["N"], scene["ref"], scene["s"]
    whole = W.feed(ref)
    feed = smh.WebFeed(vision, scene["full"], N)
    # three calls over sub-ranges == one call: the stored CRC carries over on the device
    stored, got = None, []
    for first, n in ((0, 3), (3, 4), (7, N - 7)):
        fb.feed(feed, first=first, n=n, stream=s)
        part = W.feed(ref[first:first + n], stored=stored, first=first)
        _, msgs = _same(feed, part, ("part", first))
        stored = part["stored"]
        got += msgs
    assert got == whole["messages"] and stored == whole["stored"]
    # chained without a read in between: the library orders a call behind the feed's previous one
    feed.reset()
    fb.feed(feed, first=0, n=4, stream=s)
    fb.feed(feed, first=4, n=3, stream=s)
    _same(feed, W.feed(ref[4:7], stored=W.feed(ref[:4])["stored"], first=4), "chained")
    # a second call on unchanged frames sends no Map; after reset it sends one
    feed.reset()
    fb.feed(feed, first=0, n=2, stream=s)
    first_call = W.feed(ref[:2])
    _same(feed, first_call, "A A")
    fb.feed(feed, first=0, n=2, stream=s)
    again = W.feed(ref[:2], stored=first_call["stored"])
    assert again["n_maps"] == 0 and first_call["n_maps"] == 1
    _same(feed, again, "A A again")
    feed.reset()
    assert feed.header().n_entries == len(again["entries"])                       # (the buffer keeps the last call's events)
    fb.feed(feed, first=0, n=2, stream=s)
    _same(feed, first_call, "A A after reset")
    # the snapshot of a frame with bounds and lines, and of one with a ratio and no lines: no Markers message for it
    for f, kinds in ((0, [W.MAP, W.UPDATE_STATE, W.MARKERS]), (10, [W.MAP, W.UPDATE_STATE])):   # no Markers message without lines
        snap = W.feed(ref[f:f + 1], stored=first_call["stored"], snapshot=True, first=f)
        assert [k for _, k, _, _ in snap["messages"]] == kinds
        fb.feed(feed, first=f, n=1, snapshot=True, stream=s)
        _same(feed, snap, ("snapshot", f), stored_after=first_call["stored"])
    snap = W.feed(ref, stored=first_call["stored"], snapshot=True)                # the whole batch: closed frames send nothing
    fb.feed(feed, snapshot=True, stream=s)
    _same(feed, snap, "snapshot of the batch", stored_after=first_call["stored"])
    # ... and the next normal call is what it would have been without them
    fb.feed(feed, first=0, n=5, stream=s)
    _same(feed, W.feed(ref[:5], stored=first_call["stored"]), "after the snapshots")
    feed.close()


def test_capacity_cut_and_continuation(vision, scene):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    fb, N, ref, s, rw, rh = scene["fb"], scene["N"], scene["ref"], scene["s"], scene["rw"], scene["rh"]
    first0, end0 = 4, 10                                                          # B A A' A' closed B: four Maps
    uncapped = W.feed(ref[first0:end0], first=first0)
    assert uncapped["n_maps"] == 4
    two = [e for e in uncapped["entries"] if e[0] <= 5]                           # frames 4 and 5 hold the first two
    cap = two[-1][4] + two[-1][2]                                                 # ... and the feed ends with frame 5's last message
    feed = smh.WebFeed(vision, cap, N)
    first, stored, got, rounds = first0, None, [], 0
    while first < end0:
        fb.feed(feed, first=first, n=end0 - first, stream=s)
        part = W.feed(ref[first:end0], stored=stored, capacity=cap, first=first)
        assert part["frames_done"] >= 1
        h, msgs = _same(feed, part, ("capped", first))
        assert h.bytes_used <= cap
        got += msgs
        first, stored, rounds = first + h.frames_done, part["stored"], rounds + 1
    assert got == uncapped["messages"] and stored == uncapped["stored"] and rounds >= 2
    assert W.feed(ref[first0:end0], capacity=cap, first=first0)["frames_done"] == 2
    feed.close()
    # one byte short of two Maps: the first call takes frame 4 alone
    feed = smh.WebFeed(vision, cap - 1, N)
    fb.feed(feed, first=first0, n=end0 - first0, stream=s)
    h, _ = _same(feed, W.feed(ref[first0:end0], capacity=cap - 1, first=first0), "one byte short")
    assert h.frames_done == 1 and h.n_maps == 1
    feed.close()
    # a capacity below one frame's worst case for this geometry is refused; the worst case itself is enough
    small = smh.WebFeed(vision, W.worst_case(rw, rh) - 1, N)
    with pytest.raises(smh.VisionError) as ei:
        fb.feed(small, first=0, n=1, stream=s)
    assert ei.value.code == L.E_INVALID
    small.close()
    exact = smh.WebFeed(vision, W.worst_case(rw, rh), N)
    fb.feed(exact, stream=s)
    h, _ = _same(exact, W.feed(ref, capacity=W.worst_case(rw, rh)), "the worst case")
    assert h.frames_done >= 1
    exact.close()


def test_feed_from_the_slots_of_both_pipeline_schedules(vision, scene):
    import squad_mortar_helper_amd as smh
    fb, N, ref, s, d, anchors = scene["fb"], scene["N"], scene["ref"], scene["s"], scene["d"], scene["anchors"]
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP
    plain = smh.WebFeed(vision, scene["full"], N)
    fb.feed(plain, stream=s)
    h1, first_msgs = plain.read()
    fb.feed(plain, stream=s)
    h2, later_msgs = plain.read()
    assert h1.n_maps == 6 and h2.n_maps == 6 and first_msgs == later_msgs == W.feed(ref)["messages"]   # (the sequence ends on `plain` and starts on A)
    plain.close()
    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=4, search=search)
        feed = smh.WebFeed(vision, scene["full"], N)
        slots = [p.submit(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors) for _ in range(3)]
        p.wait()
        for k, sl in enumerate(slots):                                            # in submission order, into one feed
            sb = p.slots[sl]
            sb.feed(feed, stream=p.stream_of(sl))
            h, msgs = feed.read()
            assert msgs == first_msgs and (h.n_entries, h.n_maps, h.frames_done, h.bytes_used) == (h1.n_entries, h1.n_maps, N, h1.bytes_used), (search, k)
        assert p.submit(d.data_ptr(), N, stages=stages, grayscale=False, anchors=anchors) == 3   # the pipeline goes on after its slots were fed
        p.wait()
        feed.close()
        p.close()


def test_per_call_path_on_the_golden_fixtures(vision):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    cap = max(W.worst_case(MANIFEST[st]["map_rect"][2], MANIFEST[st]["map_rect"][3]) for st in OPEN_STEMS)
    feed = smh.WebFeed(vision, cap, 1)
    stored, sizes, with_lines, maps = None, set(), 0, 0
    for k, stem in enumerate(OPEN_STEMS):
        frame, e, _ = load_fixture(stem)
        vision.load_frame(frame)
        r = vision.crop_to_map(grayscale=bool(k % 2))
        assert r is not None, stem
        ui = r[0]
        rect = vision.find_minimap()
        vision.isolate_map_markers()
        vision.mask_marker_lines()
        lines = vision.find_marker_lines(15)
        mpx = None if k % 3 == 0 else 0.25 + k
        h, w = ui.shape[:2]
        sizes.add((w, h))
        with_lines += len(lines) > 0
        want = W.feed([(True, 0, (w, h, ui.tobytes()), lines, mpx is not None, mpx or 0.0, rect is not None, rect or (0, 0, 0, 0))], stored=stored)
        vision.feed_frame(feed, lines, mpx=mpx, minimap=rect)
        _, msgs = _same(feed, want, stem)
        for f, kind, crc, data in msgs:
            if kind == W.MAP:
                assert data[10:] == ui.tobytes() and crc == zlib.crc32(ui.tobytes()), stem   # the payload is the ui_map the trait returned
                maps += 1
        stored = want["stored"]
        if k == 0:                                                                # the same frame again: no Map; as a snapshot: the Map first
            vision.feed_frame(feed, lines, mpx=mpx, minimap=rect)
            _same(feed, W.feed([(True, 0, (w, h, ui.tobytes()), lines, mpx is not None, mpx or 0.0, rect is not None, rect or (0, 0, 0, 0))], stored=stored), (stem, "again"))
            vision.feed_frame(feed, lines, mpx=mpx, minimap=rect, snapshot=True)
            _same(feed, W.feed([(True, 0, (w, h, ui.tobytes()), lines, mpx is not None, mpx or 0.0, rect is not None, rect or (0, 0, 0, 0))], stored=stored, snapshot=True),
                  (stem, "snapshot"), stored_after=stored)
        # the call changes nothing of what the trait path hands out
        assert vision.find_minimap() == rect and np.array_equal(vision.ui_map(copy=True), ui), stem
    assert maps >= len(OPEN_STEMS) - 2 and len(sizes) >= 4 and with_lines >= 10, (maps, sizes, with_lines)
    with pytest.raises(smh.VisionError) as ei:
        vision.feed_frame(feed, np.zeros((33, 4), np.float32))
    assert ei.value.code == L.E_INVALID
    # errors follow the trait path: a closed map is SMHV_E_STATE, and the feed keeps its last call's events
    before = feed.read()[1]
    frame, _, _ = load_fixture("a_point_png")
    vision.load_frame(frame)
    assert vision.crop_to_map() is None
    with pytest.raises(smh.VisionError) as ei:
        vision.feed_frame(feed, np.zeros((0, 4), np.float32))
    assert ei.value.code == L.E_STATE and feed.read()[1] == before
    feed.close()


def _state(fb, N):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    return (bytes(fb.read_results(0, N)),
            [bytes(fb.read_image(w, f).tobytes()) for f in range(N) for w in (L.IMAGE_UI_MAP, L.VIEW_LSD_INPUT, L.VIEW_OCR_INPUT, L.IMAGE_HEIGHTMAP_OVERLAY)])


def test_nothing_else_moves_and_validation(vision, scene):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    fb, N, ref, s = scene["fb"], scene["N"], scene["ref"], scene["s"]
    before = _state(fb, N)
    feed = smh.WebFeed(vision, scene["full"], N)
    fb.feed(feed, stream=s)
    fb.feed(feed, first=2, n=5, snapshot=True, stream=s)
    fb.feed(feed, first=0, n=3, stream=s)
    content = feed.read()
    assert _state(fb, N) == before
    lib = L.load()

    def call(f, first, n, flags):
        return lib.smhv_batch_feed(fb._b, f._f, first, n, flags, s)

    short = smh.WebFeed(vision, scene["full"], 4)
    for args in ((feed, 0, 0, 0), (feed, 1, N, 0), (feed, N, 1, 0), (feed, 0, N, 2), (feed, 0, N, 0x80000000), (short, 0, 5, 0)):
        assert call(*args) == L.E_INVALID, args[1:]
    assert lib.smhv_batch_feed(None, feed._f, 0, 1, 0, s) == L.E_INVALID and lib.smhv_batch_feed(fb._b, None, 0, 1, 0, s) == L.E_INVALID
    for bad in ((0, N), (1 << 30, 0), (1 << 30, 65536)):                          # no room for a message; no frames; more frames than a launch covers
        with pytest.raises(smh.VisionError) as ei:
            smh.WebFeed(vision, *bad)
        assert ei.value.code == L.E_INVALID
    # a failed call enqueues nothing: the previous call's events are still what the feed hands out, and a correct call follows
    again = feed.read()
    assert bytes(again[0]) == bytes(content[0]) and again[1] == content[1]
    assert call(short, 0, 4, 0) == 0
    _same(short, W.feed(ref[:4]), "after the failed calls")
    assert _state(fb, N) == before
    short.close()
    feed.close()
