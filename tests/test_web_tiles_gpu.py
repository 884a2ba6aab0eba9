"""The feed's map tiles on the device (smhv_batch_feed_tiles / smhv_feed_frame_tiles), byte for byte against the restatement
(tests/web_tiles_ref.py) fed with the ORACLE's ui_maps and the batch's records, no tolerance anywhere: every case of
tests/web_tiles_cases.py in colour and in grey -- header, entries, every message byte, and the stream replayed through the
library's client half to the oracle's ui_map of every open frame -- the per-call path, a pipeline slot on each search schedule,
the refused calls, and a plain smhv_batch_feed on a feed that has made tile calls."""
import ctypes as C
import zlib

import numpy as np
import pytest

import web_ref as W
import web_tiles_cases as TC
import web_tiles_ref as T
from test_web_gpu import _same

pytestmark = pytest.mark.gpu


def _stages():
    import squad_mortar_helper_amd as smh
    return smh.STAGE_MARKERS | smh.STAGE_UI_MAP | smh.STAGE_MINIMAP


def _h2d(addr, data):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    assert hip.hipMemcpy(C.c_void_p(addr), buf.ctypes.data, buf.size, 1) == 0                  # hipMemcpyHostToDevice


def _full(c, n):
    return 6 + n * (32 + W.slot(10 + c.rw * c.rh * 4) + W.slot(7 + 16 * W.MAX_LINES))


def _batch(vision, c, keys, gray, s):
    """A batch over the frames of `keys` (gathered on the device from the unique ones), run once -> (batch, the frames' tensor)."""
    import torch
    import squad_mortar_helper_amd as smh
    uniq = list(dict.fromkeys(keys))
    at = {k: i for i, k in enumerate(uniq)}
    d_uniq = torch.from_numpy(np.stack([TC.frame_of(c, k) for k in uniq])).cuda()
    big = d_uniq.index_select(0, torch.tensor([at[k] for k in keys], device="cuda"))
    fb = smh.FrameBatch(vision, c.W, c.H, len(keys))
    assert tuple(fb.roi)[2:] == (c.rw, c.rh)
    fb.run(big.data_ptr(), len(keys), stages=_stages(), grayscale=gray, stream=s)
    return fb, big


def _patch(fb, c, patches, b):
    """The case's patches of batch b, written into the ui slab and the records where they lie."""
    import torch
    import squad_mortar_helper_amd as smh
    mine = [p for p in patches if p[1] == b]
    if not mine:
        return
    lay = fb.layout
    ui = fb.device_ptrs()["ui"]                                 # (a grey batch makes the RGBA slab now)
    torch.cuda.synchronize()
    assert lay.ui_offset == 4 * c.m_xoff and lay.ui_pitch >= lay.ui_offset + 4 * c.rw
    for p in mine:
        frame = ui + p[2] * lay.ui_stride
        if p[0] == "alpha":
            _h2d(frame + p[3] * lay.ui_pitch + lay.ui_offset + 4 * p[4] + 3, bytes([p[5]]))
        elif p[0] == "leadin":
            for y in (0, c.rh // 2, c.rh - 1):
                if lay.ui_offset:
                    _h2d(frame + y * lay.ui_pitch, b"\xa5" * lay.ui_offset)
        elif p[0] == "pitchpad":
            for y in (0, c.rh // 2, c.rh - 1):
                pad = lay.ui_pitch - lay.ui_offset - 4 * c.rw
                if pad:
                    _h2d(frame + y * lay.ui_pitch + lay.ui_offset + 4 * c.rw, b"\x5a" * pad)
        elif p[0] == "status":
            rec = smh._lib.FrameResult
            _h2d(fb.device_ptrs()["results"] + p[2] * C.sizeof(rec) + rec.status.offset, (1).to_bytes(4, "little"))
        else:
            raise KeyError(p[0])
    torch.cuda.synchronize()


def _records(fb, n):
    return [(np.array([[l.x0, l.y0, l.x1, l.y1] for l in r.lines[:r.n_lines]], np.float32).reshape(-1, 4), bool(r.has_mpx), float(r.mpx), bool(r.has_minimap),
             tuple(r.minimap)) for r in fb.read_results(0, n, check=False)], [bool(r.map_open) for r in fb.read_results(0, n, check=False)]


def _replay(tex, msgs, want_ui):
    """The step's messages through MapTexture: after every open frame's messages the texture is the oracle's ui_map of that frame."""
    for f, kind, crc, data in msgs:
        if kind in (W.MAP, T.MAP_TILES):
            tex.apply(data)
        if kind == W.MARKERS:
            assert tex.map.tobytes() == want_ui(f) and tex.crc() == crc == zlib.crc32(want_ui(f)), f


def _run_case(vision, case, gray):
    import torch
    import squad_mortar_helper_amd as smh
    s = torch.cuda.current_stream().cuda_stream
    made = [_batch(vision, c, keys, gray, s) for c, keys in case.batches]
    feed = None
    try:
        records = []
        for b, (c, keys) in enumerate(case.batches):
            _patch(made[b][0], c, case.patches, b)
            recs, opened = _records(made[b][0], len(keys))
            assert opened == [TC.ui_of(c, k, gray) is not None for k in keys], (case.name, b)
            records.append(recs)
        fr = TC.ref_frames(case, gray, records)
        want = TC.run_reference(case, fr)
        case.check(want, fr)
        cap = case.capacity(fr) if case.capacity else max(_full(c, len(keys)) for c, keys in case.batches)
        feed = smh.WebFeed(vision, cap, max(len(keys) for _, keys in case.batches))
        tex = smh.MapTexture()
        for k, (st, r) in enumerate(zip(case.steps, want)):
            if st[0] == "reset":
                feed.reset()
                continue
            b = st[1]
            if st[0] == "frame":
                vision.load_frame(TC.frame_of(case.batches[b][0], case.batches[b][1][st[2]]))
                assert vision.crop_to_map(grayscale=gray) is not None
                vision.feed_frame_tiles(feed, np.zeros((0, 4), np.float32))
            elif st[0] == "tiles":
                made[b][0].feed_tiles(feed, first=st[2], n=st[3], stream=s)
            else:
                made[b][0].feed(feed, first=st[2], n=st[3], stream=s)
            h, msgs = _same(feed, r, (case.name, gray, k, st))
            assert h.bytes_used <= cap
            _replay(tex, msgs, lambda f: fr[b][st[2] if st[0] == "frame" else f][2][2])
    finally:
        if feed is not None:
            feed.close()
        for fb, _ in made:
            fb.close()


@pytest.mark.parametrize("gray", [False, True], ids=["colour", "grey"])
@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_every_case_through_the_batch_and_the_per_call_path(vision, name, gray):
    """Header, entries and every message byte == the restatement's; the replayed texture == the oracle's ui_map of every open frame.
    (The steps named "frame" go through smhv_feed_frame_tiles.)"""
    _run_case(vision, TC.BY_NAME[name], gray)


def test_per_call_path_alone(vision):
    """X, P1, P1, X one call each through smhv_feed_frame_tiles, with lines, a ratio and bounds in the messages."""
    import squad_mortar_helper_amd as smh
    c = TC.MAIN
    feed = smh.WebFeed(vision, W.worst_case(c.rw, c.rh), 1)
    tex, stored, kept, kinds = smh.MapTexture(), None, None, []
    lines = np.array([[1.5, 2.5, 30.0, 40.0], [0.0, 1.0, 2.0, 3.0]], np.float32)
    try:
        for k, key in enumerate(["X", TC.P1, TC.P1, "X"]):
            vision.load_frame(TC.frame_of(c, key))
            ui = vision.crop_to_map(grayscale=False)[0].tobytes()
            assert ui == TC.ui_of(c, key, False)
            frame = (True, 0, (c.rw, c.rh, ui), lines, True, 0.5 + k, True, (1, 2, 3, 4 + k))
            want = T.feed_tiles([frame], stored=stored, kept=kept)
            vision.feed_frame_tiles(feed, lines, mpx=0.5 + k, minimap=(1, 2, 3, 4 + k))
            _, msgs = _same(feed, want, key)
            _replay(tex, msgs, lambda f: ui)
            stored, kept = want["stored"], want["kept"]
            kinds.append([kind for _, kind, _, _ in msgs])
        U, K = W.UPDATE_STATE, W.MARKERS
        assert kinds == [[U, W.MAP, K], [U, T.MAP_TILES, K], [U, K], [U, T.MAP_TILES, K]]
    finally:
        feed.close()


@pytest.mark.parametrize("search", ["batch", "frame"])
def test_a_pipeline_slot_on_each_search_schedule(vision, search):
    import torch
    import squad_mortar_helper_amd as smh
    case, c = TC.BY_NAME["seq/X closed closed Y"], TC.MAIN
    keys = case.batches[0][1]
    d = torch.from_numpy(np.stack([TC.frame_of(c, k) for k in keys])).cuda()
    p = smh.Pipeline(vision, c.W, c.H, len(keys), depth=4, search=search)
    feed = smh.WebFeed(vision, _full(c, len(keys)), len(keys))
    try:
        sl = p.submit(d.data_ptr(), len(keys), stages=_stages(), grayscale=False)
        p.wait()
        sb = p.slots[sl]
        recs, opened = _records(sb, len(keys))
        fr = TC.ref_frames(case, False, [recs])
        (want,) = TC.run_reference(case, fr)
        case.check([want], fr)
        sb.feed_tiles(feed, stream=p.stream_of(sl))
        _, msgs = _same(feed, want, search)
        _replay(smh.MapTexture(), msgs, lambda f: fr[0][f][2][2])
        assert p.submit(d.data_ptr(), len(keys), stages=_stages(), grayscale=False) is not None   # the pipeline goes on after its slot was fed
        p.wait()
    finally:
        feed.close()
        p.close()


def test_refused_calls_leave_the_feed_as_it_was(vision):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib, c = L.load(), TC.MAIN
    s = torch.cuda.current_stream().cuda_stream
    keys = ["X", TC.P1, TC.P2]
    N = len(keys)
    fb, big = _batch(vision, c, keys, False, s)
    feed = smh.WebFeed(vision, _full(c, N), N)
    short = smh.WebFeed(vision, _full(c, N), 2)
    small = smh.WebFeed(vision, W.worst_case(c.rw, c.rh) - 1, N)
    empty = smh.FrameBatch(vision, c.W, c.H, N)
    try:
        recs, _ = _records(fb, N)
        fr = [(True, 0, (c.rw, c.rh, TC.ui_of(c, k, False))) + tuple(r) for k, r in zip(keys, recs)]
        fb.feed_tiles(feed, first=0, n=2, stream=s)
        first = T.feed_tiles(fr[:2])
        content = _same(feed, first, "before")

        def call(f, b, first_, n, flags):
            return lib.smhv_batch_feed_tiles(b._b if b else None, f._f if f else None, first_, n, flags, s)
        for args in ((feed, fb, 0, 2, L.FEED_SNAPSHOT), (feed, fb, 0, 2, 2), (feed, fb, 0, 2, 0x80000000), (feed, fb, 0, 2, 3), (feed, fb, 0, 0, 0), (feed, fb, 1, N, 0),
                     (feed, fb, N, 1, 0), (short, fb, 0, 3, 0), (small, fb, 0, 1, 0), (None, fb, 0, 1, 0), (feed, None, 0, 1, 0)):
            assert call(*args) == L.E_INVALID, args[2:]
        assert call(feed, empty, 0, 1, 0) == L.E_STATE          # no run of that batch has produced a ui_map
        vision.load_frame(TC.frame_of(c, "X"))
        assert vision.crop_to_map(grayscale=False) is not None
        for bad in (L.FEED_SNAPSHOT, 2):
            assert lib.smhv_feed_frame_tiles(vision._ctx, feed._f, None, 0, None, None, bad) == L.E_INVALID
        again = feed.read()
        assert bytes(again[0]) == bytes(content[0]) and again[1] == content[1]
        # ... and the feed goes on from where it was: the kept map is P1's
        fb.feed_tiles(feed, first=2, n=1, stream=s)
        nxt = T.feed_tiles(fr[2:], stored=first["stored"], kept=first["kept"], first=2)
        assert [k for _, k, _, _ in nxt["messages"]] == [W.UPDATE_STATE, T.MAP_TILES, W.MARKERS]
        _same(feed, nxt, "after the refused calls")
        assert call(short, fb, 0, 2, 0) == 0                    # a feed none of whose calls succeeded yet is usable too
        _same(short, first, "short")
    finally:
        for f in (feed, short, small):
            f.close()
        fb.close()
        empty.close()


def test_a_plain_feed_after_tile_calls_is_a_plain_feed(vision):
    """smhv_batch_feed on a feed that has made tile calls == smhv_batch_feed on a fresh feed with the same stored CRC."""
    import torch
    import squad_mortar_helper_amd as smh
    c = TC.MAIN
    s = torch.cuda.current_stream().cuda_stream
    keys = ["X", TC.P1, "closed", TC.P2, TC.P2]
    fb, big = _batch(vision, c, keys, True, s)
    used, fresh = smh.WebFeed(vision, _full(c, len(keys)), len(keys)), smh.WebFeed(vision, _full(c, len(keys)), len(keys))
    try:
        fb.feed_tiles(used, first=0, n=2, stream=s)
        fb.feed(fresh, first=0, n=2, stream=s)
        hu, hf = used.header(), fresh.header()
        assert (hu.has_last_crc, hu.last_crc) == (hf.has_last_crc, hf.last_crc) == (1, zlib.crc32(TC.ui_of(c, TC.P1, True)))
        for f in (used, fresh):
            fb.feed(f, stream=s)
        (h1, m1), (h2, m2) = used.read(), fresh.read()
        assert bytes(h1) == bytes(h2) and m1 == m2 and [(e.offset, e.length, e.kind) for e in used.entries] == [(e.offset, e.length, e.kind) for e in fresh.entries]
        assert h1.n_maps == 3 and all(k != T.MAP_TILES for _, k, _, _ in m1)
    finally:
        used.close()
        fresh.close()
        fb.close()
