"""The remote-viewer feed on the device where its plain path had not been, byte for byte against tests/web_ref.py (struct.pack and
zlib.crc32) fed with the ORACLE's records and ui_maps, no tolerance and no excluded case (tests/web_long_cases.py):

the long calls -- batches of 2 x 1024 + 64 frames gathered on the device from four unique frames, in colour and in grey: every
named sequence and every capacity cut through k_feed_plan's chunk loop (the stored CRC, the layout and frames_done carried from
chunk to chunk), 2112 Maps through three passes of k_feed_maps' grid;

the sweep -- k_map_crc and k_feed_maps at the geometry sweep's rows for every m_xoff, m_quads on both sides of the lanes' group
counts, every rw % 4 and (rw * rh) % 4, at every split of the rows over the waves; and single flipped pixels at the ends of the
first and the last live lane's groups."""
import zlib

import numpy as np
import pytest

import geometry_sweep_cases as G
import web_long_cases as L
import web_ref as W
from test_web_gpu import _same

pytestmark = pytest.mark.gpu
B, N = L.B, L.N_LONG


def _full(rw, rh, n):
    """Room for n frames that all send their three messages."""
    return 6 + n * (32 + W.slot(10 + rw * rh * 4) + W.slot(7 + 16 * W.MAX_LINES))


def _records_equal_oracle(fb, refs, which, n, minimap, ctx):
    """The batch's records are the oracle's: a mismatch in the feed below is then the feed's."""
    import squad_mortar_helper_amd as smh
    recs = smh.results_to_dicts(fb.read_results(0, n))
    for i in range(n):
        r, ref = recs[i], refs[which[i]]
        assert r["status"] == 0 and r["map_open"] == ref["map_open"], (ctx, i)
        if not ref["map_open"]:
            assert (r["n_lines"], r["mpx"], r["minimap"]) == (0, None, None), (ctx, i)
            continue
        assert r["n_lines"] == ref["n_lines"] and np.array_equal(r["lines"], ref["lines"]), (ctx, i, r["n_lines"], ref["n_lines"])
        assert r["mpx"] == ref["mpx"] and r["minimap"] == (ref["minimap"] if minimap else None), (ctx, i, r["mpx"], ref["mpx"], r["minimap"], ref["minimap"])


@pytest.fixture(scope="module", params=[False, True], ids=["colour", "grey"])
def world(request, vision):
    """The four unique frames on the device, one FrameBatch of N frames and one feed with room for everything; run(master) gathers
    the master's frames on the device and runs the batch over them once -- again only when another master is asked for."""
    import torch
    import squad_mortar_helper_amd as smh
    gray, c = request.param, L.LONG_CASE
    frames, per, refs = L.unique_oracle()
    L.check_unique(refs)
    uniq = [L.ref_frame(r, gray, c.rw, c.rh) for r in refs]
    d_uniq = torch.from_numpy(frames).cuda()
    big = torch.empty((N, c.H, c.W, 4), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, c.W, c.H, N)
    assert tuple(fb.roi)[2:] == (c.rw, c.rh)
    feed = smh.WebFeed(vision, _full(c.rw, c.rh, N), N)
    w = dict(gray=gray, c=c, refs=refs, uniq=uniq, fb=fb, feed=feed, s=s, current=None, runs=0)

    def run(master):
        if w["current"] != master:
            idx = L.MASTERS[master]
            torch.index_select(d_uniq, 0, torch.from_numpy(idx).cuda(), out=big)
            fb.run(big.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=gray, max_gap=L.MAX_GAP, anchors=smh.make_anchors([per[i] for i in idx]), stream=s)
            _records_equal_oracle(fb, refs, idx, N, True, (master, gray))
            w["current"], w["runs"] = master, w["runs"] + 1
        return L.master_ref(master, uniq)
    w["run"] = run
    yield w
    assert w["runs"] <= len(L.MASTERS)
    feed.close()
    fb.close()
    del big, d_uniq
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", L.SEQ_NAMES)
def test_named_sequence(vision, world, name):
    """Every call of the sequence == web_ref.feed of the oracle's frames: header, entries, every message, the layout."""
    import squad_mortar_helper_amd as smh
    seq, fb, s, c = L.SEQUENCES[name], world["fb"], world["s"], world["c"]
    fr = world["run"](seq.master)
    want = L.run_reference(seq, fr)
    seq.check(want, fr)
    for k, part in enumerate(seq.parts):
        feed = world["feed"] if part.capacity is None else smh.WebFeed(vision, part.capacity(fr), N)
        try:
            feed.reset()
            for j, (first, n, snapshot) in enumerate(part.calls):
                fb.feed(feed, first=first, n=n, snapshot=snapshot, stream=s)
                h, msgs = _same(feed, want[k][j], (name, k, j))
                assert h.bytes_used <= feed.capacity_bytes
                if name == "all_maps":                                                    # every payload is the oracle's ui_map of its unique frame
                    assert h.n_maps == N and L.copy_passes(h.n_maps, c.rw, c.rh) >= 3
                    payload = [u[2][2] for u in world["uniq"][:3]]
                    crcs = [zlib.crc32(p) for p in payload]
                    got = [(f, data[10:]) for f, kind, _, data in msgs if kind == W.MAP]
                    assert [f for f, _ in got] == list(range(N))
                    bad = [f for f, data in got if data != payload[L.MASTERS["all"][f]]]
                    assert not bad, bad[:8]
                    assert all(e.crc == crcs[L.MASTERS["all"][e.frame]] for e in feed.entries)
        finally:
            if feed is not world["feed"]:
                feed.close()


@pytest.mark.parametrize("cut", L.CUTS, ids=L.CUT_NAMES)
def test_capacity_cut_and_continuation(vision, world, cut):
    """The whole `mixed` master into a feed whose capacity ends where the cut says, fed again from first + frames_done until the end:
    every round == the reference's, the concatenated messages == the uncut reference's, in as many rounds."""
    import squad_mortar_helper_amd as smh
    fb, s = world["fb"], world["s"]
    fr = world["run"]("mixed")
    cap = L.cut_capacity(cut, fr)
    assert L.check_cut(cut, fr)["frames_done"] == cut.frames_done
    parts, want_msgs, want_stored = L.rounds_of(fr, cap)
    uncut = W.feed(fr)
    assert want_msgs == uncut["messages"] and want_stored == uncut["stored"]
    feed = smh.WebFeed(vision, cap, N)
    try:
        first, got, rounds = 0, [], 0
        while first < N:
            assert rounds < len(parts), (cut.name, rounds)
            fb.feed(feed, first=first, n=N - first, stream=s)
            h, msgs = _same(feed, parts[rounds], (cut.name, rounds, first))
            assert h.bytes_used <= cap and h.frames_done >= 1
            if rounds == 0:
                assert h.frames_done == cut.frames_done
            got += msgs
            first, rounds = first + h.frames_done, rounds + 1
        assert rounds == len(parts) and got == uncut["messages"]
        assert (feed.header().has_last_crc, feed.header().last_crc) == (1, uncut["stored"])
    finally:
        feed.close()


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------

def _feed_at_every_split(fb, feed, s, want, uis, ctx):
    """The batch into the feed at every smhv_debug_feed_rows: == want; every Map's payload is the oracle's ui_map, its entries carry
    zlib.crc32 of it, and the Markers message behind every Map is whole."""
    import squad_mortar_helper_amd as smh
    lib = smh._lib
    crcs = {f: zlib.crc32(u) for f, u in uis.items()}
    try:
        for rows in L.ROWS_PER_WAVE:
            lib.check(lib.load().smhv_debug_feed_rows(rows))
            feed.reset()
            fb.feed(feed, stream=s)
            h, msgs = _same(feed, want, (ctx, rows))
            assert {e.frame: e.crc for e in feed.entries} == crcs, (ctx, rows)
            for k, (f, kind, crc, data) in enumerate(msgs):
                if kind != W.MAP:
                    continue
                assert data[10:] == uis[f] and crc == crcs[f], (ctx, rows, f)
                nf, nkind, _, ndata = msgs[k + 1]
                assert (nf, nkind) == (f, W.MARKERS) and ndata == want["messages"][k + 1][3] and len(ndata) == feed.entries[k + 1].length, (ctx, rows, f)
    finally:
        lib.check(lib.load().smhv_debug_feed_rows(0))


@pytest.mark.parametrize("c", L.FEED_SWEEP, ids=L.FEED_SWEEP_IDS)
def test_crc_and_copy_at_the_sweep_layouts(vision, c):
    """An open, a closed and an open frame of the geometry sweep's scene; grey with the minimap walk (UpdateState with bounds), colour
    without (the short UpdateState)."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, infos, refs = G.oracle_of(c)
    n = len(frames)
    assert [r["map_open"] for r in refs] == [1, 0, 1]
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos])
    fb = smh.FrameBatch(vision, c.W, c.H, n)
    feed = smh.WebFeed(vision, _full(c.rw, c.rh, n), n)
    try:
        for gray, minimap in ((True, True), (False, False)):
            fb.run(d.data_ptr(), n, stages=smh.STAGE_ALL | (smh.STAGE_MINIMAP if minimap else 0), grayscale=gray, max_gap=G.MAX_GAP, anchors=anchors, stream=s)
            _records_equal_oracle(fb, refs, range(n), n, minimap, (c, gray))
            fr = [L.ref_frame(r, gray, c.rw, c.rh, minimap) for r in refs]
            want = W.feed(fr)
            assert want["n_maps"] == 2 and want["frames_done"] == n and {len(m[3]) for m in want["messages"] if m[1] == W.UPDATE_STATE} == {27 if minimap else 11}
            _feed_at_every_split(fb, feed, s, want, {f: fr[f][2][2] for f in range(n) if fr[f][0]}, (c.W, c.H, gray))
    finally:
        feed.close()
        fb.close()
        del d


@pytest.mark.parametrize("c", L.FLIP_CASES, ids=L.FLIP_IDS)
def test_single_flipped_pixels_at_the_lanes_ends(vision, c):
    """One ROI pixel changed per frame, at the ends of the first and the last live lane's groups of k_map_crc, in the first and the
    last row: every frame's entry carries zlib.crc32 of the oracle's ui_map, and every frame sends a Map."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, per, refs = L.flipped_oracle(c)
    n = len(frames)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, c.W, c.H, n)
    feed = smh.WebFeed(vision, _full(c.rw, c.rh, n), n)
    try:
        for gray in (True, False):
            fb.run(d.data_ptr(), n, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=gray, max_gap=L.MAX_GAP, anchors=smh.make_anchors(per), stream=s)
            _records_equal_oracle(fb, refs, range(n), n, True, (c, gray))
            fr = [L.ref_frame(r, gray, c.rw, c.rh) for r in refs]
            want = W.feed(fr)
            assert want["n_maps"] == n and [e[3] for e in want["entries"] if e[1] == W.MAP] == [zlib.crc32(f[2][2]) for f in fr]
            _feed_at_every_split(fb, feed, s, want, {f: fr[f][2][2] for f in range(n)}, (c.W, c.H, gray, "flipped"))
    finally:
        feed.close()
        fb.close()
        del d
