"""The remote-viewer feed where its plain path had not been: one call of more than 1024 frames (k_feed_plan's chunk loop and the
state it carries from chunk to chunk, k_feed_maps' persistent grid beyond one pass), and the layouts k_map_crc and k_feed_maps
branch on (the rows of tests/geometry_sweep_cases.py listed in FEED_SWEEP).

A long call is an INDEX LIST over four unique frames -- X, Y, Z open with pairwise different ui_maps, and X with its button
painted over -- so the oracle runs once per unique frame and a device batch is a gather of the four.  Every named sequence is
a list of sub-ranges of one of three index lists ("masters") and carries a check that asserts on tests/web_ref.py's feed() why it
exists; every capacity cut asserts its frames_done there; MUTANTS are copies of feed() with one rule of the chunk loop changed,
each told apart from feed() by the sequence named for it.  The launch arithmetic of csrc/smh_feed.hip is RESTATED below, so a
change of a limit in the library fails here instead of testing something else.  Pure numpy plus the library's host-only
bounds helpers; the oracle is imported inside the functions that need it."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import squad_mortar_helper_amd as smh
import geometry_sweep_cases as G
import minimap_scenes as M
import web_ref as W

# ---- the launch arithmetic, restated (smh_feed.hip: k_feed_plan, k_feed_maps, k_map_crc) ------------------------------------------
FEED_PLAN_BS = 1024                          # frames per chunk of k_feed_plan: one thread per frame
FEED_COPY_GRID = 2048                        # workgroups of k_feed_maps; an item is one workgroup's share of one Map
FEED_COPY_BS, FEED_COPY_GROUPS = 256, 4      # threads per workgroup, 16-byte groups per thread and item
CRC_LANES = 64                               # lanes of a wave of k_map_crc; a lane owns K consecutive 16-byte groups of a row
CRC_LOADS = 4                                # ... and loads them four at a time
B = FEED_PLAN_BS
N_LONG = 2 * B + 64                          # the frames of every long batch
MAX_GAP = 15


def items_per_map(rw, rh):
    """Copy items of one Map: ceil(ceil(rw * rh / 4) / 1024)."""
    groups = (rw * rh + 3) // 4
    per_item = FEED_COPY_BS * FEED_COPY_GROUPS
    return (groups + per_item - 1) // per_item


def copy_passes(n_maps, rw, rh):
    """How often the busiest workgroup of the copy grid goes round its loop."""
    return -(-(n_maps * items_per_map(rw, rh)) // FEED_COPY_GRID)


def crc_lanes(c):
    """(K, live lanes, rounds of the four-load loop) of k_map_crc at a sweep row."""
    K = -(-c.m_quads // CRC_LANES)
    return K, -(-c.m_quads // K), -(-K // CRC_LOADS)


# ---- the geometry of the long calls and its four unique frames --------------------------------------------------------------------
LONG_CASE = next(c for c in G.CASES if (c.W, c.H) == (347, 363))          # rw 33, rh 276, m_xoff 3: a Map is three copy items
X, Y, Z, CLOSED = 0, 1, 2, 3
UNIQUE_NAMES = ("X", "Y", "Z", "closed")
STRIPES = (6, 25, 120, 250)                  # X's stripe columns (left, right) and rows (top, bottom): minimap_scenes' construction
BAR = (60, 1, 13, 137)                       # Y's and Z's scale bar in the quadrant: row, left tick, right tick, the label's meters


def check_long_case():
    c = LONG_CASE
    G.check_table()
    assert c in G.CASES and 8 <= c.rw <= 72 and 2 <= items_per_map(c.rw, c.rh) <= 4
    assert N_LONG > 2 * B and N_LONG <= 65535
    # find_scale_width looks round(20 / 640 * qw) rows down from an anchor: one row at a quadrant of 16 columns, none below
    assert c.rw // 2 == 16 and int(np.floor(20.0 / 640.0 * (c.rw // 2) + 0.5)) == 1


def unique_frame(which):
    """One of the four BGRA frames of LONG_CASE -> (frame, (scales_start_y, anchors)).  Quiet terrain (geometry_sweep_cases) with
    X: a marker line and four stripes that find_minimap stops on (its rectangle is a proper part of the ROI), no scale bar;
    Y: no marker pixel at all, no stripe (the walks end on the ROI's own edges), a scale bar of ten pixels with its label anchor;
    Z: a marker line and the bar; closed: X with the button's rectangle painted over."""
    c = LONG_CASE
    src = X if which == CLOSED else which
    rng = np.random.default_rng(7100 + src)
    rx, ry, rw, rh = smh.map_bounds(c.W, c.H)
    bx, by, bw, bh = smh.button_bounds(c.W, c.H)
    qw, qh = rw // 2, rh // 2
    f = np.empty((c.H, c.W, 4), np.uint8)
    f[..., :3] = 32
    f[..., 3] = 255
    if which != CLOSED:
        f[by:by + bh, bx:bx + bw, :3] = G.BUTTON_RED
    roi = f[ry:ry + rh, rx:rx + rw, :3]
    roi[...] = G._quiet(rng, (rh, rw))
    if src in (X, Z):
        G._draw_line(roi, 28, 8, 28, 110, 3, (G.GREEN, None, G.PURPLE)[src])
    anchors = (0, [])
    if src == X:
        l, r, t, b = STRIPES
        stripe = np.array(M.STRIPE, np.uint8)[::-1]
        roi[:, l - 1:l + 2] = stripe
        roi[:, r - 1:r + 2] = stripe
        roi[t - 1:t + 2, :] = stripe
        roi[b - 1:b + 2, :] = stripe
    else:
        yb, xl, xr, meters = BAR
        q = roi[qh:2 * qh, qw:2 * qw]
        q[yb, xl:xr + 1] = 0
        q[yb:yb + 7, xl] = 0
        q[yb:yb + 7, xr] = 0
        anchors = (yb, [(meters, (xl + xr) // 2, yb)])
    return f, anchors


def oracle_frames(frames, per):
    """The CPU oracle on each frame (per[i] = (scales_start_y, anchors)) -> refs as geometry_sweep_cases.oracle_of makes them:
    process_frame's dict with the grey ui_map, plus ui_colour and minimap for an open frame."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o

    def one(i):
        ref = o.process_frame(frames[i], grayscale=True, max_gap=MAX_GAP, stages=0xF, anchors=per[i][1] or None, scales_start_y=per[i][0], want_images=True)
        if ref["map_open"]:
            ref["ui_colour"] = o.process_frame(frames[i], grayscale=False, stages=0x2, want_images=True)["ui_map"]
            ref["minimap"] = o.find_minimap(frames[i])
        return ref
    with ThreadPoolExecutor(min(len(frames), 8)) as ex:
        return list(ex.map(one, range(len(frames))))


@functools.lru_cache(maxsize=1)
def unique_oracle():
    """-> (frames uint8 [4, H, W, 4], per-frame (scales_start_y, anchors), the oracle's refs)."""
    made = [unique_frame(k) for k in (X, Y, Z, CLOSED)]
    frames = np.stack([m[0] for m in made])
    per = [m[1] for m in made]
    return frames, per, oracle_frames(frames, per)


def ref_frame(ref, gray, rw, rh, with_minimap=True):
    """web_ref.feed's input for a frame from the ORACLE's record and ui_map (with_minimap: the run had SMHV_STAGE_MINIMAP)."""
    if not ref["map_open"]:
        return (False, W.FRAME_OK, None, np.zeros((0, 4), np.float32), False, 0.0, False, (0, 0, 0, 0))
    ui = ref["ui_map"] if gray else ref["ui_colour"]
    assert ui.shape == (rh, rw, 4)
    has_mm = with_minimap and ref.get("minimap") is not None
    return (True, W.FRAME_OK, (rw, rh, ui.tobytes()), ref["lines"], ref["mpx"] is not None, ref["mpx"] or 0.0, has_mm, tuple(ref["minimap"]) if has_mm else (0, 0, 0, 0))


def check_unique(refs):
    """Every property the sequences lean on, asserted on the oracle's output -- not assumed from how a frame was drawn."""
    c = LONG_CASE
    assert [r["map_open"] for r in refs] == [1, 1, 1, 0]
    for gray in (True, False):
        uis = [ref_frame(r, gray, c.rw, c.rh)[2][2] for r in refs[:3]]
        assert len({zlib.crc32(u) for u in uis}) == 3                                  # X, Y, Z: pairwise different ui_maps
    assert refs[X]["n_lines"] >= 1 and refs[Z]["n_lines"] >= 1 and refs[Y]["n_lines"] == 0 and refs[Y]["n_mask_px"] == 0
    l, r, t, b = STRIPES
    whole = (0, c.rw - 1, 0, c.rh - 1)
    assert refs[X]["minimap"] == M.designed_rect((None, l, r, t, b, None), c.rw, c.rh) != whole   # a rectangle that was drawn
    assert refs[Y]["minimap"] == whole and refs[Z]["minimap"] == whole                  # none drawn: the walks end on the ROI's edges
    assert refs[X]["mpx"] is None and refs[Y]["mpx"] == refs[Z]["mpx"] == BAR[3] / 10.0  # ticks at 1 and 13: left 2, right 12


# ---- the three index lists --------------------------------------------------------------------------------------------------------
_PATTERN = (X, X, Y, CLOSED, Z, Z, X, CLOSED, CLOSED, Y, Y, Z, X)                        # (13 frames: no multiple of it is a power of two)
EDGE_SAME_AT, EDGE_DIFF_AT, CLOSED_TAIL_AT = 1100, 1200, 1500                           # where `mixed` holds X X / X Y / X closed closed X
CUT_MID, CUT_RUN, CUT_RUN_LEN = B + 517, B + 300, 5


def _mixed():
    m = np.array([_PATTERN[i % len(_PATTERN)] for i in range(N_LONG)])
    m[B - 2:B + 1] = (Y, X, Z)                                                           # open on both sides of the first chunk's end
    m[2 * B - 1:2 * B + 1] = (X, Y)                                                      # ... and of the second's
    m[EDGE_SAME_AT:EDGE_SAME_AT + 2] = (X, X)
    m[EDGE_DIFF_AT:EDGE_DIFF_AT + 2] = (X, Y)
    m[CLOSED_TAIL_AT:CLOSED_TAIL_AT + 4] = (X, CLOSED, CLOSED, X)
    m[CUT_MID:CUT_MID + 2] = (Y, Z)
    m[CUT_RUN:CUT_RUN + CUT_RUN_LEN + 2] = (X,) + (CLOSED,) * CUT_RUN_LEN + (Y,)
    return m


def _closed():
    """A mixed first chunk that ends on X, a second chunk of closed frames only, then X, Y and the pattern."""
    m = _mixed()
    m[B - 1] = X
    m[B:2 * B] = CLOSED
    m[2 * B:2 * B + 2] = (X, Y)
    return m


MASTERS = {"all": np.array([(X, Y, Z)[i % 3] for i in range(N_LONG)]), "closed": _closed(), "mixed": _mixed()}


def master_ref(master, uniq):
    """web_ref.feed's frames of a master from the four unique ones' (uniq = [ref_frame(...)] * 4)."""
    return [uniq[i] for i in MASTERS[master]]


# ---- named sequences --------------------------------------------------------------------------------------------------------------
# A sequence is a list of PARTS on one master; a part is one feed (capacity None: room for everything; else a function of the
# master's frames) and its calls (first, n, snapshot) in order, the stored CRC carried from call to call as the device carries it.
Part = namedtuple("Part", "capacity calls")
Seq = namedtuple("Seq", "name master parts check")


def run_reference(seq, frames, feed=W.feed):
    """-> [[feed(...) of every call] of every part], by `feed` (web_ref.feed or a mutant of it)."""
    out = []
    for part in seq.parts:
        cap = None if part.capacity is None else part.capacity(frames)
        stored, res = None, []
        for first, n, snapshot in part.calls:
            r = feed(frames[first:first + n], stored=stored, capacity=cap, snapshot=snapshot, first=first)
            stored = r["stored"]
            res.append(r)
        out.append(res)
    return out


def _maps(r):
    return [f for f, kind, _, _ in r["messages"] if kind == W.MAP]


def end_of(r, frame):
    """Where frame `frame`'s last message ends in the buffer."""
    last = [e for e in r["entries"] if e[0] == frame][-1]
    return last[4] + last[2]


def _crc(fr):
    return zlib.crc32(fr[2][2])


def _check_edge_same(res, fr):
    (r,), first = res[0], SEQUENCES["edge_same"].parts[0].calls[0][0]
    a, b = fr[first + B - 1], fr[first + B]
    assert a[0] and b[0] and _crc(a) == _crc(b)
    assert first + B - 1 in [e[0] for e in r["entries"]] and first + B not in _maps(r) and r["frames_done"] > B


def _check_edge_diff(res, fr):
    (r,), first = res[0], SEQUENCES["edge_diff"].parts[0].calls[0][0]
    a, b = fr[first + B - 1], fr[first + B]
    assert a[0] and b[0] and _crc(a) != _crc(b) and first + B in _maps(r)


def _closed_tail_capacity(frames):
    first, n, _ = SEQUENCES["closed_tail"].parts[0].calls[0]
    cap = end_of(W.feed(frames[first:first + n], first=first), first + B - 3)
    assert cap >= W.worst_case(LONG_CASE.rw, LONG_CASE.rh)
    return cap


def _check_closed_tail(res, fr):
    first = SEQUENCES["closed_tail"].parts[0].calls[0][0]
    a, b = fr[first + B - 3], fr[first + B]
    assert a[0] and b[0] and _crc(a) == _crc(b) and not fr[first + B - 2][0] and not fr[first + B - 1][0]
    (r,), (cut,) = res
    assert first + B not in _maps(r) and first + B in [e[0] for e in r["entries"]]
    # the same call with room up to frame B - 3's end: the closed frames are consumed, frame B is not; bytes_used lies in chunk 0
    assert cut["frames_done"] == B and cut["bytes_used"] == end_of(r, first + B - 3) and cut["entries"][-1][0] == first + B - 3


def _check_closed_chunk(res, fr):
    assert fr[B - 1][0] and fr[2 * B][0] and _crc(fr[B - 1]) == _crc(fr[2 * B]) and not any(f[0] for f in fr[B:2 * B])
    (r,), (two,), (one,) = res
    assert 2 * B not in _maps(r) and r["frames_done"] == 2 * B + 1 and r["entries"][-1][0] == 2 * B
    assert one["frames_done"] == B and two["frames_done"] == 2 * B
    assert (two["entries"], two["bytes_used"], two["stored"]) == (one["entries"], one["bytes_used"], one["stored"]) and one["bytes_used"] > 0
    assert r["entries"][:len(one["entries"])] == one["entries"] and r["entries"][len(one["entries"])][4] == 6 + W.slot(one["bytes_used"] - 6)


def _check_closed_first_chunk(res, fr):
    (before, r), = res
    assert fr[B - 1][0] and before["n_maps"] == 1 and before["stored"] == _crc(fr[B - 1])
    assert not any(f[0] for f in fr[B:2 * B]) and _crc(fr[2 * B]) == before["stored"] and _crc(fr[2 * B + 1]) != before["stored"]
    first_map = next(e for e in r["entries"] if e[1] == W.MAP)
    assert (first_map[0], first_map[3]) == (2 * B + 1, _crc(fr[2 * B + 1])) and r["entries"][0][0] == 2 * B


def _check_all_maps(res, fr):
    (r,), c = res[0], LONG_CASE
    assert r["n_maps"] == r["frames_done"] == N_LONG and r["n_maps"] * items_per_map(c.rw, c.rh) > 2 * FEED_COPY_GRID
    assert copy_passes(r["n_maps"], c.rw, c.rh) >= 3


def _check_lengths(res, fr):
    assert [r["frames_done"] for (r,) in res] == [B - 1, B, B + 1, 2 * B, 2 * B + 1]
    assert all(fr[k][0] for k in (B - 2, B - 1, B, 2 * B - 1, 2 * B))                      # every call ends on an open frame
    assert len({(len(r["entries"]), r["bytes_used"]) for (r,) in res}) == len(res)


def _check_snapshot_long(res, fr):
    (before, snap, after), = res
    assert snap["frames_done"] == 2 * B + 1 and snap["stored"] == before["stored"] is not None
    assert snap["n_maps"] == sum(1 for f in fr[:2 * B + 1] if f[0]) > 2 * B // 2 and _maps(snap)[-1] == 2 * B
    first, n, _ = SEQUENCES["snapshot_long"].parts[0].calls[2]
    assert after == W.feed(fr[first:first + n], stored=before["stored"], first=first)    # as if the snapshot had not happened
    assert after != W.feed(fr[first:first + n], stored=_crc(fr[2 * B]), first=first)     # ... which a kept snapshot CRC would change


_LENGTHS = (B - 1, B, B + 1, 2 * B, 2 * B + 1)
_SEQS = [
    Seq("all_maps", "all", [Part(None, [(0, N_LONG, False)])], _check_all_maps),
    Seq("closed_chunk", "closed", [Part(None, [(0, 2 * B + 1, False)]), Part(None, [(0, 2 * B, False)]), Part(None, [(0, B, False)])], _check_closed_chunk),
    Seq("closed_first_chunk", "closed", [Part(None, [(B - 1, 1, False), (B, B + 64, False)])], _check_closed_first_chunk),
    Seq("edge_same", "mixed", [Part(None, [(EDGE_SAME_AT - (B - 1), B + 20, False)])], _check_edge_same),
    Seq("edge_diff", "mixed", [Part(None, [(EDGE_DIFF_AT - (B - 1), B + 20, False)])], _check_edge_diff),
    Seq("closed_tail", "mixed", [Part(None, [(CLOSED_TAIL_AT - (B - 3), B + 20, False)]), Part(_closed_tail_capacity, [(CLOSED_TAIL_AT - (B - 3), B + 20, False)])],
        _check_closed_tail),
    Seq("lengths", "mixed", [Part(None, [(0, n, False)]) for n in _LENGTHS], _check_lengths),
    Seq("snapshot_long", "mixed", [Part(None, [(0, 40, False), (0, 2 * B + 1, True), (40, 60, False)])], _check_snapshot_long),
]
SEQUENCES = {s.name: s for s in _SEQS}
SEQ_NAMES = [s.name for s in _SEQS]                                                     # (grouped by master: a device batch is run once per group)


# ---- capacity cuts on `mixed`, the whole master in one call ------------------------------------------------------------------------
Cut = namedtuple("Cut", "name capacity frames_done why")
CUTS = [
    Cut("chunk0_last_fits", lambda r: end_of(r, B - 1), B, "the capacity ends with frame B - 1: the first frame of chunk 1 does not fit"),
    Cut("chunk0_last_does_not_fit", lambda r: end_of(r, B - 1) - 1, B - 1, "one byte less"),
    Cut("middle_of_chunk1", lambda r: end_of(r, CUT_MID), CUT_MID + 1, "the capacity ends with a frame in the middle of chunk 1"),
    Cut("closed_run_before_the_cut", lambda r: end_of(r, CUT_RUN), CUT_RUN + CUT_RUN_LEN + 1, "... with an open frame, a run of closed ones behind it: they are consumed"),
]
CUT_NAMES = [c.name for c in CUTS]


def cut_capacity(cut, frames):
    c = LONG_CASE
    cap = cut.capacity(W.feed(frames))
    assert cap >= W.worst_case(c.rw, c.rh)
    return cap


def check_cut(cut, frames, feed=W.feed):
    """The cut's frames_done on `feed`, and what makes it mean something on the frames."""
    assert all(frames[k][0] for k in (B - 2, B - 1, B, CUT_MID, CUT_MID + 1, CUT_RUN, CUT_RUN + CUT_RUN_LEN + 1))
    assert not any(frames[k][0] for k in range(CUT_RUN + 1, CUT_RUN + CUT_RUN_LEN + 1))
    r = feed(frames, capacity=cut_capacity(cut, frames))
    assert r["frames_done"] == cut.frames_done, (cut.name, r["frames_done"])
    return r


def rounds_of(frames, capacity, feed=W.feed):
    """Feeding again from first + frames_done until the end -> ([every round's result], the messages of all rounds, the stored CRC)."""
    first, stored, parts, msgs = 0, None, [], []
    while first < len(frames):
        r = feed(frames[first:], stored=stored, capacity=capacity, first=first)
        assert r["frames_done"] >= 1
        parts.append(r)
        msgs += r["messages"]
        first, stored = first + r["frames_done"], r["stored"]
    return parts, msgs, stored


# ---- mutants: web_ref.feed with one rule of the chunk loop changed -------------------------------------------------------------------
# mutant -> the sequence (or cut) that must tell it apart
MUTANTS = {
    "crc_forgotten_at_chunk_start": "edge_same",          # (a) the stored CRC is forgotten at every multiple of B
    "crc_not_taken_from_closed_tail": "closed_tail",      # (b) ... is not taken over from a chunk whose last frames are closed
    "layout_not_carried_over_closed_chunk": "closed_chunk",   # (c) bytes_used / off / the entry count do not survive a chunk without an open frame
    "done_rounded_to_chunk": "middle_of_chunk1",          # (d) frames_done is the chunk's base when the cut falls inside a later chunk
    "cut_in_first_chunk_only": "middle_of_chunk1",        # (e) the cut is looked for in the first chunk only
}


def mutant_feed(rule):
    assert rule in MUTANTS

    def feed(frames, stored=None, capacity=None, snapshot=False, first=0):
        off, used, done, n_maps = 6, 0, 0, 0
        messages, entries = [], []
        chunk_stored, chunk_open = stored, False
        for i, fr in enumerate(frames):
            if i % B == 0:
                chunk_stored, chunk_open = stored, False
                if i and rule == "crc_forgotten_at_chunk_start":
                    stored = None
            ev, crc, after = W.frame_events(fr, stored, snapshot)
            if ev:
                o, placed = off, []
                for kind, data in ev:
                    placed.append((o, kind, data))
                    o += W.slot(len(data))
                end = placed[-1][0] + len(placed[-1][2])
                if capacity is not None and end > capacity and not (rule == "cut_in_first_chunk_only" and i >= B):
                    if rule == "done_rounded_to_chunk" and i >= B:
                        done = i - i % B
                    break
                for po, kind, data in placed:
                    messages.append((first + i, kind, crc, data))
                    entries.append((first + i, kind, len(data), crc, po))
                    n_maps += kind == W.MAP
                off, used, chunk_open = o, end, True
            stored = after
            done = i + 1
            if (i + 1) % B == 0:
                if rule == "crc_not_taken_from_closed_tail" and not ev:
                    stored = chunk_stored
                if rule == "layout_not_carried_over_closed_chunk" and not chunk_open:
                    off, used, n_maps, messages, entries = 6, 0, 0, [], []
        return dict(messages=messages, entries=entries, frames_done=done, n_maps=n_maps, stored=stored, bytes_used=used)
    return feed


def mutant_is_told_apart(rule, uniq):
    """Does the sequence (or cut) named for the mutant give another result under it than under web_ref.feed?"""
    name = MUTANTS[rule]
    if name in SEQUENCES:
        seq = SEQUENCES[name]
        fr = master_ref(seq.master, uniq)
        return run_reference(seq, fr, mutant_feed(rule)) != run_reference(seq, fr)
    cut = next(c for c in CUTS if c.name == name)
    fr = master_ref("mixed", uniq)
    cap = cut_capacity(cut, fr)
    return mutant_feed(rule)(fr, capacity=cap)["frames_done"] != W.feed(fr, capacity=cap)["frames_done"]


# ---- the sweep rows for the CRC and the copy ---------------------------------------------------------------------------------------
_SWEEP_SIZES = [(319, 360), (343, 361), (454, 361), (563, 363), (567, 362), (567, 360), (568, 361), (1331, 362), (1335, 360), (1336, 361), (2233, 361),
                (2360, 360), (2361, 362), (4407, 360), (4407, 361), (1281, 721)]
FEED_SWEEP = [next(c for c in G.CASES if (c.W, c.H) == s) for s in _SWEEP_SIZES]
FEED_SWEEP_IDS = ["%dx%d" % (c.W, c.H) for c in FEED_SWEEP]
FLIP_CASES = [next(c for c in FEED_SWEEP if (c.W, c.H) == s) for s in ((567, 360), (568, 361))]     # m_xoff == 0; m_quads == 65
FLIP_IDS = ["%dx%d" % (c.W, c.H) for c in FLIP_CASES]
ROWS_PER_WAVE = (0, 1, 3, 8, 64)             # smhv_debug_feed_rows: the library's rule, and every split of the rows over the waves worth having


def check_sweep():
    rows = FEED_SWEEP
    G.check_table()                                                                      # (every row is a row of that table, held to map_bounds)
    assert all(c in G.CASES for c in rows) and len(set(rows)) == len(rows)
    have = lambda f: {f(c) for c in rows}                                                # noqa: E731
    assert have(lambda c: c.m_xoff) == {0, 1, 2, 3}
    assert have(lambda c: c.m_quads) >= {2, 63, 64, 65, 255, 256, 257, 513, 1024} and have(lambda c: c.rw) >= {8}
    assert have(lambda c: c.rw % 4) == {0, 1, 2, 3} and have(lambda c: (c.rw * c.rh) % 4) == {0, 1, 2, 3}
    assert any(c.group == "real" for c in rows) and all(c.rh <= 276 for c in rows if c.group != "real")
    assert (4096, 274) in have(lambda c: (c.rw, c.rh)) and max(c.rw * c.rh * 4 for c in rows) <= 4096 * 276 * 4      # the largest Map: about 4.5 MB
    # what the m_quads are there for: K = 1 with 63 and 64 live lanes, K = 2 with 33, K = 4 (one full round of the four-load loop),
    # K = 5 with 52 lanes (a second, partial round), K = 9 and K = 16
    assert have(crc_lanes) >= {(1, 2, 1), (1, 63, 1), (1, 64, 1), (2, 33, 1), (4, 64, 1), (5, 52, 2), (9, 57, 3), (16, 64, 4)}
    assert [(c.m_xoff == 0, c.m_quads == 65) for c in FLIP_CASES] == [(True, False), (False, True)]


def flip_spots(c):
    """(row, column) of the ROI pixels the flipped batch changes one at a time: in rows 0 and rh - 1 the first and the last pixel
    of the first and the last live lane's groups of k_map_crc, the pixel before the last lane's first, and the row's last."""
    K, lanes, _ = crc_lanes(c)
    first = lambda lane: max(4 * lane * K - c.m_xoff, 0)                                 # noqa: E731
    last = lambda lane: min(4 * min(lane * K + K, c.m_quads) - c.m_xoff, c.rw) - 1       # noqa: E731
    cols = sorted({first(0), last(0), first(lanes - 1) - 1, first(lanes - 1), last(lanes - 1), c.rw - 1})
    assert cols[0] == 0 and cols[-1] == c.rw - 1 and first(lanes - 1) == 4 * (lanes - 1) * K - c.m_xoff and len(cols) >= 4
    return [(r, col) for r in (0, c.rh - 1) for col in cols]


@functools.lru_cache(maxsize=2)
def flipped_oracle(c):
    """The case's first frame and one copy per flip_spots(c) with the top bit of that pixel's three colours flipped -> (frames, per-frame anchors, refs)."""
    frame, info = G.make_frame(c, 1000 * G.CASES.index(c) + 1)
    rx, ry, _, _ = smh.map_bounds(c.W, c.H)
    frames = [frame]
    for (py, px) in flip_spots(c):
        f = frame.copy()
        f[ry + py, rx + px, :3] ^= 0x80                                                  # (no signs of 128 x the luma weights sum to 0: the grey ui_map changes too)
        frames.append(f)
    frames = np.stack(frames)
    per = [(info["scales_start_y"], info["anchors"])] * len(frames)
    return frames, per, oracle_frames(frames, per)
