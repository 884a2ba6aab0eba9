"""The cases of the feed's map tiles (smhv_batch_feed_tiles / smhv_feed_frame_tiles): sizes, frames and call scripts, each with a
check that asserts on the restatement alone (tests/web_tiles_ref.py) why the case exists; MUTANTS are feed_tiles with one rule
changed, each told apart from it by the case named for it.

A case is a script of calls on ONE feed over one or two batches; a batch is a list of KEYS of unique frames at a row of
tests/geometry_sweep_cases.py (held to smh.map_bounds by its check_table): "X" the sweep's scene, "Y" another seed (every tile
differs), "closed" the button painted over, "falpha" X with other alpha bytes in the frame (the ui_map's alpha is 255 whatever the
frame's), "outside" X with the pixels round the ROI changed, ("flip", tiles) X with the first pixel of each listed tile flipped,
("px", y, x) X with that ROI pixel flipped.  PATCHES change a batch's ui slab on the device after the run, where no frame can reach:
("alpha", batch, position, y, x, value) one alpha byte of the ui_map (the restatement's ui_map gets it too), ("leadin" / "pitchpad",
batch, position) the bytes in front of and behind the map's rows in the slab (not part of the map), ("status", batch, position)
the record's status away from SMHV_FRAME_OK.  Pure numpy plus the library's host-only bounds helpers; the oracle is imported by
ui_of() only."""
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

import squad_mortar_helper_amd as smh
import geometry_sweep_cases as G
import web_ref as W
import web_tiles_ref as T

# ---- sizes: rows of the sweep's table, each chosen for a residue of the tile grid ------------------------------------------------------
_SIZES = {
    "33x276": (347, 363),      # rw < 64: one clipped column; m_xoff 3; the long call's size
    "8x274": (319, 360),       # rw < 64, the narrowest map; m_xoff 0
    "101x271": (409, 356),     # rh % 16 == 15; m_xoff 1; the corner tile is 37 x 15: (cw * ch) % 4 == 3
    "72x272": (381, 357),      # rh % 16 == 0; m_xoff 2
    "90x273": (401, 359),      # rh % 16 == 1; m_xoff 0; the corner tile is 26 x 1: (cw * ch) % 4 == 2
    "256x274": (567, 360),     # rw % 64 == 0
    "1921x276": (2235, 363),   # rw % 64 == 1; the one row of the table where some set of tiles gives L == 10 + 4 w h exactly
    "1919x276": (2232, 362),   # rw % 64 == 63
}
SIZES = {k: next(c for c in G.CASES if (c.W, c.H) == s) for k, s in _SIZES.items()}
SIZE_NAMES = list(SIZES)
MAIN = SIZES["101x271"]                                        # the sequences and continuations: two tile columns, 17 tile rows
OTHER = SIZES["72x272"]
LONG = SIZES["33x276"]
EQUAL = SIZES["1921x276"]
PLAN_BS = 1024                                                 # frames per chunk of the plan (csrc/smh_feedtiles.hip: TILES_PLAN_BS)


def check_sizes():
    G.check_table()
    cs = list(SIZES.values())
    assert all(c in G.CASES and c.rh <= 276 for c in cs)                                   # (the table has a row for every property below)
    have = lambda f: {f(c) for c in cs}                                                    # noqa: E731
    assert have(lambda c: c.rw % 64) >= {0, 1, 63} and {c.rw for c in cs if c.rw < 64} == {8, 33}
    assert have(lambda c: c.rh % 16) >= {0, 1, 15} and have(lambda c: c.m_xoff) == {0, 1, 2, 3}
    assert any(((c.rw % 64) * (c.rh % 16)) % 4 != 0 for c in cs)
    assert [(c.rw % 64) * (c.rh % 16) % 4 for c in (SIZES["101x271"], SIZES["90x273"])] == [3, 2]
    assert (LONG.W, LONG.H) == (347, 363)


# ---- unique frames ---------------------------------------------------------------------------------------------------------------------
def _flip(f, c, y, x):
    rx, ry, _, _ = smh.map_bounds(c.W, c.H)
    f[ry + y, rx + x, :3] ^= 0x80                              # (no signs of 128 x the luma weights sum to 0: the grey ui_map changes too)


@functools.lru_cache(maxsize=64)
def _scene(c, which):
    seed = 1000 * G.CASES.index(c) + (7 if which == "Y" else 1)
    return G.make_frame(c, seed, open_=which != "closed")[0]


def frame_of(c, key):
    """The BGRA frame of a key at size c."""
    if key in ("X", "Y", "closed"):
        return _scene(c, key)
    f = _scene(c, "X").copy()
    rx, ry, rw, rh = smh.map_bounds(c.W, c.H)
    if key == "falpha":
        f[..., 3] = np.random.default_rng(5).integers(0, 255, f.shape[:2], dtype=np.uint8)
    elif key == "outside":
        for sl in ((slice(ry - 1, ry), slice(rx - 1, rx + rw + 1)), (slice(ry + rh, ry + rh + 1), slice(rx - 1, rx + rw + 1)),
                   (slice(ry, ry + rh), slice(rx - 1, rx)), (slice(ry, ry + rh), slice(rx + rw, rx + rw + 1))):
            f[sl[0], sl[1], :3] ^= 0x80
    elif key[0] == "px":
        _flip(f, c, key[1], key[2])
    elif key[0] == "flip":
        for t in key[1]:
            x0, y0, _, _ = T.tile_rect(rw, rh, t)
            _flip(f, c, y0, x0)
    else:
        raise KeyError(key)
    return f


@functools.lru_cache(maxsize=None)
def ui_of(c, key, gray):
    """The ORACLE's ui_map of a unique frame (bytes), or None where it finds the map closed."""
    from oracle import oracle as o
    ref = o.process_frame(frame_of(c, key), grayscale=gray, stages=0x2, want_images=True)
    return ref["ui_map"].tobytes() if ref["map_open"] else None


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
# steps: ("tiles" | "plain", batch, first, n), ("frame", batch, position) the per-call path on that frame, ("reset",)
Case = namedtuple("Case", "name batches patches capacity steps check")
BLANK = (np.zeros((0, 4), np.float32), False, 0.0, False, (0, 0, 0, 0))


def ref_frames(case, gray, records=None):
    """The restatement's frames of every batch of the case: the oracle's ui_maps with the case's patches; records[b][i] = (lines,
    has_mpx, mpx, has_minimap, minimap) from the device's records, or None: blank ones."""
    out = []
    for b, (c, keys) in enumerate(case.batches):
        frames = []
        for i, key in enumerate(keys):
            ui = ui_of(c, key, gray)
            rec = BLANK if records is None else records[b][i]
            status = 1 if ("status", b, i) in case.patches else W.FRAME_OK
            if ui is not None:
                img = np.frombuffer(ui, np.uint8).reshape(c.rh, c.rw, 4).copy()
                for p in case.patches:
                    if p[0] == "alpha" and p[1:3] == (b, i):
                        img[p[3], p[4], 3] = p[5]
                ui = img.tobytes()
            frames.append((ui is not None, status, (c.rw, c.rh, ui) if ui is not None else None) + tuple(rec))
        out.append(frames)
    return out


def run_reference(case, fr, rule=None):
    """-> [the result of every step (None for a reset)], by feed_tiles (rule: a mutant's) and web_ref.feed, the stored CRC and the
    kept map carried from step to step as the device carries them."""
    cap = None if case.capacity is None else case.capacity(fr)
    stored, kept, out = None, None, []
    for st in case.steps:
        if st[0] == "reset":
            stored = None
            out.append(None)
            continue
        if st[0] == "frame":
            _, b, pos = st
            r = T.feed_tiles([fr[b][pos][:3] + BLANK], stored=stored, kept=kept, capacity=cap, rule=rule)
        else:
            kind, b, first, n = st
            if kind == "tiles":
                r = T.feed_tiles(fr[b][first:first + n], stored=stored, kept=kept, capacity=cap, first=first, rule=rule)
            else:
                r = dict(W.feed(fr[b][first:first + n], stored=stored, capacity=cap, first=first), kept=kept)
        stored, kept = r["stored"], r["kept"]
        out.append(r)
    return out


def slot_kinds(r):
    """[(frame, kind)] of the Map and MapTiles messages of a result."""
    return [(f, k) for f, k, _, _ in r["messages"] if k in (W.MAP, T.MAP_TILES)]


def tiles_in(r, frame):
    """The tile indices of frame `frame`'s MapTiles message."""
    d = next(d for f, k, _, d in r["messages"] if f == frame and k == T.MAP_TILES)
    return list(struct.unpack_from("<%dI" % struct.unpack_from("<I", d, 14)[0], d, 26))


def _tile_at(c, y, x):
    return (y // T.TH) * T.grid(c.rw, c.rh)[0] + x // T.TW


def corner_tiles(c):
    """The tiles whose four corners are flipped: an interior one (where the grid has one), one of the clipped last column, one of
    the clipped last row, the corner tile."""
    tx, ty = T.grid(c.rw, c.rh)
    tiles = [1 * tx + 0] if tx > 1 else []                                                 # tile row 1, column 0: full, neighbours on three sides
    tiles += [1 * tx + tx - 1, (ty - 1) * tx + 0, tx * ty - 1]
    return sorted(set(tiles))


def _corners_case(name, c):
    spots = []
    for t in corner_tiles(c):
        x0, y0, cw, ch = T.tile_rect(c.rw, c.rh, t)
        spots += [(t, y, x) for y, x in dict.fromkeys([(y0, x0), (y0, x0 + cw - 1), (y0 + ch - 1, x0), (y0 + ch - 1, x0 + cw - 1)])]
    keys = ["X"]
    for _, y, x in spots:
        keys += [("px", y, x), "X"]

    def check(res, fr):
        (r,) = res
        assert slot_kinds(r)[0] == (0, W.MAP) and all(k == T.MAP_TILES for _, k in slot_kinds(r)[1:]) and len(slot_kinds(r)) == len(keys)
        for k, (t, y, x) in enumerate(spots):
            assert _tile_at(c, y, x) == t and tiles_in(r, 2 * k + 1) == [t] and tiles_in(r, 2 * k + 2) == [t], (name, k)
        assert r["n_maps"] == 1 and r["frames_done"] == len(keys)
    return Case(name + "/corners", [(c, keys)], [], None, [("tiles", 0, 0, len(keys))], check)


def _alpha_case(name, c):
    y, x = c.rh - 1, c.rw - 1                                                              # in the corner tile
    t = _tile_at(c, y, x)

    def check(res, fr):
        (r,) = res
        assert fr[0][1][2] == fr[0][0][2] and fr[0][2][2] != fr[0][0][2]                    # the frame's alpha is not the ui_map's; the patched byte is
        assert slot_kinds(r) == [(0, W.MAP), (2, T.MAP_TILES), (3, T.MAP_TILES)] and tiles_in(r, 2) == [t] == tiles_in(r, 3)
    return Case(name + "/alpha", [(c, ["X", "falpha", "X", "X"])], [("alpha", 0, 2, y, x, 7)], None, [("tiles", 0, 0, 4)], check)


def _outside_case(name, c):
    def check(res, fr):
        (r,) = res
        assert all(f[2] == fr[0][0][2] for f in fr[0]) and slot_kinds(r) == [(0, W.MAP)] and len(r["entries"]) == 9
    return Case(name + "/outside", [(c, ["X", "outside", "X", "X"])], [("leadin", 0, 2), ("pitchpad", 0, 3)], None, [("tiles", 0, 0, 4)], check)


def k_star(c):
    """The least k for which the first k tiles changed give L >= 10 + 4 w h."""
    n = T.grid(c.rw, c.rh)[0] * T.grid(c.rw, c.rh)[1]
    return next(k for k in range(1, n + 1) if T.tiles_len(c.rw, c.rh, range(k)) >= T.map_len(c.rw, c.rh))


def _boundary_case(name, c):
    k, n = k_star(c), T.grid(c.rw, c.rh)[0] * T.grid(c.rw, c.rh)[1]
    keys = ["X", ("flip", tuple(range(k - 1))), "X", ("flip", tuple(range(k))), "X", ("flip", tuple(range(n)))]

    def check(res, fr):
        (r,) = res
        assert 2 <= k <= n and T.tiles_len(c.rw, c.rh, range(n)) > T.map_len(c.rw, c.rh)    # every tile changed: always a Map
        assert slot_kinds(r) == [(0, W.MAP), (1, T.MAP_TILES), (2, T.MAP_TILES), (3, W.MAP), (4, W.MAP), (5, W.MAP)]
        assert tiles_in(r, 1) == list(range(k - 1)) == tiles_in(r, 2)
    return Case(name + "/boundary", [(c, keys)], [], None, [("tiles", 0, 0, len(keys))], check)


def equal_tiles(c):
    """At EQUAL: every full tile, 14 of the last column's, 28 of the last row's and the corner: L == 10 + 4 w h exactly."""
    tx, ty = T.grid(c.rw, c.rh)
    return sorted([r * tx + col for r in range(ty - 1) for col in range(tx - 1)] + [r * tx + tx - 1 for r in range(14)] + [(ty - 1) * tx + col for col in range(28)] + [tx * ty - 1])


def _equal_case():
    c, tiles = EQUAL, tuple(equal_tiles(EQUAL))

    def check(res, fr):
        (r,) = res
        assert T.tiles_len(c.rw, c.rh, tiles) == T.map_len(c.rw, c.rh) and slot_kinds(r) == [(0, W.MAP), (1, W.MAP)]
    return Case("1921x276/equal", [(c, ["X", ("flip", tiles)])], [], None, [("tiles", 0, 0, 2)], check)


P1, P2 = ("px", 20, 5), ("px", 200, 70)                        # at MAIN: tiles 2 and 25


def _seq(name, keys, want, patches=()):
    def check(res, fr):
        (r,) = res
        assert slot_kinds(r) == want, (name, slot_kinds(r))
    return Case("seq/" + name, [(MAIN, keys)], list(patches), None, [("tiles", 0, 0, len(keys))], check)


def _sequences():
    M, Tl = W.MAP, T.MAP_TILES
    return [
        _seq("X Y X", ["X", P1, "X"], [(0, M), (1, Tl), (2, Tl)]),
        _seq("X X", ["X", "X", P1, P1], [(0, M), (2, Tl)]),
        _seq("X closed closed Y", ["X", "closed", "closed", P1], [(0, M), (3, Tl)]),
        _seq("not OK in between", ["X", P2, P1], [(0, M), (2, Tl)], [("status", 0, 1)]),
        _seq("no stored CRC", [P1, "X"], [(0, M), (1, Tl)]),
    ]


def _cut_capacity(fr):
    """Room up to the end of frame 2 of the cut case's first call: frame 3 does not fit."""
    r = T.feed_tiles(fr[0][:5])
    last = [e for e in r["entries"] if e[0] == 2][-1]
    cap = last[4] + last[2]
    assert cap >= W.worst_case(MAIN.rw, MAIN.rh)
    return cap


def _continuations():
    M, Tl = W.MAP, T.MAP_TILES
    out = []

    def add(name, batches, steps, check, capacity=None, patches=()):
        out.append(Case("cont/" + name, batches, list(patches), capacity, steps, check))

    def second_call(res, fr):
        assert slot_kinds(res[0]) == [(0, M), (1, Tl)] and slot_kinds(res[1]) == [(2, Tl)] and slot_kinds(res[2]) == []   # the kept map is P1's; the same frame again sends nothing
    add("second call", [(MAIN, ["X", P1, P2])], [("tiles", 0, 0, 2), ("tiles", 0, 2, 1), ("tiles", 0, 2, 1)], second_call)

    def cut(res, fr):
        # X P1 P2 Y X: Y is a Map and does not fit; the call stops on P2, whose map is kept -- not X's, the batch's last
        assert res[0]["frames_done"] == 3 and slot_kinds(res[0]) == [(0, M), (1, Tl), (2, Tl)] and res[0]["kept"][2] == fr[0][2][2][2]
        assert res[1]["frames_done"] == 1 and slot_kinds(res[1]) == [(3, M)] and slot_kinds(res[2]) == [(4, M)]
        assert slot_kinds(res[3]) == [(2, Tl)] and res[3]["kept"][2] == fr[0][2][2][2]
    add("capacity cut", [(MAIN, ["X", P1, P2, "Y", "X"])], [("tiles", 0, 0, 5), ("tiles", 0, 3, 2), ("tiles", 0, 4, 1), ("tiles", 0, 2, 1)], cut, capacity=_cut_capacity)

    def cut_keeps(res, fr):
        # X P1 P2 Y with room up to P2, then P1 alone: tiles against P2's map (two tiles), not a Map and not against Y's
        assert res[0]["frames_done"] == 3 and slot_kinds(res[1]) == [(1, Tl)] and tiles_in(res[1], 1) == [2, 25]
    add("cut keeps the stop", [(MAIN, ["X", P1, P2, "Y", "X"])], [("tiles", 0, 0, 4), ("tiles", 0, 1, 1)], cut_keeps, capacity=_cut_capacity)

    def reset(res, fr):
        assert slot_kinds(res[0]) == [(0, M)] and slot_kinds(res[2]) == [(1, M)]
    add("reset", [(MAIN, ["X", P1])], [("tiles", 0, 0, 1), ("reset",), ("tiles", 0, 1, 1)], reset)

    def foreign_map(res, fr):
        # tiles X; plain P2 (a Map: the viewers hold P2, the kept map is X's and stale); tiles P1: a Map -- tiles against X would be wrong
        assert slot_kinds(res[1]) == [(2, M)] and slot_kinds(res[2]) == [(1, M)] and slot_kinds(res[3]) == [(2, Tl)]
    add("foreign Map", [(MAIN, ["X", P1, P2])], [("tiles", 0, 0, 1), ("plain", 0, 2, 1), ("tiles", 0, 1, 1), ("tiles", 0, 2, 1)], foreign_map)

    def foreign_none(res, fr):
        assert slot_kinds(res[1]) == [] and slot_kinds(res[2]) == [(1, Tl)]
    add("foreign call without a Map", [(MAIN, ["X", P1])], [("tiles", 0, 0, 1), ("plain", 0, 0, 1), ("tiles", 0, 1, 1)], foreign_none)

    def other_size(res, fr):
        assert slot_kinds(res[1]) == [(0, M)] and slot_kinds(res[2]) == [(1, M)] and slot_kinds(res[3]) == [(0, Tl)]
    add("another size", [(MAIN, ["X", P1]), (OTHER, ["X"])], [("tiles", 0, 0, 1), ("tiles", 1, 0, 1), ("tiles", 0, 1, 1), ("tiles", 0, 0, 1)], other_size)

    def batch_then_frame(res, fr):
        assert slot_kinds(res[0]) == [(0, M)] and slot_kinds(res[1]) == [(0, Tl)] and slot_kinds(res[2]) == [] and slot_kinds(res[3]) == [(0, Tl)]
    add("batch then frame", [(MAIN, ["X", P1])], [("tiles", 0, 0, 1), ("frame", 0, 1), ("frame", 0, 1), ("tiles", 0, 0, 1)], batch_then_frame)
    return out


N_LONG = PLAN_BS + 6
LONG_P = ("px", 100, 10)


def long_keys():
    """X and X with one pixel flipped in turn (a MapTiles message per frame), a closed frame and a Y on the way, X P X P over the
    plan's chunk edge."""
    keys = ["X" if i % 2 == 0 else LONG_P for i in range(N_LONG)]
    keys[300], keys[301], keys[700] = "closed", "closed", "Y"
    return keys


def _long_case():
    keys = long_keys()

    def check(res, fr):
        (r,) = res
        kinds = dict(slot_kinds(r))
        assert N_LONG > PLAN_BS and r["frames_done"] == N_LONG
        assert [kinds[f] for f in range(PLAN_BS - 2, PLAN_BS + 2)] == [T.MAP_TILES] * 4 and kinds[N_LONG - 1] == T.MAP_TILES   # on both sides of the chunk edge
        assert kinds[0] == W.MAP and kinds[700] == W.MAP and kinds[701] == W.MAP and 300 not in kinds and 301 not in kinds and kinds[302] == T.MAP_TILES
        assert r["n_maps"] == 3
    return Case("long", [(LONG, keys)], [], None, [("tiles", 0, 0, N_LONG)], check)


def _per_size():
    out = []
    for name, c in SIZES.items():
        out += [_corners_case(name, c), _alpha_case(name, c), _outside_case(name, c), _boundary_case(name, c)]
    return out


CASES = _per_size() + [_equal_case()] + _sequences() + _continuations() + [_long_case()]
CASE_NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
FRAME_CASES = [c.name for c in CASES if any(s[0] == "frame" for s in c.steps)]

# mutant (web_tiles_ref.feed_tiles' rule) -> the case that must tell it apart
MUTANTS = {
    "base_is_previous_frame": "seq/X closed closed Y",
    "kept_from_batch_end": "cont/cut keeps the stop",
    "le_for_lt": "1921x276/equal",
    "unpadded_tiles": "101x271/corners",
    "alpha_ignored": "101x271/alpha",
    "kept_trusted_after_foreign_map": "cont/foreign Map",
}


def mutant_is_told_apart(rule, gray):
    case = BY_NAME[MUTANTS[rule]]
    fr = ref_frames(case, gray)
    return run_reference(case, fr, rule) != run_reference(case, fr)


def replay(case, res, fr):
    """Every step's messages through the restatement's client: the texture after every open consumed frame is that frame's map."""
    tex = None
    for st, r in zip(case.steps, res):
        if r is None:
            continue
        b = st[1]
        for f, kind, crc, data in r["messages"]:
            if kind in (W.MAP, T.MAP_TILES):
                tex = T.apply_message(tex, data)
            if kind == W.MARKERS:                              # the frame's last message: the viewer now shows the frame's map
                pos = st[2] if st[0] == "frame" else f
                assert tex is not None and bytes(tex[2]) == fr[b][pos][2][2] and zlib.crc32(bytes(tex[2])) == crc, (case.name, st, f)
