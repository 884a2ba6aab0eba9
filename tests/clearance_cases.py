"""Inputs of the terrain-clearance tests, shared by the host and the device tests.  Every case says what it is for and asserts, on the
restatement (clearance_ref.py), that it shows it: a case that no longer holds its point fails on the CPU, before any device is asked.

The geometry is kept readable: a case's minimap rectangle is (0, W, 0, H) of its W x H heightmap unless it says otherwise, so at the
identity viewport a map-ROI coordinate IS the heightmap coordinate, and a texel is a metre."""
import collections
import functools

import numpy as np

import clearance_ref as R

TW, TH = 64, 16                                                   # k_clear_map's tile (csrc/smh_kernels.h, SMH_REACH_TW / SMH_REACH_TH)
SAMPLES = (1, 2, 63, 64, 65, 128, 256)

LineCase = collections.namedtuple("LineCase", "name hm minimap lines samples margin viewport fit check")
MapCase = collections.namedtuple("MapCase", "name hm minimap origin window samples margin viewport fit show")


def _metres(z, zs):
    """Heights in metres -> u16 texels of a heightmap whose full scale is zs metres (scale[2] = zs * 0.1953125)."""
    return np.clip(np.rint(np.asarray(z, np.float64) / zs * 65535.0), 0, 65535).astype(np.uint16)


def _hm(data, zs, bounds=((0, 0), (0, 0))):
    return np.ascontiguousarray(data, np.uint16), bounds, (1.0, 1.0, zs * 0.1953125)


def whole(hm):
    h, w = hm[0].shape
    return (0, w, 0, h)


@functools.lru_cache(maxsize=None)
def one_texel():
    return _hm(np.array([[40000]]), 100.0)


@functools.lru_cache(maxsize=None)
def three_by_two():
    return _hm(np.array([[0, 65535, 100], [30000, 5, 65535]]), 50.0)


@functools.lru_cache(maxsize=None)
def wall_map():
    """257 x 129: ground at 5 m, a plateau of 450 m from column 119 on, and at its edge a wall of full height (480 m), one texel thick,
    at column 118 -- two texels before the target column 120 of the wall line.  Fired UP at the plateau a shell comes down at a
    shallower angle than it leaves at when fired from it: 1.6 m before the target the arc from below is 15 m under the wall's top, the
    arc from above 14 m over it."""
    z = np.full((129, 257), 5.0)
    z[:, 119:] = 450.0
    z[:, 118] = 480.0
    return _hm(_metres(z, 480.0), 480.0)


@functools.lru_cache(maxsize=None)
def ramp_map():
    """200 x 40: a ramp of 0.4 m per texel along x, with a ripple across it."""
    y, x = np.mgrid[0:40, 0:200]
    return _hm(_metres(0.4 * x + 2.0 * np.sin(y / 3.0) + 2.0, 120.0), 120.0)


@functools.lru_cache(maxsize=None)
def flat_map():
    return _hm(np.full((64, 900), 1234), 40.0)


@functools.lru_cache(maxsize=None)
def hill_map():
    """Level ground with a hill of 30 m across columns 390 .. 410: the 800 m line's sight line meets it, its arc is far above."""
    return hill_with_wall(0.0)


@functools.lru_cache(maxsize=None)
def hill_with_wall(wall_m):
    """... and a wall of wall_m metres at column 790, 780 m along the 800 m line from column 10 and 20 m before its target."""
    z = np.zeros((64, 900))
    z[:, 390:411] = 30.0
    z[:, 790] = wall_m
    return _hm(_metres(z, 100.0), 100.0)


@functools.lru_cache(maxsize=None)
def long_map():
    """1400 x 8, gentle: long enough for a line beyond the 1,237 m a tube reaches."""
    y, x = np.mgrid[0:8, 0:1400]
    return _hm(_metres(10.0 + 8.0 * np.sin(x / 70.0) + y, 50.0), 50.0)


@functools.lru_cache(maxsize=None)
def random_map():
    rng = np.random.default_rng(11)
    return np.ascontiguousarray(rng.integers(0, 65536, size=(48, 64)).astype(np.uint16)), ((7, -5), (0, 0)), (1.0, 1.0, 200.0 * 0.1953125)


@functools.lru_cache(maxsize=None)
def country_map():
    """257 x 129 for the dense cases: rolling ground of a few metres (clear), a belt of walls every 7 columns on the right (blocked right
    behind each wall), a mesa of 700 m in the lower left corner (out of range by altitude: a tube climbs 616 m at most) and a ridge
    across the middle rows (sight lines over it are blocked, arcs are not)."""
    y, x = np.mgrid[0:129, 0:257]
    z = 20.0 + 6.0 * np.sin(x / 17.0) * np.cos(y / 11.0)
    z[60:64, :150] += 25.0
    belt = (x >= 150) & (x % 7 < 2)
    z[belt] = 140.0
    z[100:, :40] = 700.0
    return _hm(_metres(z, 800.0), 800.0)


def restate_lines(c, samples=None, margin=None):
    return R.lines(c.lines, c.samples if samples is None else samples, c.margin if margin is None else margin, c.minimap, c.hm, c.fit, c.viewport)


def restate_map(c, samples=None):
    return R.clearance_map(c.origin, c.window, c.samples if samples is None else samples, c.margin, c.viewport, c.minimap, c.hm, c.fit)


# ---- what the line cases are for
def _statuses(recs):
    return [(a["status"], b["status"]) for a, b in recs]


def _check_none(c, recs, prof):
    assert recs == [] and prof.shape == (0, R.PROFILE)


def _check_one_clear(c, recs, prof):
    (a, b), = recs
    assert a["status"] == b["status"] == R.CLEAR and a["n_blocked"] == 0 and a["first_blocked"] == c.samples and a["los_blocked"] == 0
    assert a["min_margin"] > 0.0 and 1 <= a["min_at"] < c.samples and (prof[0, :c.samples + 1] > 0).all() and not prof[0, c.samples + 1:].any()


def _check_mixed(c, recs, prof):
    seen = set(s for pair in _statuses(recs) for s in pair)
    assert seen == {R.NONE, R.OUT_OF_RANGE, R.CLEAR, R.BLOCKED}, seen
    assert len(recs) == 32 and any(a["status"] != b["status"] for a, b in recs)


def _check_zero_length(c, recs, prof):
    for a, b in recs:
        for d in (a, b):
            assert d == dict(status=R.CLEAR, first_blocked=c.samples, n_blocked=0, los_blocked=0, min_margin=0.0, min_at=0), d
    assert (prof[:, :c.samples + 1] > 0).all()                    # the profile is the one texel, S + 1 times


def _check_outside(c, recs, prof):
    assert _statuses(recs) == [(R.NONE, R.NONE)] * len(recs) and len(recs) >= 4 and not prof.any()


def _check_out_of_range(c, recs, prof):
    (a, b), (n0, n1) = recs
    for d in (a, b):
        assert d["status"] == R.OUT_OF_RANGE and d["n_blocked"] == 0 and d["first_blocked"] == c.samples and d["min_margin"] == 0.0 and d["min_at"] == 0
    assert a["los_blocked"] > 0 and prof[0, :c.samples + 1].all()  # the sight line is still judged, the profile still written
    assert n0["status"] == R.CLEAR and n0["min_margin"] > 0.0      # 1,230 m on the same ground is in range


def _check_wall(c, recs, prof):
    (a, b), = recs
    if c.samples < 63:                                             # too few samples to meet a wall one texel thick: that is the point of S
        assert a["status"] == b["status"] == R.CLEAR
        return
    assert a["status"] == R.BLOCKED and b["status"] == R.CLEAR, (a, b)
    assert 1 <= a["n_blocked"] <= 3 and a["min_margin"] < 0.0 and b["n_blocked"] == 0 and b["min_margin"] > 0.0
    # the blocking sample lies on the wall: column 118, two texels before the target's column 120
    k, S = a["first_blocked"], c.samples
    assert round(20.0 + 100.0 * k / S) == 118 and prof[0, k] == np.float32(480.0)


def _check_equal_margin(c, recs, prof):
    """margin_m is the restatement's own least m: at that sample m == margin_m, which does not block; one ulp more does."""
    (a, b), = recs
    free, _ = restate_lines(c, margin=0.0)
    m, k = free[0][0]["min_margin"], free[0][0]["min_at"]
    assert c.margin == m > 0.0 and a["status"] == R.CLEAR and a["n_blocked"] == 0 and a["min_margin"] == m and a["min_at"] == k
    more, _ = restate_lines(c, margin=float(np.nextafter(m, np.inf)))
    assert more[0][0]["status"] == R.BLOCKED and more[0][0]["first_blocked"] == k and more[0][0]["n_blocked"] == 1


def _check_los_only(c, recs, prof):
    (a, b), = recs
    for d in (a, b):
        assert d["status"] == R.CLEAR and d["n_blocked"] == 0 and d["los_blocked"] >= 1 and d["min_margin"] > 0.0, d


def _fail(what):
    raise AssertionError(what)


def _equal_margin_case():
    base = LineCase("m == margin_m", ramp_map(), whole(ramp_map()), [(10.0, 20.0, 180.0, 22.0)], 64, 0.0, None, True, _check_equal_margin)
    recs, _ = restate_lines(base)
    return base._replace(margin=recs[0][0]["min_margin"])


@functools.lru_cache(maxsize=None)
def line_cases():
    out = []
    rng = np.random.default_rng(5)
    flat, wall, rnd, lng = flat_map(), wall_map(), random_map(), long_map()
    out.append(LineCase("no lines", flat, whole(flat), [], 64, 0.0, None, True, _check_none))
    out.append(LineCase("one line, flat", flat, whole(flat), [(10.0, 30.0, 810.0, 30.0)], 64, 0.0, None, True, _check_one_clear))
    # 32 lines over the dense cases' country, its rectangle zoomed and panned with a scale per axis and the bounds offset on: ends in
    # and outside the map, on the mesa (out of range by altitude) and behind the walls
    land = country_map_offset()
    pts = np.concatenate([rng.uniform(-2.0, 140.0, size=(32, 1)), rng.uniform(0.0, 72.0, size=(32, 1)), rng.uniform(-2.0, 140.0, size=(32, 1)),
                          rng.uniform(0.0, 72.0, size=(32, 1))], axis=1).astype(np.float32)
    pts[0] = (60.0, 20.0, 20.0, 48.0)                              # onto the mesa from the plain
    for S in SAMPLES:
        out.append(LineCase("32 lines, S = %d" % S, land, (10, 202, 5, 53), [tuple(float(v) for v in p) for p in pts], S, 2.5, (1.5, 0.75, 1.0, 2.0), False,
                            _check_mixed if S >= 63 else (lambda c, r, p: None)))
    for hm in (one_texel(), three_by_two(), flat):
        h, w = hm[0].shape
        out.append(LineCase("zero length, %d x %d" % (w, h), hm, whole(hm), [(w / 2.0 - 0.25, h / 2.0 - 0.25, w / 2.0 - 0.25, h / 2.0 - 0.25)] * 2, 64, 0.0, None, True, _check_zero_length))
    out.append(LineCase("an end outside", wall, whole(wall), [(-1.0, 5.0, 50.0, 5.0), (20.0, 5.0, 257.0, 5.0), (20.0, 129.0, 30.0, 5.0), (20.0, 5.0, 30.0, -0.6)],
                        64, 0.0, None, True, _check_outside))
    # a NaN rounds to 0 `as i32`, which lies inside: the heightmap branch with a range that is NaN, as the firing solutions have it
    out.append(LineCase("a NaN end", wall, whole(wall), [(float("nan"), 5.0, 30.0, 5.0)], 64, 0.0, None, True,
                        lambda c, r, p: _statuses(r) == [(R.OUT_OF_RANGE, R.OUT_OF_RANGE)] or _fail(r)))
    out.append(LineCase("no rectangle", wall, None, [(20.0, 64.0, 120.0, 64.0)] * 4, 64, 0.0, None, True, _check_outside))
    out.append(LineCase("no heightmap", None, whole(wall), [(20.0, 64.0, 120.0, 64.0)] * 4, 64, 0.0, None, True, _check_outside))
    out.append(LineCase("out of range", lng, whole(lng), [(20.0, 4.0, 1320.0, 4.0), (20.0, 4.0, 1250.0, 4.0)], 64, 0.0, None, True, _check_out_of_range))
    for S in SAMPLES:
        out.append(LineCase("wall, S = %d" % S, wall, whole(wall), [(20.0, 64.0, 120.0, 64.0)], S, 0.0, None, True, _check_wall))
    out.append(_equal_margin_case())
    out.append(LineCase("sight line blocked, arc clear", hill_map(), whole(hill_map()), [(10.0, 30.0, 810.0, 30.0)], 64, 0.0, None, True, _check_los_only))
    return out


def checked_lines(c):
    recs, prof = restate_lines(c)
    c.check(c, recs, prof)
    return recs, prof


# ---- the dense cases
ALL = ("clear", "blocked", "none", "out_of_range", "los")


def share(r):
    b = r["bytes"]
    s = b & 0x7F
    return dict(none=float((s == R.NONE).mean()), out_of_range=float((s == R.OUT_OF_RANGE).mean()), clear=float((s == R.CLEAR).mean()),
                blocked=float((s == R.BLOCKED).mean()), los=float(((b & R.LOS_BLOCKED) != 0).mean()))


def check_map(c, r):
    """At least 5 % of the window in each of CLEAR and BLOCKED, at least one pixel of the rest -- of what the case is meant to show."""
    sh, n = share(r), r["bytes"].size
    for what in c.show:
        need = 0.05 if what in ("clear", "blocked") else 1.0 / n
        assert sh[what] >= need - 1e-12, (c.name, what, sh)
    if not c.show:
        assert not r["bytes"].any() or c.window == (1, 1), c.name


@functools.lru_cache(maxsize=None)
def map_cases():
    out = []
    land = country_map()
    rect = (6, 134, 4, 68)                                         # the 257 x 129 map over 128 x 64 map-ROI pixels: two texels a pixel
    for w, h in ((1, 1), (64, 16), (65, 17), (130, 33), (200, 120)):
        # a scale per axis that brings map-ROI (0 .. 140, 0 .. 72) into the window: a margin outside the rectangle on every side
        view = (w / 140.0, h / 72.0, 0.0, 0.0) if (w, h) != (1, 1) else (0.01, 0.02, 0.4, 0.3)
        show = ALL if (w, h) != (1, 1) else ("clear",)
        out.append(MapCase("window %d x %d" % (w, h), land, rect, (62.3, 22.4), (w, h), 64, 0.0, view, True, show))
    view = (130 / 140.0, 33 / 72.0, -11.5, 3.25)                   # panned: the window's left and top lie inside, right and bottom outside
    for S in SAMPLES:
        out.append(MapCase("130 x 33 panned, S = %d" % S, land, rect, (62.3, 22.4), (130, 33), S, 0.0, view, True, ALL if S >= 63 else ("none", "out_of_range")))
    out.append(MapCase("a margin of 15 m, bounds offset", country_map_offset(), rect, (40.0, 30.0), (65, 17), 64, 15.0, (65 / 140.0, 17 / 72.0, 0.0, 0.0), False, ALL))
    rnd = random_map()
    out.append(MapCase("random terrain", rnd, (8, 56, 4, 40), (20.0, 11.0), (65, 33), 65, 0.0, (1.7, 0.95, -9.25, 2.5), True, ("clear", "blocked", "none", "los")))
    flat = flat_map()
    out.append(MapCase("flat: clear or out of range", flat, (0, 90, 0, 7), (3.5, 3.5), (130, 33), 64, 0.0, (1.4, 4.0, 0.0, 0.0), True, ("clear",)))
    lng = long_map()
    out.append(MapCase("out of range by distance", lng, (0, 140, 0, 8), (2.0, 4.0), (200, 17), 64, 0.0, (1.4, 2.0, 0.0, 0.0), True, ("clear", "out_of_range", "none", "los")))
    out.append(MapCase("origin outside the map", land, rect, (3.0, 30.0), (65, 17), 64, 0.0, (65 / 140.0, 17 / 72.0, 0.0, 0.0), True, ()))
    out.append(MapCase("no rectangle", land, None, (62.3, 22.4), (65, 17), 64, 0.0, None, True, ()))
    out.append(MapCase("NaN origin", land, rect, (float("nan"), 22.4), (65, 17), 64, 0.0, None, True, ()))
    for hm in (one_texel(), three_by_two()):
        h, w = hm[0].shape
        out.append(MapCase("%d x %d heightmap" % (w, h), hm, (10, 50, 4, 14), (30.0, 9.0), (64, 16), 64, 0.0, None, True, ("none",)))
    return out


@functools.lru_cache(maxsize=None)
def country_map_offset():
    data, _, scale = country_map()
    return data, ((9, -4), (0, 0)), scale


_MAPS = {}


def checked_map(c):
    """The case's restatement, after the case's own check (computed once: the host and the device tests share it)."""
    if c.name not in _MAPS:
        r = restate_map(c)
        check_map(c, r)
        _MAPS[c.name] = r
    return _MAPS[c.name]
