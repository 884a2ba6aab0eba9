"""Inputs of the ballistic-clearance tests, shared by the host and the device tests.  Every case says what it is for and asserts, on the
restatement (ballistic_clearance_ref.py), that it shows it: a case that no longer holds its point fails on the CPU, before any device is
asked.  The heightmaps are tests/clearance_cases.py's (a case's minimap rectangle is (0, W, 0, H) of its W x H heightmap unless it says
otherwise, so at the identity viewport a map-ROI coordinate IS the heightmap coordinate and a texel is a metre), the weapons
tests/ballistics_cases.py's and a few made for their arithmetic.  `families` names the switches of ballistic_clearance_ref.MUTANTS a case
is there to tell from the rule: every case must tell every switch it names (tests/test_ballistic_clearance_host.py)."""
import collections
import dataclasses
import functools

import numpy as np

import ballistic_clearance_ref as R
import ballistics_cases as BC
import ballistics_ref as B
import clearance_cases as CC

TW, TH = CC.TW, CC.TH                                              # k_bclear_map's tile
KC = 32                                                            # SMH_CLEAR_KC: samples staged at a time
SAMPLES = (1, 2, 32, 33, 34, 64, 65, 66, 256)                      # both sides of KC interior samples and of the lines kernel's 64 lanes

MORTAR = BC.MORTAR
MORTAR_LOW = dataclasses.replace(BC.MORTAR, arc=B.LOW)             # the mortar's velocity laid on the low arc
ROCKET = BC.ROCKET                                                 # low arc, 5 .. 40 degrees, 300 m minimum range
ROCKET_HIGH = dataclasses.replace(BC.ROCKET, arc=B.HIGH)           # ... laid on the arc its mount cannot reach
# V = 32, g = 8: V^2 = 2^10 and V^4 = 2^20 exactly, so the discriminant of (128, 0) is exactly 0, both roots are 1 and the arc over
# flat ground is x - x * x / 128: exact in f64 at every sample of a power-of-two S
EXACT = B.Weapon(velocity=32.0, gravity=8.0, arc=B.HIGH, unit=B.DEGREES, elev_min=0.0, elev_max=90.0)
# a lob of 25 m/s for the random terrain, whose 48 x 64 texels are 64 m across
LOB_LOW = dataclasses.replace(BC.SHORT, velocity=25.0, arc=B.LOW, elev_max=80.0)
# a short thrower laid on the high arc up to 80 degrees: at a metre a texel its whole reach (163 m) lies inside the dense cases' maps
THROWER = dataclasses.replace(BC.SHORT, arc=B.HIGH, elev_max=80.0)
THROWER_LOW = dataclasses.replace(THROWER, arc=B.LOW)

LineCase = collections.namedtuple("LineCase", "name families weapon hm minimap lines samples margin viewport fit check")
MapCase = collections.namedtuple("MapCase", "name families weapon hm minimap origin window samples margin viewport fit show")


@functools.lru_cache(maxsize=None)
def level_map():
    """512 x 8, level: a power of two wide, so the heightmap coordinate of a whole map-ROI coordinate is exact."""
    return CC._hm(np.full((8, 512), 1234), 40.0)


@functools.lru_cache(maxsize=None)
def cliff_map():
    """300 x 16: a plateau of 400 m up to column 99, ground at 0 from column 100 on."""
    z = np.zeros((16, 300))
    z[:, :100] = 400.0
    return CC._hm(CC._metres(z, 400.0), 400.0)


def restate_lines(c, mut=(), samples=None, margin=None, weapon=None):
    return R.lines(weapon or c.weapon, c.lines, c.samples if samples is None else samples, c.margin if margin is None else margin, c.minimap, c.hm, c.fit,
                   c.viewport, mut)


def restate_map(c, mut=()):
    return R.clearance_map(c.weapon, c.origin, c.window, c.samples, c.margin, c.viewport, c.minimap, c.hm, c.fit, mut)


# ---- what the line cases are for
def _st(d):
    return [a["status"] for a in d["arc"]]


def _check_low_blocked_high_clear(c, recs):
    """At the wall (780 m of 800) the low arc is about 7 m up and the high arc about 53 m up; the wall is 30 m."""
    (a, b), = recs
    k = B.rule(c.weapon)
    disc, gm, t_hi, t_lo = B.roots(k, 800.0, 0.0)
    assert 6.0 < R.arc_height(k, 800.0, t_lo, 780.0) < 8.0 and 52.0 < R.arc_height(k, 800.0, t_hi, 780.0) < 54.0
    for d in (a, b):
        assert _st(d) == [R.S_CLEAR, R.S_BLOCKED] and [x["bal"] for x in d["arc"]] == [0, 0], d
        assert d["arc"][B.LOW]["n_blocked"] == 1 and d["arc"][B.LOW]["min_margin"] < 0.0 < d["arc"][B.HIGH]["min_margin"]
        assert d["choice"] == 1 + B.HIGH                            # laid low: switch to the high arc; laid high: stay on it
    assert a["arc"][B.LOW]["first_blocked"] == c.samples * 780 // 800 and b["arc"][B.LOW]["first_blocked"] == c.samples * 20 // 800


def _check_low_blocked_high_unusable(c, recs):
    (a, b), = recs
    k = B.rule(c.weapon)
    disc, gm, t_hi, t_lo = B.roots(k, 800.0, 0.0)
    assert 19.7 < R.arc_height(k, 800.0, t_lo, 400.0) < 19.9        # 19.8 m under a 30 m hill
    for d in (a, b):
        assert _st(d) == [R.S_CLEAR, R.S_BLOCKED] and [x["bal"] for x in d["arc"]] == [B.ELEV_HIGH, 0], d
        assert d["choice"] == 0 and d["los_blocked"] > 0 and d["arc"][B.HIGH]["min_margin"] > 0.0


def _check_switch(c, recs):
    (a, b), = recs
    for d in (a, b):
        assert _st(d) == [R.S_CLEAR, R.S_CLEAR] and [x["bal"] for x in d["arc"]] == [B.ELEV_HIGH, 0] and d["choice"] == 1 + B.LOW, d


def _check_unusable_blocked(c, recs):
    """200 m, under the rocket's minimum range: both arcs unusable, and the low one runs into the hill all the same."""
    (a, b), = recs
    for d in (a, b):
        assert _st(d) == [R.S_CLEAR, R.S_BLOCKED] and all(x["bal"] & B.BELOW_MIN_RANGE for x in d["arc"]) and d["choice"] == 0, d
        assert d["arc"][B.LOW]["n_blocked"] > 1 and d["arc"][B.LOW]["min_margin"] < -20.0


def _check_disc_zero(c, recs):
    (a, b), = recs
    for d in (a, b):
        assert d["meters"] == 128.0 and d["alt_delta"] == 0.0 and d["arc"][B.HIGH] == d["arc"][B.LOW], d
        assert _st(d) == [R.S_CLEAR, R.S_CLEAR] and d["choice"] == 1 and d["arc"][0]["bal"] == 0
    k = B.rule(c.weapon)
    disc, gm, t_hi, t_lo = B.roots(k, 128.0, 0.0)
    assert disc == 0.0 and t_hi == t_lo == 1.0


def _check_ties(c, recs):
    """x - x * x / 128 is exact and symmetric about the middle: samples k and S - k tie bit for bit, and the lowest k wins."""
    _check_disc_zero(c, recs)
    k, S = B.rule(c.weapon), c.samples
    m = [float(R.arc_height(k, 128.0, 1.0, 128.0 * j / S)) for j in range(1, S)]
    assert all(m[j] == m[S - 2 - j] for j in range(S - 1)) and min(m) == m[0] == m[-1]
    for d in recs[0]:
        assert d["arc"][0]["min_at"] == 1 and d["arc"][0]["min_margin"] == m[0] and d["arc"][0]["min_margin"] == 128.0 / S - (128.0 / S) ** 2 / 128.0


def _check_far_below(c, recs):
    (a, b), = recs
    k = B.rule(c.weapon)
    disc, gm, t_hi, t_lo = B.roots(k, a["meters"], a["alt_delta"])
    assert a["alt_delta"] == -400.0 and t_lo < 0.0 < t_hi          # the low arc only falls
    assert _st(a) == [R.S_CLEAR, R.S_CLEAR] and a["arc"][B.LOW]["min_margin"] > 0.0, a
    assert a["arc"][B.LOW]["bal"] == B.ELEV_LOW and a["arc"][B.HIGH]["bal"] == 0 and a["choice"] == 1 + B.HIGH   # (the mount starts at 0 mils)
    assert b["alt_delta"] == 400.0 and _st(b) == [R.S_CLEAR, R.S_CLEAR]


def _check_no_arc(c, recs):
    (a, b), (n0, n1) = recs
    for d in (a, b):
        assert _st(d) == [R.S_OUT_OF_RANGE] * 2 and all(x["bal"] & B.OUT_OF_RANGE for x in d["arc"]) and d["choice"] == 0
        assert all(x["n_blocked"] == 0 and x["first_blocked"] == c.samples and x["min_margin"] == 0.0 and x["min_at"] == 0 for x in d["arc"])
    assert a["los_blocked"] > 0                                    # the sight line is still judged
    assert _st(n0)[B.HIGH] == R.S_CLEAR and n0["arc"][B.HIGH]["min_margin"] > 0.0   # 1,230 m on the same ground is in range


def _check_zero_length(c, recs):
    for pair in recs:
        for d in pair:
            assert d["meters"] == 0.0 and d["los_blocked"] == 0 and _st(d) == [R.S_CLEAR] * 2, d
            assert all(x["n_blocked"] == 0 and x["first_blocked"] == c.samples and x["min_margin"] == 0.0 and x["min_at"] == 0 for x in d["arc"])


def _check_one_sample(c, recs):
    assert c.samples == 1
    for d in recs[0]:
        assert _st(d) == [R.S_CLEAR] * 2 and d["los_blocked"] == 0 and d["meters"] == 800.0
        assert all(x["n_blocked"] == 0 and x["first_blocked"] == 1 and x["min_margin"] == 0.0 and x["min_at"] == 0 for x in d["arc"])


def _check_no_verdict(c, recs):
    assert len(recs) >= 1 and all(pair == (None, None) for pair in recs)


def _check_margin(c, recs):
    """The margin is above the low arc's least clearance and below the high arc's: it turns the low arc's CLEAR into BLOCKED."""
    free = restate_lines(c, margin=0.0)
    lo, hi = free[0][0]["arc"][B.LOW], free[0][0]["arc"][B.HIGH]
    assert _st(free[0][0]) == [R.S_CLEAR] * 2 and 0.0 < lo["min_margin"] < c.margin < hi["min_margin"]
    assert _st(recs[0][0]) == [R.S_CLEAR, R.S_BLOCKED] and recs[0][0]["arc"][B.LOW]["min_margin"] == lo["min_margin"]


def _check_equal_margin(c, recs):
    """margin_m is the restatement's own least m of the low arc: m == margin_m does not block; one ulp more does."""
    free = restate_lines(c, margin=0.0)
    m, k = free[0][0]["arc"][B.LOW]["min_margin"], free[0][0]["arc"][B.LOW]["min_at"]
    a = recs[0][0]["arc"][B.LOW]
    assert c.margin == m > 0.0 and a["status"] == R.S_CLEAR and a["n_blocked"] == 0 and a["min_margin"] == m and a["min_at"] == k
    more = restate_lines(c, margin=float(np.nextafter(m, np.inf)))[0][0]["arc"][B.LOW]
    assert more["status"] == R.S_BLOCKED and more["first_blocked"] == k and more["n_blocked"] == 1


def _check_mixed(c, recs):
    seen = set(s for pair in recs if pair[0] is not None for d in pair for s in _st(d))
    assert seen == {R.S_OUT_OF_RANGE, R.S_CLEAR, R.S_BLOCKED}, seen
    chosen = {d["choice"] for pair in recs if pair[0] is not None for d in pair}
    assert any(pair[0] is None for pair in recs) and 0 in chosen and (1 in chosen or c.samples > 66)   # (at S = 256 the 2.5 m margin blocks every line)
    assert any(d["arc"][a]["bal"] and d["arc"][a]["status"] == R.S_BLOCKED for pair in recs if pair[0] is not None for d in pair for a in (0, 1))


def _equal_margin_case():
    base = LineCase("m == margin_m", ("margin_le",), MORTAR_LOW, CC.ramp_map(), CC.whole(CC.ramp_map()), [(10.0, 20.0, 180.0, 22.0)], 64, 0.0, None, True, _check_equal_margin)
    return base._replace(margin=restate_lines(base)[0][0]["arc"][B.LOW]["min_margin"])


@functools.lru_cache(maxsize=None)
def line_cases():
    out = []
    flat, hill, wall30, lng, cliff, level = CC.flat_map(), CC.hill_map(), CC.hill_with_wall(30.0), CC.long_map(), cliff_map(), level_map()
    line800 = [(10.0, 30.0, 810.0, 30.0)]
    for w, nm in ((MORTAR_LOW, "laid low"), (MORTAR, "laid high")):
        out.append(LineCase("low blocked, high clear, " + nm, ("swap_arcs", "qq1_other"), w, wall30, CC.whole(wall30), line800, 80, 0.0, None, True, _check_low_blocked_high_clear))
    out.append(LineCase("low blocked, high unusable", ("choice_no_bal",), ROCKET, hill, CC.whole(hill), line800, 64, 0.0, None, True, _check_low_blocked_high_unusable))
    out.append(LineCase("high unusable, low clear", ("choice_no_bal",), ROCKET_HIGH, flat, CC.whole(flat), line800, 64, 0.0, None, True, _check_switch))
    out.append(LineCase("unusable and blocked", ("skip_unusable",), ROCKET, hill, CC.whole(hill), [(300.0, 30.0, 500.0, 30.0)], 64, 0.0, None, True, _check_unusable_blocked))
    out.append(LineCase("disc == 0.0", (), EXACT, level, CC.whole(level), [(100.0, 4.0, 228.0, 4.0)], 33, 0.0, None, True, _check_disc_zero))
    for S in (64, 256):
        out.append(LineCase("ties of m, S = %d" % S, (), EXACT, level, CC.whole(level), [(100.0, 4.0, 228.0, 4.0)], S, 0.0, None, True, _check_ties))
    out.append(LineCase("target far below", (), MORTAR_LOW, cliff, CC.whole(cliff), [(99.0, 8.0, 299.0, 8.0)], 64, 0.0, None, True, _check_far_below))
    out.append(LineCase("no arc", (), MORTAR, lng, CC.whole(lng), [(20.0, 4.0, 1320.0, 4.0), (20.0, 4.0, 1250.0, 4.0)], 64, 0.0, None, True, _check_no_arc))
    for hm in (CC.one_texel(), CC.three_by_two(), flat):
        h, w = hm[0].shape
        out.append(LineCase("d == 0, %d x %d" % (w, h), (), ROCKET, hm, CC.whole(hm), [(w / 2.0 - 0.25, h / 2.0 - 0.25, w / 2.0 - 0.25, h / 2.0 - 0.25)] * 2, 64, 0.0, None, True,
                            _check_zero_length))
    out.append(LineCase("S == 1", (), MORTAR_LOW, wall30, CC.whole(wall30), line800, 1, 0.0, None, True, _check_one_sample))
    out.append(LineCase("an end outside", (), MORTAR, hill, CC.whole(hill), [(-1.0, 5.0, 50.0, 5.0), (20.0, 5.0, 900.0, 5.0), (20.0, 64.0, 30.0, 5.0), (20.0, 5.0, 30.0, -0.6)],
                        64, 0.0, None, True, _check_no_verdict))
    out.append(LineCase("the scales branch: no rectangle", (), MORTAR, hill, None, line800, 64, 0.0, None, True, _check_no_verdict))
    out.append(LineCase("the scales branch: no heightmap", (), MORTAR, None, CC.whole(hill), line800, 64, 0.0, None, True, _check_no_verdict))
    out.append(LineCase("a margin of 10 m", (), MORTAR_LOW, flat, CC.whole(flat), line800, 80, 10.0, None, True, _check_margin))
    out.append(_equal_margin_case())
    # 32 lines over the dense cases' country, its rectangle zoomed and panned with a scale per axis and the bounds offset on: ends in and
    # outside the map, on the mesa and behind the walls; at every S on one side and the other of the kernels' strides
    rng = np.random.default_rng(5)
    land = CC.country_map_offset()
    pts = np.concatenate([rng.uniform(-2.0, 140.0, size=(32, 1)), rng.uniform(0.0, 72.0, size=(32, 1)), rng.uniform(-2.0, 140.0, size=(32, 1)),
                          rng.uniform(0.0, 72.0, size=(32, 1))], axis=1).astype(np.float32)
    pts[0] = (60.0, 20.0, 20.0, 48.0)                              # onto the mesa from the plain
    for S in SAMPLES:
        out.append(LineCase("32 lines, S = %d" % S, ("swap_arcs", "qq1_other", "skip_unusable", "choice_no_bal") if S >= 2 else ("swap_arcs", "choice_no_bal"), THROWER, land, (10, 202, 5, 53),
                            [tuple(float(v) for v in p) for p in pts], S, 2.5, (1.5, 0.75, 1.0, 2.0), False, _check_mixed if S >= 64 else (lambda c, r: None)))
    return out


_LINES = {}


def checked_lines(c):
    """The case's restatement, after the case's own check (computed once: the host and the device tests share it)."""
    if c.name not in _LINES:
        recs = restate_lines(c)
        c.check(c, recs)
        _LINES[c.name] = recs
    return _LINES[c.name]


# ---- the dense cases
ALL = tuple("own%d" % c for c in (1, 2, 3, 4)) + tuple("oth%d" % c for c in (1, 2, 3, 4)) + ("los", "switch")


ABSENT = {"low blocked, high unusable: no switch": ("switch", "own3", "oth3")}


def features(r):
    """-> {feature: (pixels, tiles it occurs in, it occurs in two tiles that share an edge)} of a restated window."""
    own, oth, los, sw = R.split(r["bytes"])
    h, w = own.shape
    ty, tx = np.mgrid[0:h, 0:w]
    masks = [("own%d" % c, own == c) for c in (1, 2, 3, 4)] + [("oth%d" % c, oth == c) for c in (1, 2, 3, 4)] + [("los", los), ("switch", sw)]
    out = {}
    for nm, m in masks:
        tiles = set(zip((ty[m] // TH).tolist(), (tx[m] // TW).tolist()))
        out[nm] = (int(m.sum()), len(tiles), any((a + 1, b) in tiles or (a, b + 1) in tiles for a, b in tiles))
    return out


def check_map(c, r):
    """Every feature the case is meant to show occurs inside the window in two tiles that share an edge: on both sides of a tile edge, at
    65 x 17 therefore in the one-pixel remainder column or row as well.  A case that shows nothing has no verdict anywhere.  The margin plane
    is a number exactly where the own class is CLEAR or BLOCKED."""
    f = features(r)
    for what in c.show:
        assert f[what][0] >= 1 and f[what][2], (c.name, what, f)
    for what in ABSENT.get(c.name, ()):
        assert f[what][0] == 0, (c.name, what, f)
    if not c.show:
        assert not r["bytes"].any() and np.isnan(r["margin"]).all(), c.name
    own = r["bytes"] & 7
    assert np.array_equal(~np.isnan(r["margin"]), (own == R.C_CLEAR) | (own == R.C_BLOCKED)) and not (r["bytes"] & 0x40).any(), c.name
    assert ((r["bytes"] != 0) | ((r["bytes"] & R.C_LOS) == 0)).all()


@functools.lru_cache(maxsize=None)
def map_cases():
    out = []
    land, rnd, hill, flat = CC.country_map(), CC.random_map(), CC.hill_map(), CC.flat_map()
    rect = (6, 134, 4, 68)                                         # the 257 x 129 map over 128 x 64 map-ROI pixels: two texels a pixel
    fam = ("swap_arcs", "qq1_other", "class_precedence", "los_not_oor")   # (a pixel's m never equals the margin exactly: margin_le is the lines')
    # a scale per axis; at 130 x 33 a margin outside the rectangle on every side
    out.append(MapCase("country, 130 x 33, a scale per axis", fam, THROWER, land, rect, (62.3, 22.4), (130, 33), 64, 0.0, (130 / 140.0, 33 / 72.0, 0.0, 0.0), True, ALL))
    # at 65 x 17 the second tiles are the remainder column x = 64 and the remainder row y = 16: viewports and origins found by search, so
    # that the rectangle covers both and every class of both arcs, the LOS bit and a switch pixel lie in them as well as in the full tile
    out.append(MapCase("country, 65 x 17, a scale per axis", fam, THROWER, land, rect, (68.2, 64.8), (65, 17), 64, 0.0, (0.541, 0.293, -8.02, -1.15), True, ALL))
    out.append(MapCase("country, 130 x 33, identity", fam, THROWER, land, rect, (62.3, 22.4), (130, 33), 64, 0.0, None, True, ALL))
    out.append(MapCase("country, 65 x 17, laid low, bounds offset", fam, THROWER_LOW, CC.country_map_offset(), rect, (43.7, 53.0), (65, 17), 66, 0.0,
                       (0.783, 0.477, -32.69, -10.43), False, ALL))
    view = (130 / 140.0, 33 / 72.0, -11.5, 3.25)                   # panned: the window's left and top lie inside, right and bottom outside
    for S in SAMPLES:
        out.append(MapCase("country, 130 x 33 panned, S = %d" % S, fam if S >= 2 else ("swap_arcs",), THROWER, land, rect, (62.3, 22.4), (130, 33), S, 0.0, view, True,
                           ALL if S >= 2 else ("own1", "oth1", "own2", "oth2", "own3", "oth3", "switch")))   # (S = 1 has no sample to block anything)
    out.append(MapCase("random terrain, 65 x 17", fam, LOB_LOW, rnd, (8, 56, 4, 40), (45.4, 17.2), (65, 17), 65, 0.0, (1.623, 0.537, -11.15, -3.86), True, ALL))
    out.append(MapCase("random terrain, 130 x 33", fam, LOB_LOW, rnd, (8, 56, 4, 40), (20.0, 11.0), (130, 33), 65, 0.0, (2.0, 0.8, 0.0, 0.0), True, ALL))
    # the issue's two named answers as maps: the rocket's low arc under the hill with its high arc beyond the mount -- no switch pixel there --
    # and the same weapon laid high over flat ground -- every pixel in reach a switch pixel
    out.append(MapCase("low blocked, high unusable: no switch", ("swap_arcs", "class_precedence"), ROCKET, hill, (0, 90, 0, 7), (1.0, 3.5), (130, 33), 64, 0.0, (1.4, 4.0, 0.0, 0.0), True,
                       ("own4", "own2", "oth2", "los")))
    out.append(MapCase("high unusable, low clear: a switch", (), ROCKET_HIGH, flat, (0, 90, 0, 7), (1.0, 3.5), (130, 33), 64, 0.0, (1.4, 4.0, 0.0, 0.0), True,
                       ("own2", "oth3", "oth2", "switch")))
    out.append(MapCase("origin outside its rectangle", (), THROWER, land, rect, (3.0, 30.0), (65, 17), 64, 0.0, (65 / 140.0, 17 / 72.0, 0.0, 0.0), True, ()))
    out.append(MapCase("no rectangle", (), THROWER, land, None, (62.3, 22.4), (65, 17), 64, 0.0, None, True, ()))
    return out


_MAPS = {}


def checked_map(c):
    """The case's restatement, after the case's own check (computed once: the host and the device tests share it)."""
    if c.name not in _MAPS:
        r = restate_map(c)
        check_map(c, r)
        _MAPS[c.name] = r
    return _MAPS[c.name]
