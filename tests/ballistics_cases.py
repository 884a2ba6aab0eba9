"""Inputs of the ballistics tests, shared by the host and the device tests.  Every case says what it is for and checks, on the
restatement (ballistics_ref.py), that it contains it: a case that no longer holds its decision boundary fails on the CPU.  The weapons
are made up and chosen for their arithmetic (powers of two where a discriminant has to vanish exactly); none is a game's.

Two kinds: a Point is one (weapon, meters, alt) for the solution rule (the host entry point, the stand-alone program and, where alt
== 0, k_ballistic_lines through the scales branch); a Map is one window for k_ballistic_map.  `families` names the rule switches of
ballistics_ref.MUTANTS a case is there to tell from the rule (FAMILY_OF)."""
import collections
import functools
import math

import numpy as np

import ballistics_ref as B
import firing_edge_cases as FE
import firing_ref as FR
import reach_cases as RC
import reach_ref as R

TW, TH = RC.TW, RC.TH
FAMILY_OF = dict(swap_arcs="arcs", mils6000="units", limit_gt="limit", no_min_range="range_min", iso_left="isochrone", tof_other_root="tof",
                 apex_no_clamp="below")
assert set(FAMILY_OF) == set(B.MUTANTS)

MORTAR = B.Weapon()
# a rocket laid on the low arc in degrees, with a minimum range and a cone; a heavy tube on the high arc in 6000 mils
ROCKET = B.Weapon(velocity=200.0, gravity=9.81, arc=B.LOW, unit=B.DEGREES, elev_min=5.0, elev_max=40.0, range_min=300.0, dispersion=0.01)
TUBE = B.Weapon(velocity=150.0, gravity=9.8, arc=B.HIGH, unit=B.MILS6000, elev_min=850.0, elev_max=1420.0, range_min=120.0, dispersion=0.002)
# V = 128, g = 8: V^2 = 2^14 and V^4 = 2^28 exactly, so the discriminant of (2048, 0) is exactly 0
BINARY = B.Weapon(velocity=128.0, gravity=8.0, arc=B.HIGH, unit=B.DEGREES, elev_min=0.0, elev_max=90.0)
# a short thrower on the low arc that may point downhill: at 3 m/px its whole reach lies inside the small windows
SHORT = B.Weapon(velocity=40.0, gravity=9.81, arc=B.LOW, unit=B.DEGREES, elev_min=-60.0, elev_max=45.0, range_min=20.0, dispersion=0.005)

Point = collections.namedtuple("Point", "name families weapon m alt check limits_apart")
Map = collections.namedtuple("Map", "name families weapon hm minimap mpx origin window viewport fit iso_s check")


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def _f(a):
    return float(np.asarray(a))


def _same(a, b):
    """Bit for bit; a NaN equals a NaN."""
    a, b = _f(a), _f(b)
    return (a != a and b != b) or np.array([a]).tobytes() == np.array([b]).tobytes()


def restate_point(p, mut=()):
    return B.solve(p.weapon, p.m, p.alt, mut)


def restate_map(c, mut=(), iso_s=None):
    return B.ballistic_map(c.weapon, c.origin, c.window, c.viewport, c.minimap, c.mpx, c.hm, c.fit, c.iso_s if iso_s is None else iso_s, mut)


def _own(p, s):
    """The arc the weapon is laid on."""
    return s["arc"][p.weapon.arc]


# ---- the default weapon is the firing solutions' mortar
def _check_tie(p, s):
    for alt, sol in ((p.alt, s), (-p.alt, B.solve(p.weapon, p.m, -p.alt))):
        assert _same(sol["arc"][B.HIGH]["elevation"], FR.calc(p.m, alt)), (p.name, alt)
        assert (int(sol["arc"][B.HIGH]["status"]) & B.OUT_OF_RANGE != 0) == math.isnan(FR.calc(p.m, alt))


def _tie_points():
    pairs = {}
    for case in FE.cases():
        for want, _ in FE.restate(case):
            if want["source"] != FR.NONE:
                m, a = float(want["meters"]), float(want["alt_delta"])
                pairs[(repr(m), repr(a))] = (m, a)                 # (by their text: a NaN is one pair)
    assert len(pairs) >= 20
    return [Point("tie %s %s" % key, ("units",), MORTAR, m, a, _check_tie, True) for key, (m, a) in sorted(pairs.items())]


# ---- disc == 0 and the f64 neighbours of its sign change
def _check_disc(kind):
    def check(p, s):
        k = B.rule(p.weapon)
        disc = _f(B.roots(k, p.m, p.alt)[0])
        hi, lo = s["arc"]
        if kind == 0:
            assert disc == 0.0 and int(hi["status"]) == 0
            assert all(_same(hi[f], lo[f]) for f in ("elevation", "tof", "apex", "fall", "along", "status", "band")), "both arcs are equal"
        elif kind < 0:
            assert 0.0 < disc < 1e-6 and int(hi["status"]) == 0 and _f(hi["elevation"]) > _f(lo["elevation"])
        else:
            assert disc < 0.0 and int(hi["status"]) & B.OUT_OF_RANGE and int(lo["status"]) & B.OUT_OF_RANGE
            assert all(math.isnan(_f(a[f])) for a in (hi, lo) for f in ("elevation", "tof", "apex", "fall", "along")) and int(hi["band"]) == 0
    return check


def _disc_points():
    return [Point("disc == 0", ("arcs",), BINARY, 2048.0, 0.0, _check_disc(0), True),
            Point("disc just above 0", ("arcs",), BINARY, down(2048.0), 0.0, _check_disc(-1), True),
            Point("disc just below 0", ("arcs",), BINARY, up(2048.0), 0.0, _check_disc(1), True)]


# ---- m at range_min and its f64 neighbours
def _check_range_min(below):
    def check(p, s):
        for a in s["arc"]:
            assert (int(a["status"]) & B.BELOW_MIN_RANGE != 0) == below and not int(a["status"]) & B.OUT_OF_RANGE
    return check


def _range_min_points():
    out = []
    for w, nm in ((ROCKET, "rocket"), (TUBE, "tube")):
        r = w.range_min
        out += [Point("%s: m == range_min" % nm, ("range_min",), w, r, 0.0, _check_range_min(False), True),
                Point("%s: m just below range_min" % nm, ("range_min",), w, down(r), 0.0, _check_range_min(True), True),
                Point("%s: m just above range_min" % nm, ("range_min",), w, up(r), 0.0, _check_range_min(False), True)]
    return out


# ---- T exactly at a threshold, and at both neighbours: found by search, alt == 0 first (those also run on the device)
def _root(k, m, alt, arc):
    disc = k["v4"] - k["g"] * (k["g"] * (m * m) + 2.0 * alt * k["v2"])
    if not disc >= 0.0:
        return math.nan
    s, gm = math.sqrt(disc), k["g"] * m
    return FR.fdiv(k["v2"] + s, gm) if arc == B.HIGH else FR.fdiv(k["v2"] - s, gm)


def _hit(k, t, alt, arc):
    """An m whose root is exactly t, with its nearest neighbours on either side whose roots are not -> (m, m_T_below, m_T_above) or None."""
    a = k["g"] * (1.0 + t * t) / (2.0 * k["v2"])
    d = t * t - 4.0 * a * alt
    if d < 0.0:
        return None
    for m0 in ((t + math.sqrt(d)) / (2.0 * a), (t - math.sqrt(d)) / (2.0 * a)):
        if not m0 > 2.0 * k["range_min"] or not abs(_root(k, m0, alt, arc) - t) < 1e-6 * t:   # (clear of the minimum range)
            continue
        lo, hi = m0 * (1.0 - 1e-9), m0 * (1.0 + 1e-9)
        flo, fhi = _root(k, lo, alt, arc) - t, _root(k, hi, alt, arc) - t
        if not flo * fhi < 0.0:
            continue
        while up(lo) < hi:
            mid = lo + (hi - lo) / 2.0
            fm = _root(k, mid, alt, arc) - t
            if fm == 0.0:
                lo = hi = mid
                break
            if (fm < 0.0) == (flo < 0.0):
                lo = mid
            else:
                hi = mid
        m = lo
        for _ in range(24):
            m = down(m)
        for _ in range(48):
            if _root(k, m, alt, arc) == t:
                before = after = m
                for _ in range(64):
                    before = down(before)
                    if _root(k, before, alt, arc) != t:
                        break
                for _ in range(64):
                    after = up(after)
                    if _root(k, after, alt, arc) != t:
                        break
                rb, ra = _root(k, before, alt, arc), _root(k, after, alt, arc)
                if rb != t and ra != t and (rb < t) != (ra < t):
                    return (m, before, after) if rb < t else (m, after, before)
            m = up(m)
    return None


@functools.lru_cache(maxsize=None)
def threshold_hits():
    """For both limited weapons and each of their nine thresholds -> [(weapon, name, t, j, alt, m, m_below, m_above)]; j = -1 / -2 for
    t_min / t_max, else the band threshold's index.  alt == 0 where such a hit exists, else the first of a ladder of altitudes."""
    out = []
    for w, nm in ((ROCKET, "rocket"), (TUBE, "tube")):
        k = B.rule(w)
        names = [("t_min", k["t_min"], -1), ("t_max", k["t_max"], -2)] + [("B_%d" % j, k["band"][j], j) for j in range(7)]
        for tn, t, j in names:
            assert math.isfinite(t) and t > 0.0
            for i in range(4000):
                alt = 0.0 if i == 0 else (i if i % 2 else -i) * 0.015625
                hit = _hit(k, t, alt, w.arc)
                if hit:
                    out.append((w, "%s %s" % (nm, tn), t, j, alt, hit[0], hit[1], hit[2]))
                    break
            else:
                raise AssertionError("no (m, alt) puts T exactly on %s of the %s" % (tn, nm))
    return out


def _check_threshold(t, j, side):
    def check(p, s):
        a = _own(p, s)
        T = _root(B.rule(p.weapon), p.m, p.alt, p.weapon.arc)
        st = int(a["status"])
        assert (T == t) if side == 0 else (T < t) if side < 0 else (T > t), (T, t)
        assert not st & (B.OUT_OF_RANGE | B.BELOW_MIN_RANGE)
        if j == -1:
            assert (st & B.ELEV_LOW != 0) == (side < 0) and not st & B.ELEV_HIGH          # T >= t_min: at the limit is inside
        elif j == -2:
            assert (st & B.ELEV_HIGH != 0) == (side > 0) and not st & B.ELEV_LOW          # t_max >= T likewise
        else:
            assert st == 0 and int(a["band"]) == (j if side < 0 else j + 1)
    return check


def _threshold_points():
    out = []
    for w, nm, t, j, alt, m, mb, ma in threshold_hits():
        fam = ("limit",) if j < 0 else ()
        out += [Point("%s: T == it (alt %r)" % (nm, alt), fam, w, m, alt, _check_threshold(t, j, 0), False),
                Point("%s: T just below (alt %r)" % (nm, alt), fam, w, mb, alt, _check_threshold(t, j, -1), False),
                Point("%s: T just above (alt %r)" % (nm, alt), fam, w, ma, alt, _check_threshold(t, j, 1), False)]
    return out


# ---- a target far below: T_lo < 0
def _check_below(p, s):
    lo, hi = s["arc"][B.LOW], s["arc"][B.HIGH]
    k = B.rule(p.weapon)
    assert _root(k, p.m, p.alt, B.LOW) < 0.0 and _f(lo["elevation"]) < 0.0 and _same(lo["apex"], 0.0)
    assert _f(hi["apex"]) > 0.0 and _f(lo["fall"]) > 0.0 and _f(lo["tof"]) > 0.0 and int(lo["status"]) & B.ELEV_LOW == (B.ELEV_LOW if p.weapon.elev_min >= 0 else 0)


def _below_points():
    return [Point("rocket: 100 m out, 500 m down", ("below", "arcs", "tof"), ROCKET, 100.0, -500.0, _check_below, True),
            Point("tube: 35 m out, 80 m down", ("below", "arcs", "tof"), TUBE, 35.0, -80.0, _check_below, True),
            Point("mortar: 12.5 m out, 3 m down", ("below", "units"), MORTAR, 12.5, -3.0, _check_below, True)]


# ---- m == 0, NaN, infinities
def _check_zero(p, s):
    hi, lo = s["arc"]
    assert math.isinf(_root(B.rule(p.weapon), 0.0, p.alt, B.HIGH)) and int(hi["status"]) & B.OUT_OF_RANGE == 0
    assert _same(hi["elevation"], (math.atan(math.inf) * B.DEG_PER_RAD) / B.unit_deg(p.weapon.unit)) and math.isnan(_f(hi["tof"])) and math.isnan(_f(hi["apex"]))
    assert math.isnan(_f(hi["fall"])) and int(hi["band"]) == 7
    t_lo = _root(B.rule(p.weapon), 0.0, p.alt, B.LOW)
    assert math.isinf(t_lo) or math.isnan(t_lo)
    if math.isnan(t_lo):
        assert int(lo["status"]) & (B.ELEV_LOW | B.ELEV_HIGH) == B.ELEV_LOW | B.ELEV_HIGH


def _check_no_solution(p, s):
    for a in s["arc"]:
        assert int(a["status"]) & B.OUT_OF_RANGE and not int(a["status"]) & (B.ELEV_LOW | B.ELEV_HIGH) and math.isnan(_f(a["elevation"]))


def _check_down_forever(p, s):
    hi, lo = s["arc"]
    assert int(hi["status"]) & B.OUT_OF_RANGE == 0 and _f(hi["elevation"]) > 0 and _f(lo["elevation"]) < 0 and _same(lo["apex"], 0.0)


def _edge_points():
    nan, inf = math.nan, math.inf
    out = [Point("m == 0, %s, alt %r" % (nm, alt), (), w, 0.0, alt, _check_zero, True)
           for w, nm in ((MORTAR, "mortar"), (ROCKET, "rocket"), (BINARY, "binary")) for alt in (0.0, -2.0)]
    out += [Point("m == 0, alt above: no solution", (), ROCKET, 0.0, 5000.0, _check_no_solution, True)]
    for nm, m, alt in (("NaN m", nan, 0.0), ("NaN alt", 500.0, nan), ("inf m", inf, 0.0), ("inf alt", 500.0, inf), ("both NaN", nan, nan)):
        out.append(Point(nm, (), TUBE, m, alt, _check_no_solution, True))
    out.append(Point("-inf alt", (), ROCKET, 500.0, -inf, _check_down_forever, True))
    return out


# ---- every unit and arc, away from every boundary: what the one-rule switches change
def _check_plain(p, s):
    hi, lo = s["arc"]
    assert int(hi["status"]) & B.OUT_OF_RANGE == 0 and _f(hi["elevation"]) > _f(lo["elevation"]) and _f(hi["tof"]) > _f(lo["tof"]) > 0.0
    assert _f(hi["apex"]) > _f(lo["apex"]) >= 0.0 and _f(hi["fall"]) > _f(lo["fall"])
    quarter = {B.MILS6400: 1600.0, B.MILS6000: 1500.0, B.DEGREES: 90.0}[p.weapon.unit]
    assert abs((_f(hi["elevation"]) + _f(lo["elevation"])) - quarter) < quarter * 0.2     # (complementary on flat ground, nearly so on a slope)
    if p.weapon.dispersion:
        assert _f(s["cross"]) > 0.0 and _f(hi["along"]) > 0.0 and _f(lo["along"]) > 0.0


def _plain_points():
    out = []
    for w, nm in ((MORTAR, "mortar"), (ROCKET, "rocket"), (TUBE, "tube")):
        rmax = w.velocity * w.velocity / w.gravity
        for frac, alt in ((0.35, 0.0), (0.6, 12.5), (0.8, -30.0), (0.93, 3.0)):
            out.append(Point("%s: %g of the flat range, alt %g" % (nm, frac, alt), ("arcs", "units", "tof"), w, rmax * frac, alt, _check_plain, True))
    return out


@functools.lru_cache(maxsize=None)
def points():
    out = _tie_points() + _disc_points() + _range_min_points() + _threshold_points() + _below_points() + _edge_points() + _plain_points()
    names = [p.name for p in out]
    assert len(set(names)) == len(names)
    return out


def checked_point(p):
    """The point's restatement, after the point's own check and the check on the cases that keeps the elevation's tolerance from
    deciding anything: no elevation within 4 ulps of a limit of the mount.  (The threshold points are exempt by construction: there T
    IS tan(limit), so the elevation is the limit but for the atan's error -- which is why the rule decides on T and never on it.)"""
    s = restate_point(p)
    p.check(p, s)
    if p.limits_apart:
        ud = B.unit_deg(p.weapon.unit)
        for a in s["arc"]:
            e = _f(a["elevation"])
            for lim in (p.weapon.elev_min, p.weapon.elev_max):
                if e == e and math.isfinite(B.tanlim(lim, ud)):     # (a quarter turn or more is no limit)
                    assert B.ulps(e, lim) > 4, (p.name, e, lim)
    return s


# ---- the maps
def _c7(r):
    return set(int(v) for v in np.unique(r["classes"] & 0x7F))


def _check_mortar_map(c, r):
    reach = R.reach(c.origin, c.window, c.viewport, c.minimap, c.mpx, c.hm, c.fit, 0.0)
    c7 = r["classes"] & 0x7F
    assert np.array_equal(c7 >= B.C_BAND0, (reach["classes"] & 0x7F) >= R.BAND0) and np.array_equal(c7 == B.C_OUT_OF_RANGE, (reach["classes"] & 0x7F) == R.OUT_OF_RANGE)
    assert _c7(r) <= {0, 1} | set(range(5, 13)) and (c7 >= B.C_BAND0).any() and (r["classes"] & B.C_ISO).any()
    assert np.isnan(r["tof"][c7 <= 1]).all() and not np.isnan(r["tof"][c7 >= 5]).any()


def _check_classes(*need):
    def check(c, r):
        assert set(need) <= _c7(r), (c.name, need, sorted(_c7(r)))
        if c.iso_s > 0.0 and r["classes"].size > 1:
            assert (r["classes"] & B.C_ISO).any()
    return check


def _iso_by(c, r):
    """Window pixels whose isochrone bit the right neighbour alone sets, and those the lower neighbour alone sets."""
    ow, oh = c.window
    full = B.ballistic_map(c.weapon, c.origin, (ow + 1, oh + 1), c.viewport, c.minimap, c.mpx, c.hm, c.fit, 0.0)
    with np.errstate(all="ignore"):
        b = np.floor(full["tof64"] / c.iso_s)
    src = full["source"]
    own_b, own_s = b[:oh, :ow], src[:oh, :ow]
    right = (src[:oh, 1:] == own_s) & ~np.isnan(b[:oh, 1:]) & (b[:oh, 1:] != own_b) & ~np.isnan(own_b) & (own_s != 0)
    low = (src[1:, :ow] == own_s) & ~np.isnan(b[1:, :ow]) & (b[1:, :ow] != own_b) & ~np.isnan(own_b) & (own_s != 0)
    return right & ~low, low & ~right, src, b


def _check_tile_edges(c, r):
    right, low, _, _ = _iso_by(c, r)
    iso = (r["classes"] & B.C_ISO) != 0
    ow, oh = c.window
    cols = [x for x in (TW - 1, 2 * TW - 1, ow - 1) if x < ow]
    rows = [y for y in (TH - 1, 2 * TH - 1, oh - 1) if y < oh]
    assert all(right[:, x].any() for x in cols), ("an isochrone across every tile's right edge and the window's", [int(right[:, x].sum()) for x in cols])
    assert all(low[y, :].any() for y in rows), ("... and across every bottom edge", [int(low[y, :].sum()) for y in rows])
    assert iso[right].all() and iso[low].all() and np.array_equal(iso, ((r["classes"] & B.C_ISO) != 0))


def _check_seam(c, r):
    right, low, src, b = _iso_by(c, r)
    oh, ow = r["classes"].shape
    assert {B.SCALES, B.HEIGHTMAP} <= set(int(v) for v in np.unique(r["source"]))
    own_s, own_b = src[:oh, :ow], b[:oh, :ow]
    across = (src[:oh, 1:ow + 1] != own_s) & (src[:oh, 1:ow + 1] != 0) & (b[:oh, 1:ow + 1] != own_b) & (own_s != 0)
    quiet = (src[1:oh + 1, :ow] != own_s) | (b[1:oh + 1, :ow] == own_b)
    sel = across & quiet
    assert sel.any() and not (r["classes"][sel] & B.C_ISO).any() and (r["classes"] & B.C_ISO).any()


def _check_nothing(valid):
    def check(c, r):
        assert r["valid"] == valid and not r["classes"].any() and np.isnan(r["tof"]).all()
    return check


def _check_zero_range(px, py):
    def check(c, r):
        assert r["meters"][py, px] == 0.0 and math.isnan(float(r["tof"][py, px])) and r["classes"][py, px] & 0x7F != 0
    return check


@functools.lru_cache(maxsize=None)
def maps():
    out = []
    whole = (0, 97, 0, 66)
    zoom = (1.7, 0.95, -9.25, 2.5)
    origin = (20.4 * 97 / 1400, 30.0)
    out.append(Map("the mortar, every band", ("units",), MORTAR, RC.long_map(), whole, None, origin, (96, 64), None, True, 2.0, _check_mortar_map))
    # the tube over the long map: its minimum range, both limits of the mount and bands between them (T runs from steep to 45 degrees)
    out.append(Map("the tube over terrain", ("range_min", "arcs", "tof"), TUBE, RC.long_map(), whole, None, origin, (96, 64), None, True, 1.5,
                   _check_classes(B.C_BELOW_MIN_RANGE, B.C_ELEV_HIGH, B.C_BAND0 + 7)))
    out.append(Map("the tube on the scales", ("limit", "range_min", "arcs", "tof"), TUBE, None, None, 35.0, (12.25, 30.75), (96, 64), None, True, 1.5,
                   _check_classes(B.C_OUT_OF_RANGE, B.C_BELOW_MIN_RANGE, B.C_ELEV_LOW, B.C_ELEV_HIGH, B.C_BAND0, B.C_BAND0 + 7)))
    out.append(Map("the rocket on the scales", ("limit", "range_min", "arcs", "tof", "isochrone"), ROCKET, None, None, 60.0, (12.25, 30.75), (96, 64), None, True, 1.0,
                   _check_classes(B.C_OUT_OF_RANGE, B.C_BELOW_MIN_RANGE, B.C_ELEV_LOW, B.C_ELEV_HIGH, B.C_BAND0, B.C_BAND0 + 7)))
    # the tile's edges: one tile, one short of it, one over in each axis, two tiles and a remainder, one pixel; steep terrain, zoomed and panned
    for w, h in ((1, 1), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 2, 2 * TH + 1)):
        need = (B.C_OUT_OF_RANGE,) if (w, h) != (1, 1) else ()
        out.append(Map("window %d x %d" % (w, h), (), SHORT, RC.steep_map(), (8, 56, 4, 40), 3.0, (12.5, 6.25), (w, h), zoom, True, 0.25, _check_classes(*need)))
    # isochrones across every tile edge: on the low arc the time of flight grows with the range, a tenth of a second every two pixels or so
    for w, h in ((TW, TH), (2 * TW + 2, 2 * TH + 1)):
        out.append(Map("isochrones across tile edges, %d x %d" % (w, h), ("isochrone",), ROCKET, None, None, 9.0, (-7.3, -11.6), (w, h), None, True, 0.1, _check_tile_edges))
    out.append(Map("seam", ("isochrone",), ROCKET, RC.long_map(), (20, 70, 10, 50), 21.0, (44.0, 31.0), (96, 64), None, True, 0.5, _check_seam))
    out.append(Map("bounds offset", (), SHORT, RC.steep_map(), (8, 56, 4, 40), 3.0, (20.0, 11.0), (65, 33), zoom, False, 0.0, _check_classes(B.C_OUT_OF_RANGE)))
    out.append(Map("NaN origin", (), TUBE, RC.steep_map(), whole, 3.0, (float("nan"), 4.0), (65, 17), None, True, 1.0, _check_nothing(0)))
    out.append(Map("no heightmap, no m/px", (), TUBE, None, None, None, (12.25, 30.75), (65, 17), None, True, 0.0, _check_nothing(1)))
    out.append(Map("m == 0, scales", (), ROCKET, None, None, 2.5, (10.5, 7.5), (65, 33), None, True, 1.0, _check_zero_range(10, 7)))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def checked_map(c):
    r = restate_map(c)
    c.check(c, r)
    return r


# ---- lines for k_ballistic_lines over a heightmap: generic, both directions, some outside the rectangle (the scales branch) and some
# with no source at all when the frame has no m/px
def lines_scene():
    hm = RC.steep_map()
    rng = np.random.default_rng(23)
    lines = np.concatenate([rng.uniform((8, 4, 8, 4), (56, 40, 56, 40), size=(40, 4)), rng.uniform(-20, 120, size=(12, 4))]).astype(np.float32)
    return dict(hm=hm, minimap=(8, 56, 4, 40), mpx=3.0, lines=lines)
