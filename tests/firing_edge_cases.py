"""Firing solutions and label strings at their decision boundaries (tests/test_firing_edges_host.py, tests/test_firing_edges_gpu.py).
Pure numpy and the restatements (tests/firing_ref.py, tests/label_ref.py): nothing here touches the library.

A Case is the input of ONE smhv_firing_solutions call -- lines, mpx, the minimap rectangle, a heightmap (a name in heightmaps()),
fit_to_minimap, the viewport -- with a check that asserts on the restatement's output that the case still sits on its boundary
(a case whose boundary has moved fails on the CPU), and, where it prints, the label rows of its lines as LITERAL bytes, typed
here by hand: rows[i] == [] means line i prints nothing, rows[i] is None that line i prints and its rows are not typed out (the
many-lined tie cases type a few lines each, {line index: rows}; the device test holds the others to label_ref's rows for the
restated numbers).  rows is None for a case the label path does not take: the per-call label path reads the current frame's own
minimap rectangle, SCENE_RECT, so of the heightmap cases only those under that rectangle go through it.

On the per-call path the record's-meters input of a line is sqrt(ax*ax + ay*ay) * mpx in f64: for a line of length 1 that is mpx
itself, so any f64 is injected as `meters` exactly.

Families: "ties" (texel rounding half away from zero and the [0, n) test), "range" (the discriminant's sign change, zero and
non-finite meters), "print" (what the label prints), "bearings", "degenerate" (geometry the public header defines)."""
import math

import numpy as np

import firing_ref as R
import label_ref as LR

f32 = np.float32
FAMILIES = ("ties", "range", "print", "bearings", "degenerate")
SCENE_RECT = (42, 321, 58, 532)                                   # scene 0 of tests/minimap_scenes.py: 279 x 474, no power of two
POW2_RECT = (0, 64, 0, 32)
MAGENTA = (255, 0, 255, 255)
DEG, PM = b"\xb0", b"\xb1"


def _ramp(w, h):
    """A heightmap whose texel names itself: no two neighbours, and no two texels a case uses, hold the same value."""
    y, x = np.mgrid[0:h, 0:w]
    v = 97 * y + 3 * x + 1
    assert v.max() < 65536
    return v.astype(np.uint16)


_HM = {}


def heightmaps():
    """name -> (data u16 [h, w], bounds, scale).  "pow2" lies under POW2_RECT at two pixels per texel; "pow2 offset" has bounds that
    make the offset of "fit to minimap" off exact (W + b0x = 64 = the rectangle's width, H + b0y = 32 = its height: the offset is
    (32, 16) and the coordinate p - 32, p - 16); "wrap" is for right < left (see the degenerate family).  The "scene" maps have the
    size of SCENE_RECT: z = 40 gives 0.003125 m per unit of the texel value, "unit" exactly 1 m per unit, "steep" 0.3125 m, "sat"
    about 2.3e34 m.  "scene offset" lies under SCENE_RECT with "fit to minimap" off, exactly: 256 x 256 with bounds[0] = (23, 218), so
    that W + b0x = 279 and H + b0y = 474 are the rectangle's own width and height, the offset is (23, 218), what is left of the
    rectangle 256 x 256 and the coordinate (p - 65, p - 276); a metre per unit."""
    if not _HM:
        z = (0, 0)
        sw, sh = SCENE_RECT[1] - SCENE_RECT[0], SCENE_RECT[3] - SCENE_RECT[2]
        _HM.update({
            "pow2": (_ramp(32, 16), (z, z), (1.0, 1.0, 40.0)),
            "pow2 offset": (_ramp(32, 16), ((32, 16), z), (1.0, 1.0, 40.0)),
            "wrap": (_ramp(32, 16), ((-16, 16), z), (1.0, 1.0, 40.0)),
            "scene": (_ramp(sw, sh), (z, z), (1.0, 1.0, 40.0)),
            "scene unit": (_ramp(sw, sh), (z, z), (1.0, 1.0, 12799.8046875)),
            "scene steep": (_ramp(sw, sh), (z, z), (1.0, 1.0, 4000.0)),
            "scene sat": (_ramp(sw, sh), (z, z), (1.0, 1.0, 3e38)),
            "scene offset": (_ramp(256, 256), ((sw - 256, sh - 256), z), (1.0, 1.0, 12799.8046875)),
        })
    return _HM


class Case:
    def __init__(self, name, family, lines, check, mpx=None, minimap=None, hm=None, fit=True, viewport=None, rows=None):
        self.name, self.family, self.check = name, family, check
        self.lines = [tuple(float(f32(v)) for v in l) for l in lines]
        if isinstance(rows, dict):                                 # {line index: rows}: every other line prints too, its rows not typed
            rows = [rows.get(i) for i in range(len(self.lines))]
        self.mpx, self.minimap, self.hm, self.fit, self.viewport, self.rows = mpx, minimap, hm, fit, viewport, rows
        assert family in FAMILIES and (rows is None or len(rows) == len(self.lines))
        assert rows is None or hm is None or minimap == SCENE_RECT, name

    def __repr__(self):
        return "Case(%s: %s)" % (self.family, self.name)

    @property
    def group(self):
        """What one label call shares: cases with the same group go into one render with labels."""
        return (repr(self.mpx), self.hm, self.fit, self.viewport)

    @property
    def silent(self):
        """The case takes the label path and none of its lines prints."""
        return self.rows is not None and all(r == [] for r in self.rows)


def restate(case, minimap="own", hm="own", mpx="own"):
    """The restatement on every line of the case -> [(firing dict, the four unrounded heightmap coordinates or None)].  The
    coordinates are the restatement's own: what it hands to round_f64."""
    mm = case.minimap if minimap == "own" else minimap
    mpx = case.mpx if mpx == "own" else mpx
    ref_hm = (heightmaps()[case.hm] if case.hm is not None else None) if hm == "own" else hm
    out = []
    for ln in case.lines:
        seen, orig = [], R.round_f64
        R.round_f64 = lambda v: (seen.append(v), orig(v))[1]
        try:
            met = R.record_meters(ln, mpx) if mpx is not None else None
            want = R.firing_line(ln, mm, met, ref_hm, case.fit, case.viewport)
        finally:
            R.round_f64 = orig
        out.append((want, tuple(seen) if seen else None))
    return out


def label_viewport(case):
    """The case's viewport as label_ref takes it: a scale of 0 means 1."""
    vp = case.viewport or (1.0, 1.0, 0.0, 0.0)
    return tuple(1.0 if (k < 2 and v == 0) else v for k, v in enumerate(vp))


def label_rows(case, wants):
    """label_ref's rows for the restated firing of every line -> [[bytes]]."""
    vp = label_viewport(case)
    return [[r[2] for r in LR.format_label(ln, w, vp, MAGENTA)["runs"]] for ln, (w, _) in zip(case.lines, wants)]


def _same_float(a, b):
    return a == b or (a != a and b != b)


def stable_bearings(want):
    """Moving atan2f's result one ulp either way leaves both bearings as they are (NaN stays NaN)."""
    p0x, p0y, p1x, p1y = want["p"]
    with np.errstate(all="ignore"):
        a = R.atan2f(f32(p0y - p1y), f32(p0x - p1x))
        if a != a:
            return all(float(b) != float(b) for b in want["bearing"])
        for s in (-10, 10):
            alt = R.bearings(p0x, p0y, p1x, p1y, angle=np.nextafter(a, f32(s)))
            if not all(_same_float(float(alt[k]), float(want["bearing"][k])) for k in range(2)):
                return False
    return True


def mils_clear_of_ties(want):
    """Every finite mils value is farther than 1e-6 from a .5: the device's atan may differ from the host's by ulps."""
    return all(m != m or abs((m % 1.0) - 0.5) > 1e-6 for m in want["mils"])


# ---- texel ties ---------------------------------------------------------------------------------------------------------------
class T(float):
    """A coordinate that must be exactly this tie."""


class IN(float):
    """The f32 neighbour, on the inside, of the end point whose coordinate is exactly this tie."""


def _texel(c, n):
    """The texel the rule gives a coordinate of the spec, stated on its own: a tie goes away from zero; the inner neighbour of
    -0.5 is texel 0, of n - 0.5 texel n - 1; any other value of the specs is positive and no tie."""
    if isinstance(c, IN):
        return 0 if c < 0 else n - 1
    return -1 if c < 0 else int(math.floor(c + 0.5))


def _tie_specs(W, H):
    """(name, (c0x, c0y, c1x, c1y)) in heightmap coordinates: every other coordinate is a quarter, far from any tie."""
    a, b, c, d = 3.25, 6.25, 10.25, 4.75
    out = []
    for k, par in ((2.5, "even"), (3.5, "odd"), (12.5, "even"), (7.5, "odd")):
        out += [("x0 = %.1f (k %s)" % (k, par), (T(k), b, c, d)), ("y0 = %.1f (k %s)" % (k, par), (a, T(k), c, d)),
                ("x1 = %.1f (k %s)" % (k, par), (a, b, T(k), d)), ("y1 = %.1f (k %s)" % (k, par), (a, b, c, T(k)))]
    out += [("ties on end 0 only", (T(2.5), T(3.5), c, d)), ("ties on end 1 only", (a, b, T(4.5), T(5.5))),
            ("ties on both ends", (T(2.5), T(3.5), T(4.5), T(5.5)))]
    for n, ax in ((W, 0), (H, 1)):
        for end in (0, 1):
            for tie, what in ((-0.5, "-0.5"), (n - 0.5, "n - 0.5")):
                for kind in (T, IN):
                    spec = [a, b, c, d]
                    spec[2 * end + ax] = kind(tie)
                    out.append(("%s%d %s %s" % ("xy"[ax], end, "=" if kind is T else "inside of", what), tuple(spec)))
    return out


# the three exact geometries: coordinate -> the end point's map-ROI value, and which way (in end-point space) the inside lies
_GEOMETRIES = {
    "identity": dict(minimap=POW2_RECT, hm="pow2", fit=True, viewport=None, p=lambda ax, c: 2.0 * c),
    "viewport": dict(minimap=POW2_RECT, hm="pow2", fit=True, viewport=(0.5, 0.5, 8.0, 8.0), p=lambda ax, c: 2.0 * c),
    "offset": dict(minimap=POW2_RECT, hm="pow2 offset", fit=False, viewport=None, p=lambda ax, c: c + (32.0, 16.0)[ax]),
    # ... and the offset under the rectangle the per-call label path reads, so that "fit to minimap" off reaches k_label_plan.  The
    # typed lines (a metre per unit: the altitude row names the texels): the tie 2.5 is texel 3, 7.5 is 8, 12.5 is 13 --
    # data[6, 3] - data[5, 10] = 592 - 516, data[8, 3] - data[5, 10] = 786 - 516, data[5, 13] - data[6, 3] = 525 - 592; the end
    # point ON -0.5 is outside, so the scales give 2 m/px over sqrt(7.5^2 + 1.5^2) px; its neighbour inside is texel 0:
    # data[6, 0] = 583; x1 on n - 0.5 is outside, its neighbour inside is texel 255: data[5, 255] = 1251, 252.25 texels away
    "scene offset": dict(minimap=SCENE_RECT, hm="scene offset", fit=False, viewport=None, p=lambda ax, c: c + (65.0, 276.0)[ax], rows={
        "x0 = 2.5 (k even)": [b"8m", PM + b"76m alt", b"<- 1597 mil", b"259" + DEG, b"1597 mil ->", b"79" + DEG],
        "y0 = 7.5 (k odd)": [b"8m", PM + b"270m alt", b"<- 1596 mil", b"249" + DEG, b"1597 mil ->", b"69" + DEG],
        "x1 = 12.5 (k even)": [b"9m", PM + b"67m alt", b"<- 1596 mil", b"261" + DEG, b"1596 mil ->", b"81" + DEG],
        "x0 = -0.5": [b"22m", b"1591 mil", b"-> 82" + DEG, b"<- 262" + DEG],
        "x0 inside of -0.5": [b"11m", PM + b"67m alt", b"<- 1595 mil", b"262" + DEG, b"1596 mil ->", b"82" + DEG],
        "x1 = n - 0.5": [b"505m", b"1385 mil", b"-> 90" + DEG, b"<- 270" + DEG],
        "x1 inside of n - 0.5": [b"252m", PM + b"659m alt", b"<- 1514 mil", b"270" + DEG, b"RANGE! ->", b"90" + DEG]}),
}


def _check_ties(spec_of):
    def check(case, wants):
        data, _, scale = heightmaps()[case.hm]
        H, W = data.shape
        seen_out = seen_in = 0
        for i, (want, coords) in enumerate(wants):
            spec = spec_of[i]
            tex = [_texel(spec[k], (W, H)[k & 1]) for k in range(4)]
            for k in range(4):
                if isinstance(spec[k], T):
                    assert coords[k] == float(spec[k]), (case, i, k, coords[k].hex(), "is not the tie", float(spec[k]))
                elif isinstance(spec[k], IN):
                    lo, hi = (float(spec[k]), float(spec[k]) + 1e-4) if spec[k] < 0 else (float(spec[k]) - 1e-4, float(spec[k]))   # (an f32 ulp below 1024)
                    assert lo < coords[k] < hi, (case, i, k, coords[k])
                else:
                    assert coords[k] == float(spec[k]), (case, i, k, coords[k])
            inside = all(0 <= tex[k] < (W, H)[k & 1] for k in range(4))
            if inside:
                assert want["source"] == R.HEIGHTMAP, (case, i)
                assert want["alt_delta"] == R.height(data, scale[2], tex[2], tex[3]) - R.height(data, scale[2], tex[0], tex[1]), (case, i, tex)
                seen_in += 1
            else:
                assert want["source"] == R.SCALES and want["alt_delta"] == 0.0, (case, i)
                seen_out += 1
            assert stable_bearings(want) and mils_clear_of_ties(want), (case, i)
        assert seen_in >= 8 and seen_out >= 4, (case, seen_in, seen_out)
    return check


def _tie_cases():
    out = []
    for gname, g in _GEOMETRIES.items():
        H, W = heightmaps()[g["hm"]][0].shape
        lines, specs, rows = [], [], {}
        for name, spec in _tie_specs(W, H):
            if name in g.get("rows", {}):
                rows[len(lines)] = g["rows"][name]
            ln = []
            for k in range(4):
                p = f32(g["p"](k & 1, float(spec[k])))
                if isinstance(spec[k], IN):                       # the neighbour of the TRANSLATED end point, taken back through the viewport
                    s, t = (f32(1), f32(0)) if g["viewport"] is None else (f32(g["viewport"][k & 1]), f32(g["viewport"][2 + (k & 1)]))
                    P = np.nextafter(f32(f32(p * s) + t), f32(1e9) if spec[k] < 0 else f32(-1e9))
                    p = f32(f32(P - t) / s)
                    assert f32(f32(p * s) + t) == P
                ln.append(p)
            lines.append(ln)
            specs.append(spec)
        out.append(Case("every tie, %s geometry" % gname, "ties", lines, _check_ties(specs), mpx=2.0, minimap=g["minimap"], hm=g["hm"], fit=g["fit"],
                        viewport=g["viewport"], rows=rows if "rows" in g else None))
        assert len(rows) == len(g.get("rows", {}))
    return out


def rect_tie_lines(rect, W, H, per_axis=4):
    """Ties under a rectangle that is no power of two wide, by search, for a heightmap of the rectangle's own size (W x H) and the
    identity viewport: scans the end points p = edge + k + 0.5 of each axis and keeps those whose RESTATED coordinate is exactly
    k + 0.5 ((p - edge) / n * n need not be p - edge) -> (lines, notes): notes[i] = (axis, end, k + 0.5, the restated coordinate).
    -0.5 and n - 0.5 are always kept: exact, they are end points outside; where the division's rounding makes one inexact, it is a
    point that is NOT a tie, and the check holds it to that."""
    left, right, top, bottom = rect
    assert (W, H) == (right - left, bottom - top)
    probe_hm = (np.zeros((H, W), np.uint16), ((0, 0), (0, 0)), (1.0, 1.0, 1.0))
    mid = (f32(left + (right - left) * 0.37), f32(top + (bottom - top) * 0.41))
    far = (f32(left + (right - left) * 0.71), f32(top + (bottom - top) * 0.67))

    def coord(ax, p):
        ln = (p, mid[1], far[0], far[1]) if ax == 0 else (mid[0], p, far[0], far[1])
        c = Case("probe", "ties", [ln], None, minimap=rect, hm=None)
        return restate(c, hm=probe_hm)[0][1][ax]

    lines, notes = [], []
    for ax, (edge, n) in enumerate(((left, W), (top, H))):
        ties = [k for k in range(0, n - 1) if coord(ax, f32(edge + k + 0.5)) == k + 0.5]
        even, odd = [k for k in ties if k % 2 == 0], [k for k in ties if k % 2 == 1]
        picked = sorted(even[:per_axis // 2] + odd[:per_axis // 2] + even[-1:] + odd[-1:])
        for k in [-1] + picked + [n - 1]:
            p = f32(edge + k + 0.5)
            c = coord(ax, p)
            for end in (0, 1):
                ln = [mid[0], mid[1], far[0], far[1]] if end == 0 else [far[0], far[1], mid[0], mid[1]]
                ln[2 * end + ax] = p
                lines.append(tuple(float(v) for v in ln))
                notes.append((ax, end, k + 0.5, c))
    return lines, notes


def _check_rect_ties(notes, W, H, need_each_kind):
    def check(case, wants):
        data, _, scale = heightmaps()[case.hm]
        ties = {0: set(), 1: set()}
        kinds = set()
        for (want, coords), (ax, end, tie, c) in zip(wants, notes):
            n = (W, H)[ax]
            got = coords[2 * end + ax]
            assert got == c, (case, ax, end, tie)
            tex = [int(R.round_f64(v)) for v in coords]
            if got == tie:                                        # exactly a tie: half away from zero
                assert tex[2 * end + ax] == (int(tie + 0.5) if tie > 0 else -1)
                if 0 < tie < n - 0.5:
                    ties[ax].add(tie)
                else:
                    kinds.add("below 0" if tie < 0 else "at n")
                    assert want["source"] != R.HEIGHTMAP, (case, ax, end, tie)
            else:                                                 # the division made it inexact: the neighbour decides, and says so
                assert tie in (-0.5, n - 0.5) and abs(got - tie) < 1e-9, (case, ax, end, tie, got)
            if want["source"] == R.HEIGHTMAP:
                assert want["alt_delta"] == R.height(data, scale[2], tex[2], tex[3]) - R.height(data, scale[2], tex[0], tex[1]), (case, tex)
            assert stable_bearings(want) and mils_clear_of_ties(want), (case, ax, end, tie)
        assert len(ties[0]) >= 4 and len(ties[1]) >= 4, (case, ties)
        assert {int(t) % 2 for t in ties[0]} == {0, 1} and {int(t) % 2 for t in ties[1]} == {0, 1}, (case, ties)
        if need_each_kind:
            assert kinds == {"below 0", "at n"}, (case, kinds)
    return check


def _scene_tie_cases():
    """The rectangle the per-call label path reads, under a heightmap of a metre per unit: the altitude row names the two texels.
    The second case has the first one's lines under a power-of-two viewport: (p / 2 + 8 - 29) / 139.5 is (p - 42) / 279 exactly, so
    the ties are where they were.  The far end is texel (198, 318) = 31441; the typed lines, by their index:
      0, 14  x on -0.5 and on n - 0.5: outside, the scales' 0.75 m/px (175.3 m, 110.4 m)
      4      x = 2.5 is texel 3:  31441 - data[194, 3] = 31441 - 18828;  5 is the same line from its other end
      6      x = 3.5 is texel 4:  31441 - data[194, 4] = 31441 - 18831
      16     y = -0.5 made inexact by the division, -0.49999999999999994: texel 0, inside: 31441 - data[0, 103] = 31441 - 310
      20     y = 2.5 is texel 3:  31441 - data[3, 103] = 31441 - 601
      22     y = 3.5 is texel 4:  31441 - data[4, 103] = 31441 - 698
    Uphill is out of range every time."""
    W, H = SCENE_RECT[1] - SCENE_RECT[0], SCENE_RECT[3] - SCENE_RECT[2]
    lines, notes = rect_tie_lines(SCENE_RECT, W, H)
    rows = {
        0: [b"175m", b"1527 mil", b"-> 122" + DEG, b"<- 302" + DEG],
        4: [b"231m", PM + b"12613m alt", b"<- 1566 mil", b"302" + DEG, b"RANGE! ->", b"122" + DEG],
        5: [b"231m", PM + b"12613m alt", b"<- 1566 mil", b"302" + DEG, b"RANGE! ->", b"122" + DEG],
        6: [b"230m", PM + b"12610m alt", b"<- 1566 mil", b"302" + DEG, b"RANGE! ->", b"122" + DEG],
        14: [b"110m", b"1554 mil", b"-> 33" + DEG, b"<- 213" + DEG],
        16: [b"332m", PM + b"31131m alt", b"<- 1566 mil", b"343" + DEG, b"RANGE! ->", b"163" + DEG],
        20: [b"329m", PM + b"30840m alt", b"<- 1567 mil", b"343" + DEG, b"RANGE! ->", b"163" + DEG],
        22: [b"328m", PM + b"30743m alt", b"<- 1567 mil", b"343" + DEG, b"RANGE! ->", b"163" + DEG],
    }
    assert notes[4][2:] == (2.5, 2.5) and notes[6][2:] == (3.5, 3.5) and notes[20][2:] == (2.5, 2.5) and notes[22][2:] == (3.5, 3.5)
    assert notes[16][2] == -0.5 and -0.5 < notes[16][3] < -0.4999999
    check = _check_rect_ties(notes, W, H, True)
    return [Case("ties by search under the scene's rectangle", "ties", lines, check, mpx=0.75, minimap=SCENE_RECT, hm="scene unit", rows=rows),
            Case("the scene's ties under a power-of-two viewport", "ties", lines, check, mpx=0.75, minimap=SCENE_RECT, hm="scene unit",
                 viewport=(0.5, 0.5, 8.0, 8.0), rows=rows)]


# ---- range --------------------------------------------------------------------------------------------------------------------
EAST, WEST, SOUTH, NORTH = (0, 0, 1, 0), (1, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 0)     # unit lines: record_meters == mpx
# the bearing rows of the four unit lines on the scales branch, by hand: a line drawn from P0 towards the east has fwd 90, bck 270,
# and d.x = P0.x - P1.x < 0, so its rows read "-> fwd", "<- bck"; towards the west fwd 270, bck 90 and d.x > 0: "-> bck", "<- fwd".
# Towards the south (y grows downwards) fwd 180, bck 0, d.x == 0 counts as >= 0: "-> bck", "<- fwd"; towards the north fwd 0, bck 180.
ARROWS = {EAST: [b"-> 90" + DEG, b"<- 270" + DEG], WEST: [b"-> 90" + DEG, b"<- 270" + DEG], SOUTH: [b"-> 0" + DEG, b"<- 180" + DEG],
          NORTH: [b"-> 180" + DEG, b"<- 0" + DEG]}


def range_limit():
    """Both f64 neighbours of the discriminant's sign change at altitude 0, by bisection on the restatement -> (last range with
    mils, first range without)."""
    lo, hi = 1232.0, 1233.0
    assert not math.isnan(R.calc(lo, 0.0)) and math.isnan(R.calc(hi, 0.0))
    while math.nextafter(lo, math.inf) != hi:
        mid = lo + (hi - lo) / 2
        if math.isnan(R.calc(mid, 0.0)):
            hi = mid
        else:
            lo = mid
    return lo, hi


def _check_injected(meters, mils, line=EAST):
    """The injected meters arrive as they are; mils: a float (both directions, exactly), "nan", or a (lo, hi) interval."""
    def check(case, wants):
        (want, _), = wants
        assert want["source"] == R.SCALES and _same_float(want["meters"], meters), (case, want["meters"])
        assert R.record_meters(line, case.mpx) == meters or meters != meters
        for m in want["mils"]:
            if mils == "nan":
                assert m != m, (case, m)
            elif isinstance(mils, tuple):
                assert mils[0] < m < mils[1], (case, m)
            else:
                assert m == mils, (case, m)
        assert mils_clear_of_ties(want) and stable_bearings(want), case
    return check


def _check_one_side(finite_dir):
    """alt_delta alone puts one direction out of range: at altitude 0 both directions have mils."""
    def check(case, wants):
        for want, _ in wants:
            assert want["source"] == R.HEIGHTMAP and not math.isnan(R.calc(want["meters"], 0.0)), case
            assert not math.isnan(want["mils"][finite_dir]) and math.isnan(want["mils"][1 - finite_dir]), (case, want["mils"])
            assert (want["alt_delta"] < 0) == (finite_dir == 0) and mils_clear_of_ties(want) and stable_bearings(want), case
    return check


def _scene(cx0, cy0, cx1, cy1):
    """A line under SCENE_RECT by its heightmap coordinates (a texel is one map pixel there)."""
    return (SCENE_RECT[0] + cx0, SCENE_RECT[2] + cy0, SCENE_RECT[0] + cx1, SCENE_RECT[2] + cy1)


def _range_cases():
    lo, hi = range_limit()
    one = lambda rows: [rows]
    out = [
        Case("0 m", "range", [EAST], _check_injected(0.0, 1600.0), mpx=0.0, rows=one([b"0m", b"1600 mil"] + ARROWS[EAST])),
        Case("the smallest subnormal", "range", [EAST], _check_injected(5e-324, 1600.0), mpx=5e-324, rows=one([b"0m", b"1600 mil"] + ARROWS[EAST])),
        Case("the last range with mils", "range", [EAST], _check_injected(lo, (800.0, 800.00001)), mpx=lo, rows=one([b"1232m", b"800 mil"] + ARROWS[EAST])),
        Case("the first range without", "range", [WEST], _check_injected(hi, "nan", WEST), mpx=hi, rows=one([b"1232m", b"RANGE!"] + ARROWS[WEST])),
        Case("+inf m", "range", [EAST], _check_injected(math.inf, "nan"), mpx=math.inf, rows=one([])),
        Case("NaN m", "range", [EAST], _check_injected(math.nan, "nan"), mpx=math.nan, rows=one([])),
        # 90 texels across and 40 rows down the ramp: 40 * 97 + 270 = 4150 units of 0.3125 m = 1296.9 m of altitude, more than the
        # V^2 / 2g = 616 m a shell climbs at most; the line runs west-north-west (294 degrees) or back (114)
        Case("out of range uphill only: mils[0] alone", "range", [_scene(100.25, 60.25, 10.25, 20.25)], _check_one_side(0), mpx=1.0, minimap=SCENE_RECT,
             hm="scene steep", rows=one([b"98m", PM + b"1296m alt", b"<- 1571 mil", b"294" + DEG, b"RANGE! ->", b"114" + DEG])),
        Case("out of range uphill only: mils[1] alone", "range", [_scene(10.25, 20.25, 100.25, 60.25)], _check_one_side(1), mpx=1.0, minimap=SCENE_RECT,
             hm="scene steep", rows=one([b"98m", PM + b"1296m alt", b"<- 1571 mil", b"294" + DEG, b"RANGE! ->", b"114" + DEG])),
    ]
    return out


# ---- what the label prints ------------------------------------------------------------------------------------------------------
def _check_meters_tie(meters, line, labelled=True):
    """The injected meters sit exactly on the .5 (or on the cut-off's neighbour) the case names."""
    inner = _check_injected(meters, (0.0, 1600.0) if meters <= 1232.0 else "nan", line)

    def check(case, wants):
        inner(case, wants)
        m = wants[0][0]["meters"]
        assert (m < 999999.5) == labelled and (m % 1.0 == 0.5 or abs(m - 999999.5) < 1e-9), (case, m)
    return check


def _check_altitude(pred, dx_sign, dy_sign=None):
    """The altitude's property, and which way the arrows' rule sees the line (the signs of d = P0 - P1)."""
    def check(case, wants):
        (want, coords), = wants
        assert want["source"] == R.HEIGHTMAP and pred(want["alt_delta"]), (case, want["alt_delta"])
        p0x, p0y, p1x, p1y = want["p"]
        assert np.sign(p0x - p1x) == dx_sign and (dy_sign is None or np.sign(p0y - p1y) == dy_sign), case
        assert all(abs((c % 1.0) - 0.5) > 0.2 for c in coords), (case, coords)           # (no texel tie here: another family's business)
        assert abs((want["meters"] % 1.0) - 0.5) > 1e-3 and mils_clear_of_ties(want) and stable_bearings(want), case
    return check


def _frac_above_half(sign):
    return lambda a: a * sign > 1.0 and (abs(a) % 1.0) > 0.5      # trunc, round and floor all differ on one sign or the other


def _print_cases():
    up, below = math.nextafter(999999.5, math.inf), math.nextafter(999999.5, 0.0)
    out = []
    for meters, line, rows in (
            (0.5, EAST, [b"0m", b"1600 mil"]), (1.5, WEST, [b"2m", b"1599 mil"]), (2.5, SOUTH, [b"2m", b"1599 mil"]), (9.5, NORTH, [b"10m", b"1596 mil"]),
            (99.5, EAST, [b"100m", b"1559 mil"]), (999.5, WEST, [b"1000m", b"1118 mil"]), (99999.5, SOUTH, [b"100000m", b"RANGE!"]),
            (below, NORTH, [b"999999m", b"RANGE!"]), (999999.5, EAST, None), (up, SOUTH, None)):
        out.append(Case("%r m" % meters, "print", [line], _check_meters_tie(meters, line, rows is not None), mpx=meters,
                        rows=[rows + ARROWS[line] if rows is not None else []]))
    out.append(Case("NaN m on a vertical line", "print", [NORTH], _check_injected(math.nan, "nan", NORTH), mpx=math.nan, rows=[[]]))
    hm = dict(mpx=1.0, minimap=SCENE_RECT)
    # "scene": 41 rows and 21 columns apart is 41 * 97 + 63 = 4040 units of 0.003125 m = 12.625 m; the line runs 153 degrees or back
    out += [
        Case("altitude +12.6", "print", [_scene(10.25, 10.25, 31.25, 51.25)], _check_altitude(_frac_above_half(1), -1), hm="scene",
             rows=[[b"46m", PM + b"12m alt", b"<- 1581 mil", b"333" + DEG, b"1581 mil ->", b"153" + DEG]], **hm),
        Case("altitude -12.6", "print", [_scene(31.25, 51.25, 10.25, 10.25)], _check_altitude(_frac_above_half(-1), 1), hm="scene",
             rows=[[b"46m", PM + b"12m alt", b"<- 1581 mil", b"333" + DEG, b"1581 mil ->", b"153" + DEG]], **hm),
        # "scene unit": a metre per unit, one row and two columns apart is exactly 103 m
        Case("altitude exactly +103", "print", [_scene(10.25, 10.25, 12.25, 11.25)], _check_altitude(lambda a: a == 103.0, -1), hm="scene unit",
             rows=[[b"2m", PM + b"103m alt", b"<- 1599 mil", b"297" + DEG, b"1599 mil ->", b"117" + DEG]], **hm),
        Case("altitude exactly -103", "print", [_scene(12.25, 11.25, 10.25, 10.25)], _check_altitude(lambda a: a == -103.0, 1), hm="scene unit",
             rows=[[b"2m", PM + b"103m alt", b"<- 1599 mil", b"297" + DEG, b"1599 mil ->", b"117" + DEG]], **hm),
        Case("altitude 0: both ends on one texel", "print", [_scene(10.25, 10.25, 9.75, 9.75)], _check_altitude(lambda a: a == 0.0 and math.copysign(1, a) > 0, 1),
             hm="scene", rows=[[b"1m", PM + b"0m alt", b"<- 1600 mil", b"315" + DEG, b"1600 mil ->", b"135" + DEG]], **hm),
        # "scene sat": any two texels are more than 2^31 m apart; the lower saturation prints one more.  Vertical lines: d.x == 0, and
        # d.y < 0 (P1 below P0 on the screen) counts as forward
        Case("altitude saturates above, vertical down", "print", [_scene(10.25, 10.25, 10.25, 30.25)], _check_altitude(lambda a: a > 2.0 ** 31, 0, -1),
             hm="scene sat", rows=[[b"20m", PM + b"2147483647m alt", b"<- RANGE!", b"180" + DEG, b"1600 mil ->", b"0" + DEG]], **hm),
        Case("altitude saturates below, vertical up", "print", [_scene(10.25, 30.25, 10.25, 10.25)], _check_altitude(lambda a: a < -2.0 ** 31, 0, 1),
             hm="scene sat", rows=[[b"20m", PM + b"2147483648m alt", b"<- RANGE!", b"180" + DEG, b"1600 mil ->", b"0" + DEG]], **hm),
        Case("altitude saturates above, eastwards", "print", [_scene(10.25, 10.25, 40.25, 10.25)], _check_altitude(lambda a: a > 2.0 ** 31, -1),
             hm="scene sat", rows=[[b"30m", PM + b"2147483647m alt", b"<- 1600 mil", b"270" + DEG, b"RANGE! ->", b"90" + DEG]], **hm),
        Case("altitude saturates below, westwards", "print", [_scene(40.25, 10.25, 10.25, 10.25)], _check_altitude(lambda a: a < -2.0 ** 31, 1),
             hm="scene sat", rows=[[b"30m", PM + b"2147483648m alt", b"<- 1600 mil", b"270" + DEG, b"RANGE! ->", b"90" + DEG]], **hm),
    ]
    for c in out:                                                  # the 16-byte rows are the run's limit
        assert all(len(r) <= 16 for rows in c.rows for r in rows), c
    assert sum(len(r) == 16 for c in out for rows in c.rows for r in rows) == 4
    return out


# ---- bearings -------------------------------------------------------------------------------------------------------------------
def _ray(deg, length=1000.0):
    """A line whose d = P0 - P1 points at `deg` degrees: angle.to_degrees() is about deg."""
    a = math.radians(deg)
    return (length * math.cos(a), length * math.sin(a), 0.0, 0.0)


def _check_bearings(expect, degrees=None, d_exact=None):
    """The bearings, stable against an ulp of atan2f; degrees = (lo, hi): where angle.to_degrees() lies; d_exact: the value that
    reaches roundf."""
    def check(case, wants):
        assert len(wants) == len(expect)
        for (want, _), (fwd, bck) in zip(wants, expect):
            assert (float(want["bearing"][0]), float(want["bearing"][1])) == (fwd, bck), (case, want["bearing"], fwd, bck)
            assert stable_bearings(want) and mils_clear_of_ties(want), (case, want["p"])
            p0x, p0y, p1x, p1y = want["p"]
            deg = f32(R.atan2f(f32(p0y - p1y), f32(p0x - p1x)) * R.PIS_IN_180_F32)
            if degrees is not None:
                assert degrees[0] < deg <= degrees[1], (case, deg)
            if d_exact is not None:
                for s in (-10, 0, 10):                             # ... whichever neighbour of the angle the device's atan2f returns
                    a = R.atan2f(f32(p0y - p1y), f32(p0x - p1x))
                    a = np.nextafter(a, f32(s)) if s else a
                    d = f32(f32(a * R.PIS_IN_180_F32) - f32(90.0))
                    assert f32(d + f32(360.0)) == f32(d_exact), (case, d)
    return check


def _bearing_cases():
    o = 100.0
    compass = [("N", (0, -1), (0.0, 180.0)), ("NE", (1, -1), (45.0, 225.0)), ("E", (1, 0), (90.0, 270.0)), ("SE", (1, 1), (135.0, 315.0)),
               ("S", (0, 1), (180.0, 0.0)), ("SW", (-1, 1), (225.0, 45.0)), ("W", (-1, 0), (270.0, 90.0)), ("NW", (-1, -1), (315.0, 135.0))]
    # 30 px at 0.5 m/px: 15 m along an axis (1594 mil), 21.2 m along a diagonal (1591 mil); d.x >= 0 for N, S and the western three
    rows = {"N": [b"15m", b"1594 mil", b"-> 180" + DEG, b"<- 0" + DEG], "NE": [b"21m", b"1591 mil", b"-> 45" + DEG, b"<- 225" + DEG],
            "E": [b"15m", b"1594 mil", b"-> 90" + DEG, b"<- 270" + DEG], "SE": [b"21m", b"1591 mil", b"-> 135" + DEG, b"<- 315" + DEG],
            "S": [b"15m", b"1594 mil", b"-> 0" + DEG, b"<- 180" + DEG], "SW": [b"21m", b"1591 mil", b"-> 45" + DEG, b"<- 225" + DEG],
            "W": [b"15m", b"1594 mil", b"-> 90" + DEG, b"<- 270" + DEG], "NW": [b"21m", b"1591 mil", b"-> 135" + DEG, b"<- 315" + DEG]}
    out = [Case("the eight compass directions", "bearings", [(o, o, o + 30 * v[0], o + 30 * v[1]) for _, v, _ in compass],
                _check_bearings([b for _, _, b in compass]), mpx=0.5, rows=[rows[n] for n, _, _ in compass]),
           Case("the zero-length line", "bearings", [(5, 5, 5, 5)], _check_bearings([(270.0, 90.0)]), mpx=0.5, rows=[[]])]
    # 1000 px at 0.25 m/px: 250 m, 1496 mil
    head = [b"250m", b"1496 mil"]
    out += [
        Case("359.7 rounds to 360 and wraps to 0", "bearings", [_ray(89.7)], _check_bearings([(0.0, 180.0)], degrees=(89.5, 90.0)), mpx=0.25,
             rows=[head + [b"-> 180" + DEG, b"<- 0" + DEG]]),
        Case("just below 0 degrees: 269.7 is 270", "bearings", [_ray(-0.3)], _check_bearings([(270.0, 90.0)], degrees=(-0.5, 0.0)), mpx=0.25,
             rows=[head + [b"-> 90" + DEG, b"<- 270" + DEG]]),
        Case("forward 180: the back bearing is fmod(360, 360)", "bearings", [SOUTH], _check_bearings([(180.0, 0.0)]), mpx=3.0,
             rows=[[b"3m", b"1599 mil"] + ARROWS[SOUTH]]),
        # 0.5 degrees - 90 is -89.5 exactly for every angle within 3.8e-6 degrees (f32 at 90), and -89.5 + 360 is 270.5 exactly
        Case("270.5 exactly: half away from zero is 271", "bearings", [_ray(0.5)], _check_bearings([(271.0, 91.0)], d_exact=270.5), mpx=0.25,
             rows=[head + [b"-> 91" + DEG, b"<- 271" + DEG]]),
        Case("one, two and three digits", "bearings", [_ray(95.0), _ray(97.0), _ray(130.0)], _check_bearings([(5.0, 185.0), (7.0, 187.0), (40.0, 220.0)]),
             mpx=0.25, rows=[head + [b"-> 5" + DEG, b"<- 185" + DEG], head + [b"-> 7" + DEG, b"<- 187" + DEG], head + [b"-> 40" + DEG, b"<- 220" + DEG]]),
    ]
    return out


# ---- degenerate geometry the public header defines ----------------------------------------------------------------------------------
def _check_degenerate(expect):
    """expect[i] = (source, meters, (fwd, bck), texels or None): meters None = not looked at, "nan" / a float = exactly."""
    def check(case, wants):
        data, _, scale = heightmaps()[case.hm] if case.hm is not None else (None, None, None)
        assert len(wants) == len(expect)
        for (want, coords), (source, meters, bearing, tex) in zip(wants, expect):
            assert want["source"] == source, (case, want["source"])
            if meters is not None:
                assert _same_float(want["meters"], meters), (case, want["meters"])
            assert all(_same_float(float(want["bearing"][k]), bearing[k]) for k in range(2)), (case, want["bearing"])
            if tex is not None:
                assert [R.as_i32(R.round_f64(c)) for c in coords] == list(tex), (case, coords)
                assert want["alt_delta"] == R.height(data, scale[2], tex[2], tex[3]) - R.height(data, scale[2], tex[0], tex[1]), case
            assert stable_bearings(want) and mils_clear_of_ties(want), case
    return check


def _degenerate_cases():
    nan, inf = math.nan, math.inf
    two32 = 2.0 ** 32
    return [
        # a rectangle of zero width: an end point ON it has the coordinate 0 / 0 = NaN, `NaN as i32` is 0 -- column 0, inside -- and the
        # range is NaN; an end point beside it has +-inf, which saturates: outside
        Case("left == right", "degenerate", [(50, 5, 50, 9), (51, 5, 50, 9), (49, 5, 50, 9)],
             _check_degenerate([(R.HEIGHTMAP, nan, (180.0, 0.0), (0, 3, 0, 5)), (R.SCALES, None, (194.0, 14.0), None), (R.SCALES, None, (166.0, 346.0), None)]),
             mpx=2.0, minimap=(50, 50, 0, 32), hm="pow2"),
        # right < left with "fit to minimap" off: right - left wraps in u32 to 2^32 - 64, 2^32 as f32; with b0x = -16 the offset is
        # -16 * (2^32 / 16) = -2^32, the rectangle runs from -2^32 to 0 and a texel is 2^27 wide.  (A signed difference would give the
        # offset +64 and a rectangle from 128 to 0.)
        Case("right < left, the u32 wrap", "degenerate", [(-two32 + 2.5 * 2 ** 27, 16 + 3.25, -two32 + 10.25 * 2 ** 27, 16 + 4.75), (10, 19.25, 20, 19.25)],
             _check_degenerate([(R.HEIGHTMAP, None, (90.0, 270.0), (3, 3, 10, 5)), (R.SCALES, None, (90.0, 270.0), None)]),
             mpx=2.0, minimap=(64, 0, 0, 32), hm="wrap", fit=False),
        # ... and fitted: a rectangle of negative width mirrors the map
        Case("right < left, fitted", "degenerate", [(10, 5, 20, 9)], _check_degenerate([(R.HEIGHTMAP, None, (112.0, 292.0), (27, 3, 22, 5))]),
             mpx=2.0, minimap=(64, 0, 0, 32), hm="pow2"),
        Case("non-finite end points", "degenerate", [(nan, 5, 10, 9), (inf, 5, 10, 9), (10, 5, 10, -inf), (10, 5, nan, nan)],
             _check_degenerate([(R.HEIGHTMAP, nan, (nan, nan), (0, 3, 5, 5)), (R.SCALES, inf, (270.0, 90.0), None), (R.SCALES, inf, (0.0, 180.0), None),
                                (R.HEIGHTMAP, nan, (nan, nan), (5, 3, 0, 0))]),
             mpx=2.0, minimap=POW2_RECT, hm="pow2", rows=None),
        Case("non-finite end points print nothing", "degenerate", [(nan, 5, 10, 9), (inf, 5, 10, 9), (10, 5, 10, -inf)],
             _check_degenerate([(R.SCALES, nan, (nan, nan), None), (R.SCALES, inf, (270.0, 90.0), None), (R.SCALES, inf, (0.0, 180.0), None)]),
             mpx=2.0, rows=[[], [], []]),
        Case("a viewport scale of 0 means 1", "degenerate", [(5, 7, 9, 11)], _check_degenerate([(R.HEIGHTMAP, 2.0 * math.sqrt(2.0), (135.0, 315.0), (3, 4, 5, 6))]),
             mpx=2.0, minimap=POW2_RECT, hm="pow2", viewport=(0.0, 0.0, 0.0, 0.0)),
        # ... and where the label path reads it: the line and the rows of "altitude +12.6" (the print family), texels (10, 10) and (31, 51)
        Case("a viewport scale of 0 means 1, in the label too", "degenerate", [_scene(10.25, 10.25, 31.25, 51.25)],
             _check_degenerate([(R.HEIGHTMAP, math.sqrt(21.0 ** 2 + 41.0 ** 2), (153.0, 333.0), (10, 10, 31, 51))]), mpx=1.0, minimap=SCENE_RECT, hm="scene",
             viewport=(0.0, 0.0, 0.0, 0.0), rows=[[b"46m", PM + b"12m alt", b"<- 1581 mil", b"333" + DEG, b"1581 mil ->", b"153" + DEG]]),
    ]


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend(_tie_cases() + _scene_tie_cases() + _range_cases() + _print_cases() + _bearing_cases() + _degenerate_cases())
        names = [c.name for c in _CASES]
        assert len(set(names)) == len(names) and {c.family for c in _CASES} == set(FAMILIES)
    return _CASES


def expected(case):
    """What the restatements give for the case, as comparable text: per line the firing numbers and the label's rows (a mutant that
    reads past the heightmap counts as a different answer)."""
    try:
        wants = restate(case)
        rows = label_rows(case, wants)
    except IndexError:
        return "reads outside the heightmap"
    return [(w["source"], repr(float(w["meters"])), repr(float(w["alt_delta"])), [repr(round(float(m), 6)) for m in w["mils"]],
             [repr(float(b)) for b in w["bearing"]], r) for (w, _), r in zip(wants, rows)]


# ---- the batch's label path: the heightmap families on any scene's rectangle ------------------------------------------------------------
def batch_lines(rect, W, H):
    """Lines for a frame whose minimap rectangle is `rect`, under heightmaps of W x H = the rectangle's own size built by
    batch_heightmaps(): texel ties by search, altitudes that separate trunc from round and floor, and lines far enough down the
    ramp that one direction is out of range -> (lines, check(steep wants, sat wants))."""
    tie_lines, notes = rect_tie_lines(rect, W, H)
    left, _, top, _ = rect
    # short hops down the ramp of several lengths and the longest one the rectangle holds, each both ways
    fx, fy = W - 1.75, H - 1.75
    hops = []
    for k in range(1, 7):
        cx, cy = min(W - 1, k) + 0.25, min(H - 1, 7 - k) + 0.25
        hops += [(left + 0.25, top + 0.25, left + cx, top + cy), (left + cx, top + cy, left + 0.25, top + 0.25)]
    hops += [(left + 0.25, top + 0.25, left + fx, top + fy), (left + fx, top + fy, left + 0.25, top + 0.25)]
    lines = tie_lines + hops

    def check(steep, sat):
        n = len(tie_lines)
        tie_hits = sum(1 for (w, co), (ax, end, tie, c) in zip(steep[:n], notes) if co[2 * end + ax] == tie and 0 < tie)
        assert tie_hits >= 4, (rect, tie_hits)
        alts = [w["alt_delta"] for w, _ in steep if w["source"] == R.HEIGHTMAP]
        assert any(a > 1 and a % 1.0 > 0.5 for a in alts) and any(a < -1 and (-a) % 1.0 > 0.5 for a in alts), (rect, alts)
        one_sided = [w["mils"] for w, _ in steep[n:] if math.isnan(w["mils"][0]) != math.isnan(w["mils"][1])]
        assert len(one_sided) >= 2 and {math.isnan(m[0]) for m in one_sided} == {True, False}, (rect, one_sided)
        assert all(abs(w["alt_delta"]) > 2.0 ** 31 for w, _ in sat[n:]) and {w["alt_delta"] > 0 for w, _ in sat[n:]} == {True, False}
        for w, _ in steep + sat:
            assert stable_bearings(w) and mils_clear_of_ties(w) and (w["meters"] != w["meters"] or abs((w["meters"] % 1.0) - 0.5) > 1e-9), (rect, w)
    return lines, check


def batch_heightmaps(W, H):
    """-> {"steep": ..., "sat": ...} of W x H.  The steep one's z scale makes the ramp's far corner 1400 m higher than its near one:
    out of range uphill whatever the rectangle's size."""
    data = _ramp(W, H)
    span = float(data.max() - data.min())
    z = float(f32(1400.0 * 65535.0 / span * 0.1953125))
    return {"steep": (data, ((0, 0), (0, 0)), (1.0, 1.0, z)), "sat": (data, ((0, 0), (0, 0)), (1.0, 1.0, 3e38))}
