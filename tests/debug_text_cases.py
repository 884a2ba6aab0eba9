"""The cases of the debug text tests (tests/test_debug_text_host.py, tests/test_debug_text_gpu.py).  Pure numpy: nothing here
touches the library.  A drawing case is a Case: a window, a viewport (render_geometry_cases.View), the text's scale S, runs,
probe points and flags, and what it CLAIMS: runs and probe windows that lie wholly inside the window and that nothing painted
later touches -- or nothing at all: the case must change no pixel.

The minimum a claim stands for is reasoned, not measured.  A run of k characters other than the space changes at least
5 S^2 k pixels: the lightest glyph of the font but the space inks 5 font pixels ('-', '/', '^', '_', '`', '~': the host test
checks that against the font table), a font pixel is S x S window pixels when the run lies wholly inside, and the run's colour
is none the scene holds there.  A probe window wholly inside changes at least Wd Hd - 8 * 9 S * 6 S C pixels: all of it is
filled with (15, 15, 15) and the text cells -- eight lines of C characters -- are the only place where white ink can stand where
the scene was white; the provisos are that the scene holds no (15, 15, 15) pixel there and none of the swatch's colour under the
swatch.  A window partly outside is counted the same way over the part of it that is inside.  check_minimum() asserts the
provisos on the image the pass is drawn over, and that the claimed items are wholly inside and clear of each other and of
everything painted after them, all on the restatement."""
import colorsys

import numpy as np

import debug_text_ref as R
import render_geometry_cases as G

f32 = np.float32
TW, TH = 64, 32                                                  # k_debug_draw's tile
WINDOWS = ((1, 1), (255, 31), (257, 33), (515, 67), (640, 360))
INK, AMBER, MINT = (250, 1, 203, 255), (251, 180, 2, 255), (3, 252, 150, 255)   # colours no scene of the tests holds
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)


class Case:
    def __init__(self, name, window, view, S, runs=(), points=(), flags=0, claim_runs=(), claim_probes=(), nothing=False, partly_outside=False):
        self.name, self.window, self.view, self.S = name, window, view, S
        self.runs, self.points, self.flags = list(runs), list(points), flags
        self.claim_runs, self.claim_probes, self.nothing, self.partly_outside = tuple(claim_runs), tuple(claim_probes), nothing, partly_outside

    def __repr__(self):
        return "Case(%s)" % self.name


def run(x, y, text, rgba=INK, map_coords=False):
    return (float(f32(x)), float(f32(y)), tuple(rgba), R.MAP_COORDS if map_coords else 0, text if isinstance(text, bytes) else text.encode("latin-1"))


def unit_view(rw, rh):
    return G.View.direct(rw, rh, 1.0, 1.0, 0.0, 0.0)


def ink_of(text):
    return sum(1 for c in text if c not in (0x20, 0x0A))


def check_minimum(case, base, item_list, probes):
    """The case's claims on the restatement's items over `base` (the image the pass is drawn over) -> the minimum of changed
    pixels, or None for a case that must change nothing."""
    if case.nothing:
        return None
    ow, oh = case.window
    S = case.S or 2
    masks = [R.item_mask(ow, oh, it, S) for it in item_list]
    # the items of probe k: a valid probe with SMHV_DEBUG_DRAW_PROBES owns four, in list order, after the runs and the caption
    first_probe_item = len(item_list) - 4 * sum(1 for p in probes if p["valid"]) if (case.flags & R.DRAW_PROBES) else len(item_list)
    claimed, total = [], 0
    for i in case.claim_runs:
        kind, (px, py), rgb, lines = item_list[i]
        assert kind == "text" and lines == case.runs[i][4].split(b"\n")
        wide = max(len(l) for l in lines)
        assert 0 <= px and px + 6 * S * wide <= ow and 0 <= py and py + 9 * S * len(lines) <= oh, (case, "run %d is not wholly inside" % i)
        assert not (base[masks[i]][:, :3] == np.array(rgb, np.uint8)).all(axis=1).any(), (case, "the scene holds run %d's colour" % i)
        claimed.append([i])
        total += 5 * S * S * ink_of(case.runs[i][4])
    for k in case.claim_probes:
        assert probes[k]["valid"], (case, "probe %d is not valid" % k)
        j = first_probe_item + 4 * sum(1 for p in probes[:k] if p["valid"])
        kind, (ax, ay, bx, by), rgb = item_list[j]
        assert kind == "fill" and rgb == R.WINDOW_BG
        C = max(len(l) for l in item_list[j + 1][3])
        Wd, Hd = R.window_size(S, C)
        tx, ty = item_list[j + 1][1]
        cells = R.fill_mask(ow, oh, (tx, ty, tx + f32(6 * S * C), ty + f32(72 * S)))
        if not case.partly_outside:
            assert 0 <= ax and bx <= ow and 0 <= ay and by <= oh, (case, "window %d is not wholly inside" % k, ax, ay, bx, by)
            assert int(masks[j].sum()) == int(Wd) * int(Hd) and int(cells.sum()) == 8 * 9 * S * 6 * S * C
        assert not (base[masks[j]][:, :3] == np.array(R.WINDOW_BG, np.uint8)).all(axis=1).any(), (case, "the scene holds (15, 15, 15) under window %d" % k)
        assert not (base[masks[j + 2]][:, :3] == np.array(probes[k]["rgb"], np.uint8)).all(axis=1).any(), (case, "the scene holds the swatch's colour under it", k)
        claimed.append([j, j + 1, j + 2])
        total += int((masks[j] & ~cells).sum())                    # wholly inside: Wd Hd - 8 * 9 S * 6 S C
    for n, own in enumerate(claimed):
        mine = masks[own[0]]
        for j in range(own[0] + 1, len(item_list)):
            if j not in own:
                assert not (mine & masks[j]).any(), (case, "item %d paints over claimed item %d" % (j, own[0]))
        for other in claimed[:n]:
            assert not (mine & masks[other[0]]).any(), (case, "claimed items %d and %d overlap" % (other[0], own[0]))
    assert total > 0, (case, "a drawing case claims something")
    return total


# ---- text runs ------------------------------------------------------------------------------------------------------------------
def tile_cases(rw, rh):
    """S = 1 .. 4: runs whose cells straddle the tile corner (64, 32), the border x = 128 and the border y = 64, an eight-line run
    and a one-character run."""
    view = unit_view(rw, rh)
    out = []
    for S in (1, 2, 3, 4):
        runs = [run(64 - 9 * S, 32 - 4 * S, "Ag[%]"), run(128 - 3 * S, 100, "RGB {0,1}", AMBER), run(170, 64 - 5 * S, "x=\"y\" ~_^", MINT),
                run(400, 20, "1\n22\n333\n4444\n55555\n666666\n7777777\n88888888", AMBER), run(600 + S, 300, "#")]
        out.append(Case("tiles, S = %d" % S, (640, 360), view, S, runs, claim_runs=range(5)))
    return out


def edge_case(rw, rh):
    """A run cut by each edge of the window: of a row of ten 'M' cut by the left or the right edge eight are wholly inside at
    least; of two lines cut by the top or the bottom edge one is."""
    view = unit_view(rw, rh)
    ow, oh = 640, 360
    runs = [run(-10.5, 100, "MMMMMMMMMM"), run(ow - 110.25, 140, "MMMMMMMMMM", AMBER), run(200, -9.75, "WWWW\nWWWW", MINT), run(300, oh - 27.5, "WWWW\nWWWW")]
    return Case("cut by each edge", (ow, oh), view, 2, runs)


EDGE_MINIMUM = 5 * 4 * (8 + 8 + 4 + 4)                            # S = 2: the characters of edge_case that are wholly inside


def small_window_cases(rw, rh):
    """The windows at the tile's edges: one run across them (cut by the right edge where the window is narrow), S = 1."""
    view = unit_view(rw, rh)
    out = []
    for ow, oh in WINDOWS[:4]:
        runs = [run(0, 0, "@"), run(ow - 40, oh - 20, "[true, false]", AMBER)]
        if ow == 1:                                               # pixel (0, 0) lies in row 0 of the cell, above the glyph: nothing is painted
            out.append(Case("window 1 x 1", (ow, oh), view, 1, runs, nothing=True))
        else:
            out.append(Case("window %d x %d" % (ow, oh), (ow, oh), view, 1, runs, claim_runs=(0,)))
    return out


def stack_case(rw, rh, n=64):
    """All runs on one spot, the same text in n colours: the last one's colour is what every painted pixel has."""
    view = unit_view(rw, rh)
    runs = [run(60, 28, "last wins", (3 * i + 1, 255 - 3 * i, (7 * i) % 256, 255)) for i in range(n)]
    return Case("stack of %d" % n, (257, 128), view, 1, runs, claim_runs=(n - 1,))


def coords_case(rw, rh):
    """Map-coordinate and window-coordinate anchors under a zoomed viewport with a scale per axis."""
    view = G.View.direct(rw, rh, 2.5, 1.75, -100.25, -50.5)
    runs = [run(100, 60, "map (100, 60)", INK, True), run(100, 160, "window (100, 160)", AMBER, False), run(rw + 500, 10, "off the window", MINT, True)]
    return Case("map and window anchors", (640, 360), view, 2, runs, claim_runs=(0, 1))


def nothing_cases(rw, rh):
    """Anchors that are not finite, runs wholly outside the window, an empty run, no runs at all: no pixel changes."""
    view = unit_view(rw, rh)
    return [Case("anchors not finite", (515, 67), view, 1, [run(NAN, 10, "NaN"), run(10, INF, "inf"), run(-INF, NAN, "both"), run(FLT_MAX, 5, "max")], nothing=True),
            Case("a map anchor that overflows", (515, 67), G.View((0.0, 0.0, float(rw), float(rh)), (3.0e38, 1.0), (0.0, 0.0)), 1, [run(2.0, 5, "inf", INK, True)], nothing=True),
            Case("outside", (640, 360), view, 2, [run(-500, 10, "left"), run(700, 10, "right"), run(10, -100, "above"), run(10, 400, "below\nstill")], nothing=True),
            Case("empty and spaces", (640, 360), view, 3, [run(10, 10, ""), run(50, 50, "   \n \n")], nothing=True),
            Case("no runs, no probes, no flags", (640, 360), view, 0, nothing=True)]


# ---- probes ---------------------------------------------------------------------------------------------------------------------
# The GPU tests paint colours of their own on one row of the map (the threshold colours, see below), one every other column: a
# probe that is claimed looks at one of these cells, so that its swatch has a colour the scene holds nowhere else.
CELL_Y = 300


def cells(n):
    return [(50 + 2 * i, CELL_Y) for i in range(n)]


def view_at(rw, rh, cell, wx, wy, sw=1.0, sh=1.0):
    """The viewport with these scales under which the centre of map pixel `cell` lies at window position (wx, wy)."""
    return G.View.direct(rw, rh, sw, sh, wx - (cell[0] + 0.5) * sw, wy - (cell[1] + 0.5) * sh)


def probe_window_cases(rw, rh):
    """The debugger's window where it stays (15 px right of and below the point), where it flips at the right edge, at the bottom
    edge and at both, and where it lies partly outside after the flip; S = 1 (window about 226 x 106) in 640 x 360."""
    ow, oh = 640, 360
    c = cells(8)
    out = []
    for k, (name, (wx, wy), S, window, outside) in enumerate((("window stays", (40.5, 30.25), 1, (ow, oh), False), ("flips at the right edge", (450.0, 130.0), 1, (ow, oh), False),
                                                              ("flips at the bottom edge", (300.0, 340.0), 1, (ow, oh), False), ("flips at both", (500.0, 350.0), 1, (ow, oh), False),
                                                              ("partly outside after the flip", (100.0, 300.0), 2, (ow, oh), True),
                                                              ("the small windows flip always", (200.0, 20.0), 1, (257, 33), True))):
        out.append(Case(name, window, view_at(rw, rh, c[k], wx, wy), S, points=[(wx, wy)], flags=R.DRAW_PROBES, claim_probes=(0,), partly_outside=outside))
    return out


def pixel_frame_cases(rw, rh):
    """floorf(sw) = 0, 1, 2 and 3 (and another floorf(sh)): the frame snaps to the pixel grid only above 1."""
    out = []
    for k, (sw, sh) in enumerate(((0.75, 0.875), (1.5, 1.25), (2.5, 3.5), (3.25, 2.0))):
        view = view_at(rw, rh, cells(12)[8 + k], 150.75, 101.5, sw, sh)
        out.append(Case("pixel frame, floorf(sw) = %d" % int(sw), (640, 360), view, 1, points=[(150.75, 101.5)], flags=R.DRAW_PROBES, claim_probes=(0,)))
    return out


def sixteen_case(rw, rh):
    """Sixteen probes: a grid of points, some windows over each other, the last one claimed; points off the map, one at (FLT_MAX,
    FLT_MAX), one NaN (valid at map column 0, draws nothing)."""
    view = view_at(rw, rh, cells(13)[12], 30.5, 200.25)
    pts = [(20.0 + 37 * i, 15.0 + 19 * i) for i in range(12)] + [(-5000.0, 10.0), (FLT_MAX, FLT_MAX), (NAN, 50.0), (30.5, 200.25)]
    return Case("sixteen probes", (640, 360), view, 1, [run(5, 340, "runs lie under the windows")], points=pts, flags=R.DRAW_PROBES, claim_probes=(15,))


def full_case(rw, rh):
    """The longest item list there is: 64 runs, the caption (on a frame without a rectangle) and sixteen drawn probes, every one
    valid -- 129 items, both waves of the draw's compaction in use wherever windows pile up.  The last probe's window is claimed."""
    view = view_at(rw, rh, cells(14)[13], 30.5, 200.25)
    runs = [run(8 + 78 * (i % 8), 4 + 12 * (i // 8), "r%02d;" % i, (AMBER, MINT, INK)[i % 3]) for i in range(64)]
    pts = [(20.0 + 18 * i, 15.0 + 19 * i) for i in range(15)] + [(30.5, 200.25)]
    return Case("64 runs, the caption and sixteen probes", (640, 360), view, 1, runs, points=pts, flags=R.DRAW_PROBES | R.MINIMAP_CAPTION, claim_probes=(15,))


def all_cases(rw, rh):
    return (tile_cases(rw, rh) + [edge_case(rw, rh)] + small_window_cases(rw, rh) + [stack_case(rw, rh), coords_case(rw, rh)] + nothing_cases(rw, rh) +
            probe_window_cases(rw, rh) + pixel_frame_cases(rw, rh) + [sixteen_case(rw, rh), full_case(rw, rh)])


def minimum_of(case, base, item_list, probes):
    """check_minimum, and the cases whose minimum is counted by hand."""
    if case.name == "cut by each edge":
        return EDGE_MINIMUM
    return check_minimum(case, base, item_list, probes)


# ---- colours round every threshold of the marker tests --------------------------------------------------------------------------
def colour_with(h, s, v):
    """An RGB colour whose hsv() is exactly (h, s, v) by the restatement, found round the textbook conversion; None if there is none."""
    r, g, b = colorsys.hsv_to_rgb(((h + 0.5) % 360) / 360.0, min((s + 0.5) / 100.0, 1.0), min((v + 0.5) / 100.0, 1.0))
    base = [int(round(255 * c)) for c in (r, g, b)]
    best = None
    for dr in range(-3, 4):
        for dg in range(-3, 4):
            for db in range(-3, 4):
                c = (base[0] + dr, base[1] + dg, base[2] + db)
                if min(c) < 0 or max(c) > 255:
                    continue
                if R.hsv(*c) == (h, s, v):
                    d = abs(dr) + abs(dg) + abs(db)
                    if best is None or d < best[0]:
                        best = (d, c)
    return None if best is None else best[1]


def threshold_colours(consts):
    """-> [(what, (r, g, b), (h, s, v))]: for every team its hue, saturation and value windows at tolerance and tolerance + 1 on
    both sides (where the number format has such a value), the player-arc saturation branch likewise, s = 34 and 35, and black."""
    th, ts, tv = consts["FIND_MARKER_HSV_HUE_TOLERANCE"], consts["FIND_MARKER_HSV_SAT_TOLERANCE"], consts["FIND_MARKER_HSV_VIB_TOLERANCE"]
    arc, min_sat = consts["FIND_MARKER_PLAYER_DIR_ARC_SAT"], consts["FIND_MARKER_HSV_MIN_SAT"]
    out = []
    for name in R.TEAMS:
        mh, ms, mv = consts[name + "_MARKER_COLOR_HSV"]
        targets = []
        for d in (th, th + 1):
            targets += [("hue -%d" % d, (mh - d, ms, mv)), ("hue +%d" % d, (mh + d, ms, mv))]
        for d in (ts, ts + 1):
            targets += [("sat -%d" % d, (mh, ms - d, mv)), ("sat +%d" % d, (mh, ms + d, mv)),
                        ("arc sat -%d" % d, (mh, ms - arc - d, mv)), ("arc sat +%d" % d, (mh, ms - arc + d, mv))]
        for d in (tv, tv + 1):
            targets += [("value -%d" % d, (mh, ms, mv - d)), ("value +%d" % d, (mh, ms, mv + d))]
        targets += [("min sat - 1", (mh, min_sat - 1, mv)), ("min sat", (mh, min_sat, mv))]
        for what, (h, s, v) in targets:
            if not (0 <= h < 360 and 0 <= s <= 100 and 0 <= v <= 100):
                continue
            c = colour_with(h, s, v)
            assert c is not None, (name, what, h, s, v)
            out.append(("%s %s" % (name, what), c, (h, s, v)))
    out.append(("black", (0, 0, 0), (0, 0, 0)))
    return out


def probe_views(rw, rh):
    """The identity, a zoomed viewport with a scale per axis, and one with sw < 1."""
    return {"identity": unit_view(rw, rh), "zoomed": G.View.direct(rw, rh, 2.5, 1.75, -100.25, -50.5), "sw < 1": G.View.direct(rw, rh, 0.375, 1.5, 7.5, 3.25)}


def probe_points(view, rw, rh, cells):
    """Sixteen window positions at most, under `view`: the first and the last pixel of the ROI, one past each edge, negative
    inverse coordinates, NaN, (FLT_MAX, FLT_MAX), and the centres of map pixels `cells`."""
    def at(x, y):
        wx, wy = view.to_window(x, y)
        return (float(f32(wx)), float(f32(wy)))
    pts = [at(0.25, 0.25), at(rw - 0.5, rh - 0.5), at(rw + 0.25, 5.5), at(5.5, rh + 0.25), at(-0.75, 5.5), at(5.5, -0.75), (NAN, at(0, 7.5)[1]),
           (FLT_MAX, FLT_MAX), (FLT_MAX, at(0, 3.5)[1])]
    pts += [at(x + 0.5, y + 0.5) for x, y in cells]
    assert len(pts) <= R.MAX_PROBES
    return pts
