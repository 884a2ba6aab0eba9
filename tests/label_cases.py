"""The cases of the label tests (tests/test_labels_host.py, tests/test_labels_gpu.py).  Pure numpy: nothing here touches the
library.  A case is a Case: a window, a viewport (render_geometry_cases.View), the text's scale S, lines in map-ROI coordinates
with their colours, and the minimum number of pixels its labels must change on the restatement -- or None: the case must change
nothing.

The minimum is reasoned, not measured.  A label that has a range prints at least "{d}m", a mil row ("{d} mil" or "RANGE!") and
two bearing rows of at least "{d}" and the degree sign with an arrow in front or a block beside them.  The lightest glyphs that
can stand there ink 10 ('1'), 12 ('m'), 8 ('i'), 10 ('l'), 5 ('-'), 7 ('<', '>') and 8 (degree) font pixels, so the lightest
label inks 22 + 40 + 2 * 30 = 122 font pixels, 122 S^2 window pixels of area.  The hard-edged sampling of a rotated glyph keeps
its area within the pixels its outline cuts; INK = 60 S^2 per label wholly inside the window is far below that.  A label cut by
the window's edge is counted with the rows that are wholly inside, by the same figures."""
import numpy as np

import render_geometry_cases as G

f32 = np.float32
TW, TH = 64, 32                                                  # k_label_draw's tile
WINDOWS = ((1, 1), (255, 31), (257, 33), (515, 67), (640, 360))
MAGENTA, RED, CYAN = (255, 0, 255, 255), (255, 0, 0, 255), (0, 200, 255, 255)


def ink(S, labels=1):
    return 60 * S * S * labels


class Case:
    def __init__(self, name, window, view, S, lines, minimum):
        self.name, self.window, self.view, self.S, self.lines, self.minimum = name, window, view, S, lines, minimum

    def __repr__(self):
        return "Case(%s)" % self.name


def _line(view, cx, cy, angle_deg, length, rgba=MAGENTA):
    """A line whose translated midpoint is about (cx, cy) in the window, `length` window pixels long, from P0 towards P1 at
    `angle_deg` (0 = +x, 90 = +y: down) -> ((x0, y0, x1, y1) in map-ROI coordinates as f32 values, rgba)."""
    a = np.deg2rad(angle_deg)
    hx, hy = 0.5 * length * np.cos(a), 0.5 * length * np.sin(a)
    x0, y0 = view.from_window(cx - hx, cy - hy)
    x1, y1 = view.from_window(cx + hx, cy + hy)
    return (float(f32(x0)), float(f32(y0)), float(f32(x1)), float(f32(y1))), rgba


def unit_view(rw, rh):
    """Scale 1, top left 0: window coordinates are the lines' own."""
    return G.View.direct(rw, rh, 1.0, 1.0, 0.0, 0.0)


def window_cases(rw, rh):
    """Every window at the tile's edges, S = 1: labels whose midpoints lie on tile corners and borders, so their runs straddle
    up to four tiles; in the windows of 31 and 33 rows a label is cut after its third row (3 x 9 = 27 rows below a midpoint at
    y = 1), which leaves the range, the mil row and a bearing row: 22 + 40 + 30 = 92 >= ink(1)."""
    view = unit_view(rw, rh)
    out = []
    for ow, oh in WINDOWS:
        lines = []
        if (ow, oh) == (1, 1):
            lines = [_line(view, 0.5, 0.5, 0.0, 40.0)]
            minimum = 0                                          # one pixel: whether a glyph's ink lies on it is not the point; equality is
        elif oh < 40:
            lines = [_line(view, 64.0, 1.0, 0.0, 50.0), _line(view, 192.0, 1.0, 180.0, 50.0, RED)]
            minimum = ink(1, 2)
        else:
            for i, (cx, cy, ang) in enumerate(((64.0, 1.0, 0.0), (128.0, 32.0, 12.0), (256.0, 32.0, -20.0), (320.0, 2.0, 90.0), (447.9, 16.0, 171.0))):
                if cx + 80 < ow and cy + 40 < oh:
                    lines.append(_line(view, cx, cy, ang, 60.0, (MAGENTA, RED, CYAN)[i % 3]))
            if oh >= 360:
                lines += [_line(view, 192.0, 160.0, 45.0, 80.0), _line(view, 384.0, 192.0, -60.0, 80.0, RED), _line(view, 520.0, 224.0, 100.0, 30.0, CYAN)]
            minimum = ink(1, len(lines))
        out.append(Case("window %d x %d" % (ow, oh), (ow, oh), view, 1, lines, minimum))
    return out


def scale_cases(rw, rh):
    """S = 1 .. 4 in a window of 515 x 67 .. 640 x 360: one label along a slanted line at a tile corner, one hanging from a
    vertical line each way, one with d.x < 0."""
    view = unit_view(rw, rh)
    out = []
    for S in (1, 2, 3, 4):
        lines = [_line(view, 128.0, 64.0, 17.0, 90.0), _line(view, 320.0, 40.0, 90.0, 50.0, RED), _line(view, 470.0, 200.0, -90.0, 50.0, CYAN),
                 _line(view, 256.0, 200.0, 200.0, 70.0)]
        out.append(Case("S = %d" % S, (640, 360), view, S, lines, ink(S, 4)))
    return out


def outside_case(rw, rh):
    """Labels wholly outside the window: above it (the text hangs below a midpoint 200 px above the top edge, 72 S = 144 px
    tall), left of it and right of it.  Nothing changes."""
    view = unit_view(rw, rh)
    lines = [_line(view, 300.0, -200.0, 0.0, 50.0), _line(view, -400.0, 100.0, 0.0, 50.0, RED), _line(view, 1100.0, 100.0, 30.0, 50.0, CYAN)]
    return Case("outside", (640, 360), view, 2, lines, None)


def stack_case(rw, rh, n=64):
    """All extra slots on one spot: the same line n times in n colours.  The last one's colour is what every painted pixel has."""
    view = unit_view(rw, rh)
    line = _line(view, 128.0, 32.0, 8.0, 70.0)[0]
    lines = [(line, (3 * i + 1, 255 - 3 * i, (7 * i) % 256, 255)) for i in range(n)]
    return Case("stack of %d" % n, (257, 128), view, 1, lines, ink(1))


def zoom_case(rw, rh):
    """MapViewport::calc at zoom 10 with a far pan (render_geometry_cases.line_views): lines that land in the window have
    coordinates of 1.7e4 and pass through a top-left corner of -1e4."""
    view = G.line_views(rw, rh)["zoom 10, far pan"]
    ow, oh = G.WINDOW
    lines = [_line(view, 130.0, 3.0, 5.0, 120.0), _line(view, 380.0, 2.0, -7.0, 90.0, RED)]
    return Case("zoom 10", (ow, oh), view, 1, lines, ink(1, 2))


def anisotropic_case(rw, rh):
    """A scale per axis (1.43 across, 0.11 down: render_geometry_cases.matrix_views)."""
    view = G.matrix_views(rw, rh)["anisotropic"]
    ow, oh = G.WINDOW
    lines = [_line(view, 100.0, 2.0, 10.0, 80.0), _line(view, 330.0, 1.0, 160.0, 80.0, RED)]
    return Case("anisotropic", (ow, oh), view, 1, lines, ink(1, 2))


def degenerate_case(rw, rh):
    """A zero-length line, end points that are not finite, and one good line after them: only the last one has a label."""
    view = unit_view(rw, rh)
    good = _line(view, 200.0, 60.0, 25.0, 60.0, CYAN)
    lines = [((50.0, 50.0, 50.0, 50.0), MAGENTA), ((10.0, 10.0, float("inf"), 10.0), RED), ((float("nan"), 5.0, 50.0, 50.0), RED),
             ((10.0, 10.0, float("-inf"), float("inf")), RED), good]
    return Case("degenerate", (515, 67 + 60), view, 1, lines, ink(1))


def all_cases(rw, rh):
    return window_cases(rw, rh) + scale_cases(rw, rh) + [outside_case(rw, rh), stack_case(rw, rh), zoom_case(rw, rh), anisotropic_case(rw, rh),
                                                          degenerate_case(rw, rh)]


def synthetic_firing(line, view, source=1):
    """Numbers for the host tests, which have no device: plausible, from the translated line alone.  (The GPU tests feed the
    restatement the device's own numbers.)"""
    sw, sh = (float(v) for v in view.scale)
    tx, ty = (float(v) for v in view.top_left)
    with np.errstate(all="ignore"):
        p = [f32(f32(f32(line[0]) * f32(sw)) + f32(tx)), f32(f32(f32(line[1]) * f32(sh)) + f32(ty)),
             f32(f32(f32(line[2]) * f32(sw)) + f32(tx)), f32(f32(f32(line[3]) * f32(sh)) + f32(ty))]
    if not all(np.isfinite(p)):
        return {"meters": 100.0, "alt_delta": 0.0, "mils": (1000.0, 1000.0), "bearing": (float("nan"), float("nan")), "source": source}
    deg = np.degrees(np.arctan2(float(p[1]) - float(p[3]), float(p[0]) - float(p[2])))
    fwd = float(np.floor((deg - 90.0) % 360.0 + 0.5) % 360.0)
    meters = float(np.hypot(float(p[0]) - float(p[2]), float(p[1]) - float(p[3]))) * 7.3
    return {"meters": meters, "alt_delta": -12.7 if source == 2 else 0.0, "mils": (1234.5, 987.4), "bearing": (fwd, (fwd + 180.0) % 360.0),
            "source": source}
