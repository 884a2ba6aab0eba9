"""The inputs of the geometry tests of the map view, the overlay and the firing solutions (tests/test_render_geometry_gpu.py and
tests/test_render_geometry_host.py): heightmaps of odd shapes and value ranges, viewports, windows at the tile's edges and
families of lines around tile borders.  Pure numpy: nothing here touches the library."""
import numpy as np

import render_ref as RR

f32 = np.float32
TW, TH = 256, 32                                                 # k_render_map's tile
WINDOW = (515, 67)                                               # 3 x 3 tiles, the last of each axis 3 px wide / high
WINDOWS = ((1, 1), (255, 31), (256, 32), (257, 33), (515, 67), (1, 70))
BG = (12, 34, 56, 255)


class View:
    """A viewport as the render options hold it: quad (left, top, right, bottom), scale (w, h), top_left (x, y)."""

    def __init__(self, quad, scale, top_left):
        self.quad = tuple(f32(v) for v in quad)
        self.scale = tuple(f32(v) for v in scale)
        self.top_left = tuple(f32(v) for v in top_left)

    @classmethod
    def direct(cls, rw, rh, sw, sh, tx, ty):
        """The map at (tx, ty), scaled by (sw, sh): scales of their own per axis."""
        sw, sh, tx, ty = f32(sw), f32(sh), f32(tx), f32(ty)
        return cls((tx, ty, tx + f32(rw) * sw, ty + f32(rh) * sh), (sw, sh), (tx, ty))

    @classmethod
    def calc(cls, *a, **k):
        return cls(*RR.viewport_calc(*a, **k))

    def to_window(self, x, y):
        return float(x) * float(self.scale[0]) + float(self.top_left[0]), float(y) * float(self.scale[1]) + float(self.top_left[1])

    def from_window(self, x, y):
        return (float(x) - float(self.top_left[0])) / float(self.scale[0]), (float(y) - float(self.top_left[1])) / float(self.scale[1])


# ---- heightmaps ----------------------------------------------------------------------------------------------------------
def _rand(seed, w, h, lo=0, hi=65536):
    return np.random.default_rng(seed).integers(lo, hi, size=(h, w), dtype=np.uint16)


def _with(data, *values):
    """`data` with the given values planted (a range that is meant to end at a value does)."""
    d = data.copy()
    flat = d.reshape(-1)
    for k, v in enumerate(values):
        flat[(7 * k + 3) % flat.size] = v
    return d


def heightmaps():
    """name -> (data uint16 [h, w], bounds ((b00, b01), (b10, b11)), covers_nothing_with_the_offset).  The bounds' offsets,
    b / (size + b) of the rectangle, are kept moderate so that SMHV_RENDER_BOUNDS_OFFSET moves the rectangle and keeps it."""
    z = (0, 0)
    return {
        "2048x3": (_rand(101, 2048, 3), ((-100, 1), z), False),
        "5x1500": (_rand(102, 5, 1500), ((1, -100), z), False),
        "1x1": (np.array([[30000]], np.uint16), ((1, 1), z), False),
        "1x9": (_rand(103, 1, 9), ((1, -2), z), False),
        "9x1": (_rand(104, 9, 1), ((-2, 1), z), False),
        "2x2": (np.array([[0, 65535], [40000, 20000]], np.uint16), ((1, 1), z), False),
        "flat": (np.full((48, 64), 4242, np.uint16), ((-15, 9), z), False),
        "two-valued": (_with(_rand(105, 64, 48, 1000, 1002), 1000, 1001), ((-15, 9), z), False),
        "narrow": (_with(_rand(106, 64, 48, 1000, 1004), 1000, 1003), ((9, -15), z), False),
        "from 0": (_with(_rand(107, 64, 48, 0, 3000), 0, 2999), ((-15, 9), z), False),
        "to 65535": (_with(_rand(108, 64, 48, 60000, 65536), 60000, 65535), ((9, -15), z), False),
        "333x97, W + b00 == 0": (_rand(109, 333, 97), ((-333, 5), z), True),
        "1024x640": (_rand(110, 1024, 640), ((-15, 9), z), False),
    }


# (lowest, highest) texel values the colour table's invariant is checked on beside the ranges of the maps above
VALUE_RANGES = ((0, 65535), (1000, 1001), (5, 5), (65534, 65535), (0, 1), (1, 65535), (0, 2), (32767, 32769))


# ---- viewports of the heightmap x form matrix (window WINDOW) ----------------------------------------------------------------
def matrix_views(rw, rh):
    """name -> View.  "panned": the map magnified 1.2 across and minified to 0.25 down, its left edge and its upper part outside the
    window: every rectangle lies partly outside, and what the code does with the width it must not do with the height.
    "anisotropic": the whole map across the window, the two scales far apart (1.43 and 0.11).  "thin": the map 14 px wide across
    the tile border at x = 256 and 59 px high -- a rectangle is a few pixels wide, with tens to hundreds of texel columns per
    pixel (the narrow scene's rectangle, 0.7 px wide, holds the pixel centre 253.5 with every offset in use)."""
    ow, oh = WINDOW
    return {
        "panned": View.direct(rw, rh, 1.2, 0.25, -40.3, -63.7),
        "anisotropic": View.direct(rw, rh, ow / rw, 0.11, 0.0, 1.3),
        "thin": View.direct(rw, rh, 0.04, 0.1, 246.1, 3.2),
    }


def window_view(rw, rh, ow, oh):
    """The whole map across a window of ow x oh (a scale per axis)."""
    return View.direct(rw, rh, ow / rw, oh / rh, 0.0, 0.0)


# ---- the staged form's footprint, restated ---------------------------------------------------------------------------------
def staged_bands(out_w, out_h, rect, W, H, lds_texels):
    """Which 4-row bands of which tiles the staged form keeps in LDS and which it gathers, from the overlay's rectangle
    (x0, y0, x1, y1, sx, sy as np.float32) -> (staged, gathered) counts over the window's tiles.  A band stages when the tile's tap
    columns times the band's tap rows fit lds_texels."""
    import overlay_ref as O
    x0, y0, x1, y1, sx, sy = rect
    staged = gathered = 0
    for tx in range(0, out_w, TW):
        xs = O.covered(out_w, x0, x1)
        xs = xs[(xs >= tx) & (xs < tx + TW)]
        if not len(xs):
            continue
        ia, ib, _, _ = O.taps(xs, x0, sx, W)
        c_w = int(max(ia.max(), ib.max()) - min(ia.min(), ib.min()) + 1)
        for by in range(0, out_h, 4):
            ys = O.covered(out_h, y0, y1)
            ys = ys[(ys >= by) & (ys < by + 4)]
            if not len(ys):
                continue
            ja, jb, _, _ = O.taps(ys, y0, sy, H)
            r_h = int(max(ja.max(), jb.max()) - min(ja.min(), jb.min()) + 1)
            if c_w * r_h <= lds_texels:
                staged += 1
            else:
                gathered += 1
    return staged, gathered


# ---- lines -------------------------------------------------------------------------------------------------------------------
OFFSETS = tuple(-1.5 + 0.25 * k for k in range(13))             # -1.5 ... +1.5 around a tile border
PAIRS = ((63, 64), (127, 128), (191, 192))                      # the last line of a wave and the first of the next
ZERO_LENGTH = (10, 70, 130, 200)
PAIR_CENTRES = ((40, 49), (110, 49), (180, 49))                 # window (x, y) where the lines of a pair cross


def border_family():
    """Strokes in window coordinates around the tile borders x in {256, 512}, y in {32, 64} of WINDOW -> list of (x0, y0, x1, y1).
    Vertical and horizontal strokes at every offset beside a border, strokes that end at every offset before and after a border,
    and diagonals that end near the four tile corners inside the window."""
    out = []
    for bx in (256, 512):
        for k, o in enumerate(OFFSETS):
            out.append((bx + o, 5 * k + 0.5, bx + o, 5 * k + 4.5))                     # beside a vertical border
            out.append((bx + o - 12.0, 3 + 5 * k, bx + o, 3 + 5 * k))                  # ends at it
    for by, xa, xe in ((32, 8, 262), (64, 270, 380)):
        for k, o in enumerate(OFFSETS):
            out.append((xa + 18 * k, by + o, xa + 18 * k + 14, by + o))                # beside a horizontal border
            out.append((xe + 9 * k, by + o - 10.0, xe + 9 * k, by + o))                # ends at it
    for cx in (256, 512):
        for cy in (32, 64):
            for (dx, dy), (ux, uy) in (((-0.75, -0.75), (-15, -12)), ((0.6, -0.4), (14, -11)), ((0.3, 0.3), (13, 12)), ((-0.2, 0.9), (-12, 14))):
                out.append((cx + dx + ux, cy + dy + uy, cx + dx, cy + dy))             # a diagonal that ends near a tile corner
    return out


def line_list(view, seed=9):
    """256 lines in map-ROI coordinates (float32 [256, 4]) that `view` brings to: the border family, three pairs of crossing lines
    at the indices PAIRS, lines of zero length at ZERO_LENGTH, and short random lines; the order is shuffled, so every tile's list
    holds lines of all four waves.  -> (lines, indices of the border family)."""
    rng = np.random.default_rng(seed)
    fam = border_family()
    n_fill = 256 - len(fam) - 2 * len(PAIRS) - len(ZERO_LENGTH)
    assert n_fill > 0
    fill = []
    for _ in range(n_fill):
        x, y = rng.uniform(265.0, 500.0), rng.uniform(2.0, 28.0)
        a, ln = rng.uniform(0.0, 2 * np.pi), rng.uniform(3.0, 25.0)
        fill.append((x, y, x + ln * np.cos(a), y + ln * np.sin(a)))
    fixed = {}
    for (i, j), (cx, cy) in zip(PAIRS, PAIR_CENTRES):
        fixed[i] = (cx - 15, cy - 9, cx + 15, cy + 9)
        fixed[j] = (cx - 15, cy + 9, cx + 15, cy - 9)
    for i in ZERO_LENGTH:
        fixed[i] = (300.0 + i, 20.0, 300.0 + i, 20.0)
    rest = [("fam", l) for l in fam] + [("fill", l) for l in fill]
    order = rng.permutation(len(rest))
    lines, fam_idx, k = [], [], 0
    for i in range(256):
        if i in fixed:
            w = fixed[i]
        else:
            kind, w = rest[order[k]]
            k += 1
            if kind == "fam":
                fam_idx.append(i)
        x0, y0 = view.from_window(w[0], w[1])
        x1, y1 = view.from_window(w[2], w[3])
        lines.append((x0, y0, x1, y1))
    assert k == len(rest)
    lines = np.array(lines, np.float32)
    for i in ZERO_LENGTH:
        lines[i, 2:] = lines[i, :2]
    return lines, fam_idx


NON_FINITE = (([10, 10, np.inf, 10], 33835), ([10, 10, -np.inf, 300], 670), ([10, 10, np.inf, np.inf], 0), ([np.nan, 5, 50, 50], 0))


def tile_of(x, y):
    return int(np.floor(x / TW)), int(np.floor(y / TH))


def check_line_family(lines, fam_idx, view, out_w, out_h):
    """What a line list must do in the restatement for a comparison on it to mean something -> the lines' masks.  Every finite line
    of non-zero length with an end point inside the window paints at least one pixel; at least one stroke of the border family
    whose end points lie in one tile paints a pixel of another tile (the cull has to keep it there: its bounding box alone does
    not reach that tile's pixel centres without the margin)."""
    masks, crossing = [], 0
    for i, ln in enumerate(lines):
        m = RR.line_mask(out_w, out_h, ln, view.scale, view.top_left)
        masks.append(m)
        if not np.all(np.isfinite(ln)) or (ln[0] == ln[2] and ln[1] == ln[3]):
            continue
        p = [view.to_window(ln[0], ln[1]), view.to_window(ln[2], ln[3])]
        if any(1.0 <= x <= out_w - 1.0 and 1.0 <= y <= out_h - 1.0 for x, y in p):
            assert m.any(), (i, ln.tolist(), p)
        if i in fam_idx and tile_of(*p[0]) == tile_of(*p[1]):
            ys, xs = np.nonzero(m)
            crossing += any(tile_of(x, y) != tile_of(*p[0]) for x, y in zip(xs, ys))
    assert crossing >= 8, crossing
    return masks


def check_pairs(want, masks, n):
    """The crossing of each pair of PAIRS belongs to the pair's second line, the first line of the next wave: both paint the
    pixel, and no later line does."""
    for (i, j), (cx, cy) in zip(PAIRS, PAIR_CENTRES):
        assert masks[i][cy, cx] and masks[j][cy, cx] and not any(m[cy, cx] for m in masks[j + 1:]), (i, j)
        assert np.array_equal(want[cy, cx], RR.line_color(j, n)), (i, j, want[cy, cx].tolist())


def line_views(rw, rh):
    """The viewports of the line tests (window WINDOW): the identity, where window coordinates are the lines' own, and
    MapViewport::calc at zoom 10 with a pan of tens of thousands of map pixels: lines that land in the window then have
    coordinates of 1.7e4 and pass through a top-left corner of -1e4, where an f32's last place is 1e-3 px."""
    ow, oh = WINDOW
    return {"identity": View(*RR.identity(rw, rh)), "zoom 10, far pan": View.calc(ow, oh, rw, rh, 10, (0.5, 0.45), (-88000.0, -87000.0))}


# ---- what a case must change for its comparison to mean something ------------------------------------------------------------------
# A case whose overlay covers nothing proves nothing, so every (scene, heightmap, viewport, fit) case asserts, on the
# restatement, a minimum number of pixels that differ from the same render without the heightmap.  The figures were chosen on
# the CPU from the restatement: four fifths of the smallest count over the heightmaps and both settings of the offset, per scene
# (the nine open scenes in order).  The narrow and the flat scene are 17 px wide and 13 px high, and the "thin" view is the
# one that makes a rectangle a few pixels wide, so their figures are small where that is the point of the case.  0 declares a
# case that covers nothing: it asserts equality instead.
MATRIX_MIN = {
    "panned": (7615, 4121, 6587, 448, 305, 1417, 10022, 2324, 9651),
    "anisotropic": (4139, 2528, 4793, 288, 182, 1857, 6784, 1188, 6348),
    "thin": (110, 62, 100, 21, 5, 45, 168, 22, 162),
}
# The windows, with the "to 65535" map (bounds (9, -15): the offset moves the left edge right by 9 / 73 of the width and the top
# edge up by 15 / 33 of the height) and the whole map across the window, without lines -> per fit_to_minimap, per scene.  Declared
# as covering nothing: the flat scene at 256 x 32 without the offset (its 13 rows lie between two pixel centres), and the scene
# that hugs the centre on the left in the one-pixel-wide windows with the offset (the window's column shows the ROI's centre
# column, 3 px inside the rectangle; the offset moves the edge 18 px).
WINDOW_MAP = "to 65535"
WINDOW_MIN = {
    (1, 1): {True: (1, 1, 1, 1, 1, 1, 1, 1, 1), False: (1, 0, 1, 1, 1, 1, 1, 1, 1)},
    (255, 31): {True: (3940, 2419, 4388, 268, 180, 1865, 6299, 1085, 6100), False: (3875, 2256, 4588, 240, 157, 2232, 5530, 1428, 5332)},
    (256, 32): {True: (4118, 2505, 4579, 278, 0, 1704, 6528, 1176, 6323), False: (4036, 2356, 4736, 272, 158, 2244, 5734, 1513, 5529)},
    (257, 33): {True: (4298, 2616, 4748, 288, 181, 1874, 6758, 1267, 6547), False: (4176, 2432, 4910, 256, 159, 2393, 5913, 1582, 5728)},
    (515, 67): {True: (17236, 10289, 19471, 1171, 364, 7532, 27550, 5068, 25792), False: (17080, 9779, 20046, 1092, 638, 9600, 24172, 6403, 22967)},
    (1, 70): {True: (45, 49, 47, 51, 1, 18, 56, 26, 54), False: (51, 0, 56, 54, 1, 26, 56, 38, 55)},
}


def changed(a, b):
    return int(np.any(a != b, axis=2).sum())


def assert_changes(want, base, minimum, ctx):
    """The honesty condition of one case: `want` (with the heightmap) against `base` (without), both the restatement's."""
    n = changed(want, base)
    if minimum == 0:
        assert n == 0, (ctx, "declared as covering nothing", n)
    else:
        assert n >= minimum, (ctx, n, minimum)
    return n
