"""Crafted decision-boundary cases of the line search (tests/test_lsd_cases_host.py, tests/test_lsd_cases_gpu.py).

A case is a named set of SEED pixels, given relative to an anchor of the map ROI.  frame(case, W, H) paints them in a marker colour
into a marker-free synthetic frame; what the search sees is the seeds after the L1 dilation (every seed becomes a plus of five
pixels, a one-pixel bar becomes three pixels thick and two longer), so the seeds are designed for the dilated mask.  The reference
mask is always the oracle's own.  Anchors: "tile" (ROI pixel (160, 160): a corner of the 32 x 8 px tiles, on the ROI's diagonal, so
that a shape that is symmetric under transposition casts mirrored rays with bit-equal lengths), the four ROI corners "tl" "tr" "bl"
"br", and "col2048" (ROI pixel (2048, 160); ultrawide only).  All cases fit the smallest ROI they are placed in (360 x 585 at
1024 x 768), so a case is the same mask at every size up to the anchor's shift.

Every case carries an expectation that tests assert on the REFERENCE (never on the device): the number of lines, the number of
rounds, and for some a check(R) of what makes the case sit on its edge (R: see Ref).  A case whose expectation fails on the oracle
is a broken case.

Families ("The line search"):
  acceptance  len² just on either side of 2500 (the bars' lengths were found on the oracle: one seed fewer and no candidate of the
              bar reaches 2500.003), along the axes, the diagonals, against the raster order (180°, 270°: a first line's band hides
              the near end of a bar, so that its first surviving candidate looks back), in the last, 16-ray unit (a first line
              that the bar's winning ray runs into, up and to the right), with ray 63 or ray 0 of a 64-ray unit as the winner
              (units 4, 7, 9 and 14), with a best len² of 2500.0 to the bit, and carried over a gap of exactly max_gap samples
              by one white sample (what sector culling rests on); small filled squares, discs and crosses, whose hundreds of
              candidates are all rejected
  gaps        dotted lines with gaps of T and T + 1 samples at max_gap = T; a fatal and a passable gap across steps 32, 64, 67
              (window radius) and 256; rays that leave the image inside a gap through the left, right and bottom edge (not the top
              one: the winning ray would have to point up from its shape's first pixel)
  ties        diagonals on the ROI's diagonal: mirrored rays in different 64-ray units with bit-equal maximal len² (the last
              one's line is the answer).  Filled squares, discs and crosses give no such tie at any size tried
  proximity   pixels at dist² 40.5 / 50 / 60.5 of an exactly diagonal line, pixels beyond a line's end (distance to the INFINITE line),
              a collinear far segment and its twin 9 px to the side
  verdict     an accepted line followed in raster order by k stubs inside its band and k outside, k = 1 .. 25; two lines
              accepted back to back
  cap         32 and 33 acceptable segments, stubs in flight behind the 32nd, the 32nd on the last word of a list segment
  storage     tile borders, the ROI's last row and column, column 2048, rays longer than 256 and 512 steps, rays leaving through
              each edge, get_centre walks that stop at an edge, more than 1024 non-zero words in front of a line
"""
import collections
import functools

import numpy as np

SMALL, HD, QHD, WIDE = (1024, 768), (1920, 1080), (2560, 1440), (3440, 1440)
SIZES = (SMALL, HD, QHD, WIDE)
ROI = {SMALL: (650, 126, 360, 585), HD: (914, 178, 986, 822), QHD: (1219, 237, 1314, 1096), WIDE: (1219, 237, 2194, 1096)}   # map_bounds; the host test checks it
ANCHORS = {"tile": lambda rw, rh: (160, 160), "tl": lambda rw, rh: (0, 0), "tr": lambda rw, rh: (rw - 1, 0),
           "bl": lambda rw, rh: (0, rh - 1), "br": lambda rw, rh: (rw - 1, rh - 1), "col2048": lambda rw, rh: (2048, 160)}
COLOURS = ((0, 255, 64, 255), (217, 117, 192, 255), (181, 232, 93, 255))      # BGRA of the three marker colours

Case = collections.namedtuple("Case", "name family anchor max_gap seeds lines rounds check rep heavy")
Ref = collections.namedtuple("Ref", "case lines rounds mask ax ay n_mask_px steps")   # lines: float32[n, 4] in ROI coordinates; mask: the oracle's lsd image


# ---- seeds ---------------------------------------------------------------------------------------------------------------------

def hbar(x0, y, n, th=1):
    return [(x0 + i, y + j) for j in range(th) for i in range(n)]


def vbar(x, y0, n, th=1):
    return [(x + j, y0 + i) for j in range(th) for i in range(n)]


def seg(x0, y0, ang, length):
    t = np.arange(0.0, length, 0.5)
    a = np.deg2rad(ang)
    p = np.stack([np.rint(x0 + np.cos(a) * t), np.rint(y0 + np.sin(a) * t)], 1).astype(int)
    return sorted(set(map(tuple, p.tolist())))


def diag(x0, y0, n, sx=1):
    return [(x0 + sx * i, y0 + i) for i in range(n)]


# ---- what the checks look at ---------------------------------------------------------------------------------------------------

def local(R):
    """The reference's lines relative to the anchor."""
    return R.lines - np.array([R.ax, R.ay, R.ax, R.ay], np.float32)


def tied_rays(R, k=0):
    """(ray indices whose len² is bit-equal to the maximum, the maximum) at line k's start, by the numpy restatement."""
    import independent_lsd as ind
    _, _, ln = ind.ray_lengths(R.mask, R.lines[k][0], R.lines[k][1], np.float32(R.case.max_gap))
    return np.nonzero(ln == ln.max())[0], ln


def raw_line(R, k=0):
    from oracle import oracle as o
    return o.find_longest_line(R.mask, float(R.lines[k][0]), float(R.lines[k][1]), float(R.case.max_gap))


def words_before(mask, x, y):
    """Non-zero 32-pixel words of the mask in raster order in front of the word that holds (x, y)."""
    h, w = mask.shape
    p = np.zeros((h, (w + 31) // 32 * 32), bool)
    p[:, :w] = mask != 0
    nz = p.reshape(h, -1, 32).any(axis=2)
    return int(nz[:y].sum() + nz[y, :x // 32].sum())


def first_pixel_of_line(R, k):
    """The candidate pixel whose get_centre is line k's start: the first white pixel in raster order that maps to it."""
    from oracle import oracle as o
    sx, sy = R.lines[k][:2]
    ys, xs = np.nonzero(R.mask[max(int(sy) - 6, 0):int(sy) + 7])
    for yy, xx in zip(ys + max(int(sy) - 6, 0), xs):
        if abs(xx - sx) <= 6 and o.get_centre(R.mask, float(xx), float(yy)) == (sx, sy):
            return int(xx), int(yy)
    raise AssertionError("no candidate maps to the start of line %d" % k)


def _looks_back(axis):
    def check(R):
        ln = local(R)
        assert ln[1][2 + axis] < ln[1][axis] - 45, ln              # the second line runs against the raster order
        raw, len2 = raw_line(R, 1)
        assert 2500 < len2 < 2605, len2                             # 51 steps: the candidate before it had exactly 50
    return check


def _winner_in(lo, hi, k=0):
    def check(R):
        w, ln = tied_rays(R, k)
        assert lo <= w[-1] <= hi, w                                  # line k's winning ray
        assert 2500 < ln.max() < 2501, ln.max()                      # on the acceptance edge
    return check


def _all_rejected_below(limit):
    def check(R):
        from oracle import oracle as o
        ys, xs = np.nonzero(R.mask)
        best = max(o.find_longest_line(R.mask, *o.get_centre(R.mask, float(x), float(y)), float(R.case.max_gap))[1] for x, y in zip(xs, ys))
        assert R.rounds == len(xs) and best < limit, (R.rounds, len(xs), best)      # every white pixel is a candidate
    return check


def _centre_on_half(R):
    """The deciding candidate's centre lies on a .5 coordinate (get_centre gives both kinds)."""
    from oracle import oracle as o
    ys, xs = np.nonzero(R.mask)
    cx, cy = R.lines[0][:2] if len(R.lines) else o.get_centre(R.mask, float(xs[0]), float(ys[0]))
    assert cx % 1 == 0.5 or cy % 1 == 0.5, (cx, cy)


def _white_on(*edges):
    """White pixels in the ROI's first / last column / row: get_centre walks from them stop at the edge, rays from them leave at once."""
    def check(R):
        m = R.mask
        for e in edges:
            assert {"left": m[:, 0], "right": m[:, -1], "top": m[0], "bottom": m[-1]}[e].any(), e
    return check


def _leaves_in_a_gap(edge):
    """The line's ray heads for `edge`, and the white pixels end 1 .. max_gap pixels short of it: the rays that go on leave the image inside a gap."""
    def check(R):
        ys, xs = np.nonzero(R.mask)
        h, w = R.mask.shape
        d = {"left": xs.min(), "right": w - 1 - xs.max(), "bottom": h - 1 - ys.max()}[edge]
        assert 1 <= d <= R.case.max_gap, d
        x0, y0, x1, y1 = R.lines[0]
        assert {"left": x1 < x0 - 40, "right": x1 > x0 + 40, "bottom": y1 > y0 + 40}[edge], R.lines
    return check


def _ends_at_origin(R):
    """max_gap = 0: a ray aborts at its first black sample and restores a position it never saved, (0, 0): every line ends at the ROI's origin."""
    assert len(R.lines) and (np.abs(R.lines[:, 2:]) < 2).all(), R.lines


def _dist2_range(lo, hi, clamped_at_least=None):
    """Some white pixel that is no part of the line lies at lo <= dist² < hi of the infinite line 0 (and, with clamped_at_least, at that
    much or more of the segment: only the distance to the infinite line hides it)."""
    def check(R):
        f32 = np.float32
        d2 = _dist2_of_white(R)
        hit = (d2 >= lo) & (d2 < hi)
        if clamped_at_least is not None:
            x0, y0, x1, y1 = (f32(v) for v in R.lines[0])
            ys, xs = np.nonzero(R.mask)
            u = np.clip(((xs - x0) * (x1 - x0) + (ys - y0) * (y1 - y0)) / ((x1 - x0) ** 2 + (y1 - y0) ** 2), 0, 1)
            hit &= (xs - (x0 + u * (x1 - x0))) ** 2 + (ys - (y0 + u * (y1 - y0))) ** 2 >= clamped_at_least
        assert hit.any(), (lo, hi)
    return check


def _white_at_local(*pts):
    def check(R):
        for (x, y) in pts:
            assert R.mask[R.ay + y, R.ax + x] == 255, (x, y)
    return check


def _longer_than(steps, k=0):
    def check(R):
        ln = R.lines[k]
        assert np.hypot(ln[2] - ln[0], ln[3] - ln[1]) > steps, ln
    return check


def _crosses_column_2048(R):
    assert R.lines[0][0] < 2040 and R.lines[0][2] > 2056, R.lines


def _both(*checks):
    def check(R):
        for c in checks:
            c(R)
    return check


def _best_is_exactly_2500(R):
    """No line, and the best len² among all the candidates is 2500.0 to the bit: `>` and `>=` part here."""
    from oracle import oracle as o
    ys, xs = np.nonzero(R.mask)
    best = max(o.find_longest_line(R.mask, *o.get_centre(R.mask, float(x), float(y)), float(R.case.max_gap))[1] for x, y in zip(xs, ys))
    assert len(R.lines) == 0 and best == np.float32(2500), best


def _ties_in_two_units(R):
    w, ln = tied_rays(R)
    assert len(set(int(i) // 64 for i in w)) >= 2, w                # several waves / lanes hold the maximum
    raw, len2 = raw_line(R)
    import independent_lsd as ind
    xe, ye, _ = ind.ray_lengths(R.mask, R.lines[0][0], R.lines[0][1], np.float32(R.case.max_gap))
    assert (raw[2], raw[3]) == (xe[w[-1]], ye[w[-1]]) and (raw[2], raw[3]) != (xe[w[0]], ye[w[0]]), (raw, w)    # the LAST maximum's end point


def _ends_near(axis, where, tol=3.0):
    def check(R):
        ln = local(R)
        assert abs(ln[0][2 + axis] - where) <= tol, (ln, where)
    return check


def _dist2_of_white(R):
    import independent_lsd as ind
    f32 = np.float32
    x0, y0, x1, y1 = (f32(v) for v in R.lines[0])
    dx, dy = f32(x1 - x0), f32(y1 - y0)
    ys, xs = np.nonzero(R.mask)
    x, y = xs.astype(f32), ys.astype(f32)
    u = ((x - x0) * dx + (y - y0) * dy).astype(f32) / f32(f32(dx * dx) + f32(dy * dy))
    ex, ey = x - (x0 + u * dx).astype(f32), y - (y0 + u * dy).astype(f32)
    return (ex * ex + ey * ey).astype(f32)


def _exact_diagonal(R):
    ln = R.lines[0]
    assert ln[0] == ln[1] and ln[2] == ln[3], ln                    # exactly 45°
    d2 = _dist2_of_white(R)
    assert (d2 == np.float32(50)).sum() >= 4 and (d2 == np.float32(40.5)).sum() >= 4 and (d2 == np.float32(60.5)).sum() >= 4, np.unique(d2[(d2 > 40) & (d2 < 61)])


def _list_segment_ends_at(k, segment):
    def check(R):
        x, y = first_pixel_of_line(R, k)
        assert words_before(R.mask, x, y) == 1024 * segment - 1, words_before(R.mask, x, y)      # line k's candidate lies on the segment's last word
    return check


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def _stubs(k, x_in, x_out, dx_out, y0):
    """k single seeds inside a vertical line's band (column x_in) and k outside (x_out, x_out + dx_out, ...), on alternating rows, every one
    more than max_gap away from all the others: in raster order a suppressed stub, then a surviving one (five candidates, all rejected)."""
    return [(x_in, y0 + 20 * j) for j in range(k)] + [(x_out + dx_out * (j % 5), y0 + 10 + 20 * j) for j in range(k)]


def _dots(T, gap, x0=-100, y=0):
    """Dashes of three seeds (five white samples) with `gap` black samples between them, 60 px or more in all."""
    period = 5 + gap
    n = max(2, -(-62 // period) + 1)
    return [(x0 + period * k + i, y) for k in range(n) for i in range(3)]


def _straddle(a, gap, tail=20, x=0, y0=-150):
    """A vertical bar from y0 whose first candidate's centre is (x, y0 + 1): white up to step a - 1, black for `gap` steps, white again."""
    cy = y0 + 1
    y1 = cy + a - 2
    y2 = cy + a + gap + 1
    return vbar(x, y0, y1 - y0 + 1) + vbar(x, y2, tail)


def _noise_columns(end_left, end_right, end_mid=None):
    """Two vertical lines, the left one with its band across a word border and the right one inside a word, and single seeds inside
    the bands from row -90 to end_left / end_right: two non-zero words and one per row that cost no round."""
    s = vbar(-128, -158, 60) + vbar(132, -158, 60)
    for r in list(range(-90, end_left, 3)) + [end_left - 1]:
        s += [(-130, r), (-126, r)]
    for r in list(range(-90, end_right, 3)) + [end_right - 1]:
        s += [(130, r), (134, r)]
    if end_mid is not None:                                          # a third line and band, inside a word
        s += vbar(42, -158, 60)
        for r in list(range(-90, end_mid, 3)) + [end_mid - 1]:
            s += [(40, r), (44, r)]
    return s


PINNED = {   # (lines, rounds) of the cases whose counts were not worked out by hand: what the oracle gave when the case was built
    "acc_exactly_2500_0": (0, 146), "acc_exactly_2500_0_longer": (1, 1), "acc_exactly_2500_1": (0, 152), "acc_exactly_2500_1_longer": (1, 1),
    "acc_exactly_2500_2": (0, 146), "acc_exactly_2500_2_longer": (1, 1),
    "acc_unit_4_ray_319_short": (0, 140), "acc_unit_7_ray_511_short": (0, 136), "acc_last_unit_short": (1, 194), "acc_last_unit": (2, 41),
    "acc_180_short": (1, 53), "acc_180": (2, 24), "acc_270_short": (1, 53), "acc_270": (2, 53),
    "acc_unit_9_ray_639_short": (0, 143),
    "acc_unit_14_ray_896_short": (0, 149), "acc_gap1_c0_dropped": (0, 154), "acc_gap1_c5_dropped": (0, 208), "acc_gap15_c0_dropped": (0, 112),
    "acc_gap15_c5_dropped": (0, 152), "acc_gap31_c0_dropped": (0, 64), "acc_gap31_c5_dropped": (0, 88), "acc_gap49_c0_dropped": (0, 13),
    "acc_gap49_c5_dropped": (0, 20), "gap_dots_0_pass": (7, 7), "gap_dots_0_fatal": (6, 6), "gap_dots_1_pass": (1, 1),
    "gap_dots_1_fatal": (0, 110), "gap_dots_15_pass": (1, 1), "gap_dots_15_fatal": (0, 44), "gap_dots_31_pass": (1, 1),
    "gap_dots_31_fatal": (0, 33), "gap_dots_32_pass": (1, 1), "gap_dots_32_fatal": (0, 33), "gap_dots_49_pass": (1, 1),
    "gap_dots_49_fatal": (0, 33), "gap_dots_50_pass": (1, 1), "gap_dots_50_fatal": (0, 33), "gap_step32_fatal": (0, 139),
    "gap_step64_fatal": (1, 1), "gap_radius67_fatal": (1, 1), "gap_step256_fatal": (1, 1), "gap_exit_bottom": (1, 1),
    "gap_exit_right": (1, 1), "acc_filled_square_int": (0, 117), "acc_filled_square_half": (0, 140), "acc_filled_disc_int": (0, 149),
    "acc_filled_disc_half": (0, 164), "acc_filled_cross_int": (0, 241), "acc_filled_cross_half": (0, 328), "prox_diag_50": (1, 49),
    "prox_beyond_end": (1, 6), "prox_band_edge": (1, 82), "cap_31": (31, 31), "st_tile_rows": (2, 2),
    "st_last_row_and_column": (2, 2), "st_first_row_and_column": (4, 4), "st_long_560": (2, 2), "st_exits_top_right": (2, 88),
    "st_exits_bottom_left": (2, 26), "st_col_2048_ends": (3, 3),
}


NOISE_CAP, NOISE_STORAGE = (108, 110), (358, 358, 359)      # tuned on the oracle's mask: see _list_segment_ends_at


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, family, seeds, lines, rounds, check=None, anchor="tile", max_gap=15, rep=False, heavy=False):
        s = np.array(sorted(set(map(tuple, seeds)), key=lambda q: (q[1], q[0])), np.int64).reshape(-1, 2)
        s.setflags(write=False)
        assert name not in [c.name for c in out], name
        if lines is None or rounds is None:
            lines, rounds = PINNED[name]
        out.append(Case(name, family, anchor, max_gap, s, lines, rounds, check, rep, heavy))

    # -- acceptance
    add("acc_h_49", "acceptance", hbar(-60, 0, 49), 0, 149)
    add("acc_h_50", "acceptance", hbar(-60, 0, 50), 1, 51, _winner_in(0, 63), rep=True)
    add("acc_h2_49", "acceptance", hbar(-60, 0, 49, 2), 0, 200)
    add("acc_h2_50", "acceptance", hbar(-60, 0, 50, 2), 1, 51, _winner_in(0, 63))
    add("acc_v_49", "acceptance", vbar(0, -60, 49), 0, 149)
    add("acc_v_50", "acceptance", vbar(0, -60, 50), 1, 1, _winner_in(832, 959))
    add("acc_v2_49", "acceptance", vbar(0, -60, 49, 2), 0, 200)
    add("acc_v2_50", "acceptance", vbar(0, -60, 50, 2), 1, 1, _winner_in(832, 959))
    add("acc_d45_34", "acceptance", diag(-30, -30, 34), 0, 104)
    add("acc_d45_35", "acceptance", diag(-30, -30, 35), 1, 1, _winner_in(384, 511))
    add("acc_d135_35", "acceptance", diag(30, -30, 35, -1), 0, 107)
    add("acc_d135_36", "acceptance", diag(30, -30, 36, -1), 1, 1, _winner_in(1280, 1407))
    band_h = [(-150 + t, -120 + int(round(t / 5.0))) for t in range(61)]
    add("acc_180_short", "acceptance", band_h + hbar(50, -80, 49), 1, None)
    add("acc_180", "acceptance", band_h + hbar(50, -80, 75), 2, None, _looks_back(0))
    band_v = [(-120 + int(round(t / 5.0)), -150 + t) for t in range(61)]
    add("acc_270_short", "acceptance", band_v + vbar(-80, 50, 49), 1, None)
    add("acc_270", "acceptance", band_v + vbar(-80, 50, 75), 2, None, _looks_back(1))
    # the winner IS a unit border's ray, on the acceptance edge (found by sweeping angle and start on the restatement): ray 63 of
    # units 4, 7 and 9, ray 0 of unit 14
    for u, ray, (x0, y0), ang, n in ((4, 319, (-120, 100), 31.75, 49), (7, 511, (-20, -20), 50.9, 49), (9, 639, (-20, -20), 63.8, 49),
                                     (14, 896, (-20, -20), 89.45, 50)):
        add("acc_unit_%d_ray_%d_short" % (u, ray), "acceptance", seg(x0, y0, ang, n - 1), 0, None)
        add("acc_unit_%d_ray_%d" % (u, ray), "acceptance", seg(x0, y0, ang, n), 1, 1, _winner_in(ray, ray))
    # the last unit (rays 3584 .. 3599): a first, vertical line above the right end of a thick bar; the bar's first candidate looks
    # right and slightly up into it
    add("acc_last_unit_short", "acceptance", hbar(-100, 0, 46, 3) + vbar(-100 + 46 + 2, -100, 100), 1, None)
    add("acc_last_unit", "acceptance", hbar(-100, 0, 47, 3) + vbar(-100 + 47 + 2, -100, 100), 2, None, _winner_in(3584, 3599, k=1))
    # segments (found by a random search on the oracle) on which some candidate's best ray has len² = 2500.0 exactly and none has more
    for k, (x0, y0, ang) in enumerate(((-5, -77, 118.4), (-94, 22, 26.4), (-100, 79, 151.8))):
        add("acc_exactly_2500_%d" % k, "acceptance", seg(x0, y0, ang, 49), 0, None, _best_is_exactly_2500)
        add("acc_exactly_2500_%d_longer" % k, "acceptance", seg(x0, y0, ang, 51), 1, None)
    # carried over a gap of exactly max_gap samples by one seed; one pixel further and nothing is a line
    for T in (1, 15, 31, 49):
        for th in (1, 2):
            s = 50 - T if T < 49 else 2                            # (T = 49: the candidate's centre lies on x.5)
            for d, tag in ((0, "carried"), (1, "dropped")):
                add("acc_gap%d_%s_%s" % (T, "c0" if th == 1 else "c5", tag), "acceptance",
                    hbar(-40, 0, s, th) + [(-40 + s + 2 + T + d, j) for j in range(th)], 1 - d, 1 if d == 0 else None,
                    _centre_on_half if th == 2 or T == 49 else None, max_gap=T)

    # -- gaps
    for T in (0, 1, 15, 31, 32, 49, 50):
        add("gap_dots_%d_pass" % T, "gaps", _dots(T, T), None, None, _ends_at_origin if T == 0 else _longer_than(60), max_gap=T)
        add("gap_dots_%d_fatal" % T, "gaps", _dots(T, T + 1), None, None, _ends_at_origin if T == 0 else None, max_gap=T)
    for a in (25, 57, 60, 249):
        name = {25: "step32", 57: "step64", 60: "radius67", 249: "step256"}[a]
        add("gap_%s_fatal" % name, "gaps", _straddle(a, 16), 0 if a == 25 else 1, None, None if a == 25 else _ends_near(1, -149 + a - 1), rep=(a == 57))
        add("gap_%s_pass" % name, "gaps", _straddle(a, 15), 1, 1, _ends_near(1, -149 + a + 15 + 20))
    add("gap_exit_left", "gaps", diag(60, 4, 56, -1), 1, 1, _both(_ends_near(0, 0, 6.0), _leaves_in_a_gap("left")), anchor="tl")
    add("gap_exit_bottom", "gaps", diag(60, -60, 56, -1), None, None, _leaves_in_a_gap("bottom"), anchor="bl")
    add("gap_exit_right", "gaps", diag(-60, -100, 56), None, None, _leaves_in_a_gap("right"), anchor="br")

    # -- ties: shapes that are symmetric under transposition, on the ROI's diagonal (the filled shapes below them belong to "acceptance":
    # hundreds of candidates, all rejected, integer and half-pixel centres)
    add("tie_diag_int", "ties", diag(-30, -30, 40), 1, 1, _ties_in_two_units, rep=True)
    add("tie_diag_half", "ties", diag(-30, -30, 40) + diag(-29, -30, 40) + diag(-30, -29, 40), 1, 1, _ties_in_two_units)
    add("tie_diag_int_58", "ties", diag(-60, -60, 58), 1, 1, _ties_in_two_units)       # three maxima: 442, 450, 458
    add("acc_filled_square_int", "acceptance", [(i, j) for i in range(-4, 5) for j in range(-4, 5)], 0, None, _all_rejected_below(2500))
    add("acc_filled_square_half", "acceptance", [(i, j) for i in range(-4, 6) for j in range(-4, 6)], 0, None, _all_rejected_below(2500))
    add("acc_filled_disc_int", "acceptance", [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j <= 36], 0, None, _all_rejected_below(2500))
    add("acc_filled_disc_half", "acceptance", [(i, j) for i in range(-6, 8) for j in range(-6, 8) if (i - .5) ** 2 + (j - .5) ** 2 <= 42], 0, None, _all_rejected_below(2500))
    add("acc_filled_cross_int", "acceptance", hbar(-20, 0, 41) + vbar(0, -20, 41), 0, None, _all_rejected_below(2500))
    add("acc_filled_cross_half", "acceptance", hbar(-20, 0, 42, 2) + vbar(0, -20, 42, 2), 0, None, _all_rejected_below(2500))

    # -- proximity
    # (a three-seed-wide diagonal of 42: the 45.0° ray alone is the longest, so the line is exactly diagonal and a pixel ten columns
    # beside it lies at dist² = 50 exactly)
    line45 = diag(-60, -60, 42) + diag(-59, -60, 42) + diag(-60, -59, 42)
    add("prox_diag_50", "proximity", line45 + [(-58 + i + 10, -58 + i) for i in range(0, 160, 20)] + [(-48 + i, -48 + i + 10) for i in range(0, 160, 20)],
        1, None, _exact_diagonal, rep=True)
    hline = hbar(-150, 0, 60)
    add("prox_beyond_end", "proximity", hline + [(-90 + 7, 0), (-90 + 5 + 20, 5), (-90 + 7 + 40, 1), (-90 + 60, -5), (-90 + 80, 6)], 1, None, _dist2_range(0, 50, clamped_at_least=50))
    add("prox_band_edge", "proximity", hline + [(-140 + 20 * j, 6 + (j % 2)) for j in range(16)] + [(-130 + 20 * j, -6 - (j % 2)) for j in range(16)], 1, None, _both(_dist2_range(40, 50), _dist2_range(50, 66)))
    add("prox_collinear", "proximity", hline + hbar(60, 0, 60), 1, 1)
    add("prox_collinear_twin", "proximity", hline + hbar(60, -9, 60), 2, 2)

    # -- verdict order
    for k in (1, 2, 4, 8, 12, 16, 24, 25):
        add("verdict_%d" % k, "verdict", vbar(0, -150, 70) + _stubs(k, 4, 24, 20, -140), 1, 1 + 5 * k)
    for k in (4, 12):
        add("verdict_two_%d" % k, "verdict", vbar(0, -150, 70) + vbar(-40, -150, 70) + _stubs(k, 4, 24, 20, -140) + _stubs(k, -44, -64, -20, -135), 2, 2 + 10 * k)

    # -- cap
    # (two columns of bars, 30 rows apart and 15 against each other: further than max_gap from one another, and outside the bands of
    # each other's infinite lines; in raster order they alternate between the columns)
    bars = lambda n: [p for i in range(n) for p in hbar((-100, 20)[i % 2], -155 + 30 * (i // 2) + 15 * (i % 2), 56)]
    add("cap_32", "cap", bars(32), 32, 32)
    add("cap_33", "cap", bars(33), 32, 32, rep=True)
    add("cap_31", "cap", bars(31), 31, None)
    add("cap_in_flight", "cap", bars(32) + [(100 + 20 * j, 310 + (3 if j % 2 else 13)) for j in range(4)] + [(110 + 20 * j, 311) for j in range(4)], 32, 32)
    add("cap_list_segment", "cap", _noise_columns(*NOISE_CAP) + bars(30), 32, 32, _list_segment_ends_at(31, 1), heavy=True)

    # -- storage
    add("st_tile_columns", "storage", vbar(-1, -60, 56) + vbar(31, -4, 56), 2, 2, _white_at_local((-1, -30), (0, -30), (31, 20), (32, 20)))
    add("st_tile_rows", "storage", hbar(-60, -1, 56) + hbar(-28, 7, 56), None, None, _white_at_local((-30, -1), (-30, 0), (0, 7), (0, 8)))
    add("st_last_row_and_column", "storage", hbar(-80, 0, 60) + vbar(0, -120, 60) + hbar(-160, -1, 56), None, None, _white_on("right", "bottom"), anchor="br")
    add("st_first_row_and_column", "storage", hbar(20, 0, 60) + vbar(0, 30, 60) + vbar(120, 0, 56) + hbar(0, 120, 56), None, None, _white_on("left", "top"), anchor="tl")
    add("st_long_300", "storage", hbar(-155, 0, 300), 1, 1, _longer_than(256))
    add("st_long_560", "storage", vbar(-100, -155, 560) + seg(-80, -150, 64.0, 600), None, None, _both(_longer_than(512, 0), _longer_than(512, 1)))
    add("st_exits_top_right", "storage", [q for q in seg(-100, 0, 20.0, 120) if q[0] <= 0] + vbar(-2, 60, 60, 3) + hbar(-60, 0, 20, 3), None, None, _white_on("top", "right"), anchor="tr")
    add("st_exits_bottom_left", "storage", [q for q in seg(100, -100, 110.0, 120) if q[1] <= 0] + hbar(0, -140, 60) + [(i, j) for i in range(4) for j in range(-3, 1)], None, None, _white_on("left", "bottom"), anchor="bl")
    add("st_list_segment", "storage", _noise_columns(*NOISE_STORAGE) + hbar(-60, 400, 56), 4, 4, _list_segment_ends_at(3, 2), heavy=True)
    for dx in (-1, 0, 1):
        add("st_col_%d" % (2048 + dx), "storage", vbar(dx, -60, 56) + hbar(-80 + dx, 40, 56), 2, 2, anchor="col2048")
    add("st_col_2048_ends", "storage", hbar(-56, 0, 56) + hbar(0, 30, 56) + hbar(-55, 60, 56), 3, None, _white_at_local((-1, 0), (0, 30), (0, 60), (1, 60)), anchor="col2048")
    add("wide_long_flat", "storage", hbar(-700, 100, 820), 1, 1, _both(_longer_than(800), _crosses_column_2048), anchor="col2048")
    add("wide_long_slanted", "storage", seg(-500, -100, 17.0, 640), 1, 1, _both(_longer_than(600), _crosses_column_2048), anchor="col2048")
    return out


FAMILIES = ("acceptance", "gaps", "ties", "proximity", "verdict", "cap", "storage")


def cases_at(size):
    """The cases a frame size carries: everything but the column-2048 cases up to 1080p; at 2560 x 1440 one representative per
    family plus all of storage and verdict order (24 frames at most); at 3440 x 1440 the column-2048 cases."""
    cs = cases()
    if size == WIDE:
        return [c for c in cs if c.anchor == "col2048"]
    cs = [c for c in cs if c.anchor != "col2048"]
    if size == QHD:
        cs = [c for c in cs if c.rep or c.family in ("storage", "verdict")]
        assert len(cs) <= 24, len(cs)
    return cs


def anchor_of(case, size):
    _, _, rw, rh = ROI[size]
    return ANCHORS[case.anchor](rw, rh)


@functools.lru_cache(maxsize=4)
def _blank(size):
    from squad_mortar_helper_amd import synth
    f, info = synth.make_frame(size[0], size[1], 7, n_lines=0)
    assert tuple(info["roi"]) == ROI[size], info["roi"]
    f.setflags(write=False)
    return f


def frame(case, W, H):
    """The BGRA frame of a case: its seeds in the marker colours (one per case, by its position in the list) over a marker-free frame."""
    x, y, rw, rh = ROI[(W, H)]
    ax, ay = anchor_of(case, (W, H))
    f = _blank((W, H)).copy()
    xs, ys = case.seeds[:, 0] + ax, case.seeds[:, 1] + ay
    assert xs.min() >= 0 and ys.min() >= 0 and xs.max() < rw and ys.max() < rh, case.name
    f[y + ys, x + xs] = COLOURS[[c.name for c in cases()].index(case.name) % 3]
    return f


def groups(size):
    """[(max_gap, [case])]: a size's cases grouped by their gap threshold (a pipeline relaunches its service per threshold)."""
    by = collections.OrderedDict()
    for c in cases_at(size):
        by.setdefault(c.max_gap, []).append(c)
    return sorted(by.items())


@functools.lru_cache(maxsize=None)
def reference(size):
    """[Ref] of cases_at(size): the oracle's record and mask of every case's frame (o.process_frame, on a few threads: the calls
    release the interpreter lock).  Shared by the tests of a session; nothing may write to it."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o
    cs = cases_at(size)

    def one(c):
        r = o.process_frame(frame(c, *size), stages=0x1, max_gap=c.max_gap, want_images=True)
        assert r["map_open"] == 1
        r["lsd"].setflags(write=False)
        ax, ay = anchor_of(c, size)
        return Ref(c, r["lines"], r["rounds"], r["lsd"], ax, ay, r["n_mask_px"], r["steps"])

    _blank(size)
    with ThreadPoolExecutor(max(1, min(os.cpu_count() or 1, len(cs), 16))) as ex:
        return tuple(ex.map(one, cs))


def check_expectation(R):
    """A case's expectation on the reference's answer R; raises AssertionError."""
    c = R.case
    assert (len(R.lines), R.rounds) == (c.lines, c.rounds), (c.name, len(R.lines), R.rounds, c.lines, c.rounds)
    if c.check is not None:
        c.check(R)
