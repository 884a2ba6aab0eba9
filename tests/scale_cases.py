"""Inputs of the scale-bar tests (tests/test_scale_host.py, tests/test_scale_gpu.py): scales images of the bottom-right
quadrant (uint8; 255 background, 0 black) with label anchors (meters, x, y), and the BGRA frames that carry them.

Three sets:
  fixed_cases(W, H)   one image + one anchor each, aimed at the places where the device's scan (csrc/smh_record.inc: rows by
                      ballot, 256 columns per step in four clamped chunks of 64) can go wrong; NONE_NAMES says by hand which
                      of them the reference answers with None
  ladder()            three bars in one image whose mean depends on the order of the sum, and every success / failure
                      outcome of two and of three anchors
  random_images()     noisy images with broken and unbroken bars, forty anchors each

Frame sizes: 2560 x 1440 (quadrant 657 x 548, max_scale_y_offset 21: the smallest common size at which a tick can lie beyond
the second and third 256-column step) and 1024 x 768 (quadrant 180 x 292, offset 6: every search is one partial step).
"""
import functools

import numpy as np

import scale_ref as R

BIG, SMALL = (2560, 1440), (1024, 768)
QUADRANT = {BIG: (657, 548), SMALL: (180, 292)}            # (rw // 2, rh // 2) of map_bounds; test_scale_host checks it
DISTANCES = {BIG: (1, 5, 6, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 319, 320, 511, 512, 513, 600),
             SMALL: (1, 5, 6, 62, 63, 64, 65, 66, 127, 128, 129, 150)}
YB = 100                                                    # the bar's row where a case has no reason for another


def blank(size):
    qw, qh = QUADRANT[size]
    return np.full((qh, qw), 255, np.uint8)


def bar(img, xl, xr, yb):
    """A scale bar as the game draws it: row yb black from xl to xr, ticks in columns xl and xr over rows yb..yb+6 (clipped
    at the bottom of the image)."""
    if yb < img.shape[0]:
        img[yb, xl:xr + 1] = 0
    img[yb:yb + 7, xl] = 0
    img[yb:yb + 7, xr] = 0
    return img


def fixed_cases(size):
    """-> [dict(name, img, anchor=(meters, x, y))]; cases that share an image share the array object."""
    return list(_fixed_cases(size))


@functools.lru_cache(maxsize=None)
def _fixed_cases(size):
    w, h = QUADRANT[size]
    off = R.max_scale_y_offset(w)
    lead = min(6, off - 1)                                  # rows from the anchor down to the bar
    cases = []

    def add(name, img, x, y):
        img.setflags(write=False)
        cases.append(dict(name=name, img=img, anchor=(100 + 7 * len(cases), x, y)))

    # the tick's distance from the anchor, to the right (anchor at 20, left tick at 8) and to the left (anchor at w - 20,
    # right tick at w - 8)
    for d in DISTANCES[size]:
        add("dist_right_%d" % d, bar(blank(size), 8, 20 + d, YB), 20, YB - lead)
    for d in DISTANCES[size]:
        add("dist_left_%d" % d, bar(blank(size), w - 20 - d, w - 8, YB), w - 20, YB - lead)
    # the image's first and last column
    add("left_tick_col0", bar(blank(size), 0, 60, YB), 30, YB - lead)
    add("left_tick_col1", bar(blank(size), 1, 60, YB), 30, YB - lead)
    add("right_tick_last_col", bar(blank(size), w - 60, w - 1, YB), w - 30, YB - lead)
    add("anchor_x0", bar(blank(size), 0, 40, YB), 0, YB - lead)
    img = bar(blank(size), w - 40, w - 1, YB)
    add("anchor_x_last", img, w - 1, YB - lead)
    add("anchor_x_width", img, w, YB - lead)
    # the anchor on a tick
    img = bar(blank(size), 30, 90, YB)
    add("anchor_on_right_tick", img, 90, YB - lead)
    add("anchor_on_left_tick", img, 30, YB - lead)
    img = bar(blank(size), 30, 90, YB)
    img[YB:YB + 7, 89] = 0
    add("anchor_on_two_wide_tick", img, 90, YB - lead)       # right = 89, left = 90: the width wraps to 0xFFFFFFFF
    add("all_black", np.zeros((h, w), np.uint8), 50, 50)
    add("all_white", blank(size), 50, 50)
    # a stub hanging from the bar between the anchor and the tick: three rows are walked past, four rows are a tick
    for rows in (3, 4):
        img = bar(blank(size), 30, 120, YB)
        img[YB:YB + rows, 100] = 0
        add("stub_%d_rows" % rows, img, 60, YB - lead)
    # MIN_SCALE_WIDTH: a bar of width 9, 10, 11 (right - left: the ticks are width + 2 columns apart) and a wider one five rows lower
    lead_w = min(6, off - 6)
    for wd in (9, 10, 11):
        img = bar(bar(blank(size), 20, 140, YB + 5), 50, 50 + wd + 2, YB)
        add("width_%d" % wd, img, 55, YB - lead_w)
    # the bar in the last two searched rows and in the first two rows that are not searched
    for k in (off - 2, off - 1, off, off + 1):
        add("bar_%s_rows_down" % {off - 2: "off-2", off - 1: "off-1", off: "off", off + 1: "off+1"}[k], bar(blank(size), 30, 90, YB), 60, YB - k)
    # the bottom of the image: the ticks need four rows
    shared = None
    for k in (5, 4, 3, 1):
        img = bar(blank(size), 30, 90, h - k)
        add("bar_at_h-%d" % k, img, 60, h - k - lead)
        if k == 4:
            shared = img
    add("anchor_y_h-4", shared, 60, h - 4)
    add("anchor_y_h", shared, 60, h)
    # the top of the image and an anchor row whose sum with the offset wraps
    img = bar(blank(size), 30, 90, 8)
    add("anchor_y3", img, 60, 3)
    add("anchor_y4", img, 60, 4)
    add("anchor_y_0xFFFFFFF0", img, 60, 0xFFFFFFF0)
    # a stray black pixel in the anchor column one row down, with a four-row run on one side of it only: that row fails,
    # the bar further down is the answer
    for side, col in (("right", 80), ("left", 45)):
        img = bar(blank(size), 30, 120, YB)
        img[YB - lead + 1, 60] = 0
        img[YB - lead + 1:YB - lead + 5, col] = 0
        add("stray_pixel_run_%s" % side, img, 60, YB - lead)
    img = bar(blank(size), 30, 120, YB)
    img[YB - lead:YB - lead + off - 1, 60] = 0
    add("anchor_column_black", img, 60, YB - lead)
    return tuple(cases)


# Which fixed cases the reference answers with None, by hand from mpx_ratio.rs (the names are the same at both sizes).
NONE_NAMES = frozenset((
    "left_tick_col0",            # left == 0 is "not found" (mpx_ratio.rs:53)
    "anchor_x0",                 # (0..0).rev() is empty: left stays 0
    "anchor_x_width",            # defined: x >= width
    "anchor_on_left_tick",       # the tick is found going right; nothing lies to the left of it
    "all_white",
    "bar_off_rows_down",         # y..min(h, y + off) excludes row y + off
    "bar_off+1_rows_down",
    "bar_at_h-3",                # the tick test reads rows h-3..h: one below the image
    "bar_at_h-1",
    "anchor_y_h",                # y..min(h, ..) is empty
    "anchor_y3",                 # y < MIN_SCALE_VERTICAL_BAR_HEIGHT
    "anchor_y_0xFFFFFFF0",       # y + off wraps to a small number: an empty range
))


def expected_bar(size, case):
    """(left, y, right) of some fixed cases, worked out by hand; None where this table has no entry (NONE_NAMES says whether
    the case succeeds at all)."""
    w, h = QUADRANT[size]
    lead = min(6, R.max_scale_y_offset(w) - 1)
    name, (_, x, y) = case["name"], case["anchor"]
    if name.startswith("dist_right_"):
        return (9, YB, 19 + int(name.rsplit("_", 1)[1]))
    if name.startswith("dist_left_"):
        return (w - 19 - int(name.rsplit("_", 1)[1]), YB, w - 9)
    return {"left_tick_col1": (2, YB, 59), "right_tick_last_col": (w - 59, YB, w - 2), "anchor_x_last": (w - 39, YB, w - 2),
            "anchor_on_right_tick": (31, YB, 89), "anchor_on_two_wide_tick": (90, YB, 89), "all_black": (50, 50, 49),
            "stub_3_rows": (31, YB, 119), "stub_4_rows": (31, YB, 99), "width_9": (21, YB + 5, 139), "width_10": (51, YB, 61),
            "width_11": (51, YB, 62), "bar_off-2_rows_down": (31, YB, 89), "bar_off-1_rows_down": (31, YB, 89),
            "bar_at_h-5": (31, h - 5, 89), "bar_at_h-4": (31, h - 4, 89), "anchor_y_h-4": (31, h - 4, 89), "anchor_y4": (31, 8, 89),
            "stray_pixel_run_right": (31, YB, 119), "stray_pixel_run_left": (31, YB, 119)}.get(name)


LADDER_METERS = (3, 77, 7)
LADDER_WIDTHS = (11, 198, 548)
LADDER_MEAN = 0.2247966280812996                            # ((3/11 + 77/198) + 7/548) / 3; every other order of the sum ends in ...963


@functools.lru_cache(maxsize=None)
def ladder():
    """-> (img, calls): three bars of width 11, 198, 548 in row bands of their own (2560 x 1440 quadrant); calls = the anchor
    lists of all eight outcomes of three anchors and all four of two, a failing anchor being one moved to y = 3."""
    img = blank(BIG)
    anchors = []
    for k, (m, wd) in enumerate(zip(LADDER_METERS, LADDER_WIDTHS)):
        yb = 100 + 100 * k
        bar(img, 30, 30 + wd + 2, yb)
        anchors.append((m, 36 + 3 * k, yb - 6))
    img.setflags(write=False)
    calls = []
    for n in (3, 2):
        for mask in range(1 << n):
            calls.append([(m, x, y if mask >> i & 1 else 3) for i, (m, x, y) in enumerate(anchors[:n])])
    return img, calls


N_RANDOM, N_ATTEMPTS = 12, 40


@functools.lru_cache(maxsize=None)
def random_images():
    """-> [(img, [(meters, x, y)] * 40)] * 12 in the 2560 x 1440 quadrant, and the set's statistics on the restatement
    (share of successes, distinct widths) -- asserted here, so that the set cannot quietly degenerate."""
    w, h = QUADRANT[BIG]
    rng = np.random.default_rng(1)
    out = []
    for _ in range(N_RANDOM):
        img = blank(BIG)
        img[rng.random((h, w)) < 0.02] = 0
        for _ in range(120):
            x, y0, n = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(2, 9))
            img[y0:y0 + n, x] = 0
        anchors = []
        for _ in range(N_ATTEMPTS):
            xl = int(rng.integers(0, w - 8))
            xr = min(xl + int(rng.integers(8, 501)), w - 1)
            yb = int(rng.integers(8, h))
            if rng.random() < 0.7:
                img[yb, xl:xr + 1] = 0
            for col in (xl, xr):
                if rng.random() < 0.8:
                    img[yb:yb + int(rng.integers(3, 8)), col] = 0
            ax = int(rng.integers(xl, xr + 1))
            ay = max(yb - int(rng.integers(0, 24)), 0)
            anchors.append((int(rng.integers(1, 1000)), ax, ay))
        img.setflags(write=False)
        out.append((img, anchors))
    found, widths = 0, set()
    for img, anchors in out:
        rows = img.tolist()
        for (m, x, y) in anchors:
            r = R.find_scale_width(m, x, y, rows)
            if r is not None:
                found += 1
                widths.add((r[1][2] - r[1][0]) % (1 << 32))
    share = found / float(N_RANDOM * N_ATTEMPTS)
    assert 0.3 <= share <= 0.7, share
    assert len(widths) >= 64, len(widths)
    return out, dict(anchors=N_RANDOM * N_ATTEMPTS, found=found, share=share, distinct_widths=len(widths))


@functools.lru_cache(maxsize=4)
def _base_frame(size, idx):
    from squad_mortar_helper_amd import synth
    f, info = synth.make_frame(size[0], size[1], idx, n_lines=2)
    f.setflags(write=False)
    return f, info["roi"]


def frame_of(img, size, idx=0):
    """The BGRA frame whose find_scales_preprocess image is `img`: a synthetic frame (terrain and two marker lines, so that
    the line search does real work before the record is written), its bottom-right quadrant painted mid-grey, (0, 0, 0)
    wherever img is 0."""
    base, (x, y, rw, rh) = _base_frame(size, idx % 3)
    qh, qw = img.shape
    assert (qw, qh) == (rw // 2, rh // 2) == QUADRANT[size]
    f = base.copy()
    q = f[y + rh // 2:y + rh // 2 + qh, x + rw // 2:x + rw // 2 + qw, :3]
    q[...] = 128
    q[img == 0] = 0
    return f
