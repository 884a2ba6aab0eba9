"""Inputs of the scale-label tests (tests/test_scale_labels_host.py, tests/test_scale_labels_gpu.py): grey images of the
bottom-right quadrant and the BGRA frames that carry them, and the label strips cut from the reference's screenshots.

A quadrant image V is uint8[qh, qw], every pixel (v, v, v):
  GREY  = 128   background: ocr_preprocess drops it (P = 255), find_scales_preprocess keeps it non-zero
  WHITE = 255   text: P != 255, foreground
  EDGE  = 150   an anti-aliased glyph edge: foreground only within three pixels of WHITE (ocr_preprocess' dilation)
  BLACK = 0     a scale bar: P = 255, find_scales_preprocess gives 0
Each case carries `expect`: what the case is there for, said of the restatement (tests/scale_labels_ref.py) by hand --
n_found, n_words, n_runs, flags, and `boxes`, the boxes of the proposals in order; test_scale_labels_host asserts it.

Frame sizes: 1024 x 768 (quadrant 180 x 292, g = 1, max_scale_y_offset 6) unless a case needs another: 1600 x 1024 (357 x
389, g = 2), 2560 x 1440 (657 x 548, g = 4) and 5120 x 2880 (quadrant wider than 1024 pixels: the second half of the device's
row).
"""
import functools
import json
import os

import numpy as np
from PIL import Image

import scale_cases as S
import scale_labels_ref as R

SMALL, MID, BIG, HUGE = (1024, 768), (1600, 1024), (2560, 1440), (5120, 2880)
GREY, WHITE, EDGE, BLACK = 128, 255, 150, 0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def geometry(size):
    """-> (rx, ry, rw, rh, qw, qh, off): the map ROI, the quadrant and max_scale_y_offset of a frame size."""
    from oracle import oracle as o
    rx, ry, rw, rh = o.map_bounds(*size)
    import scale_ref
    return rx, ry, rw, rh, rw // 2, rh // 2, scale_ref.max_scale_y_offset(rw // 2)


def blank(size):
    _, _, _, _, qw, qh, _ = geometry(size)
    return np.full((qh, qw), GREY, np.uint8)


def word(V, l, t, w, h, v=WHITE):
    V[t:t + h, l:l + w] = v
    return (l, t, l + w, t + h)


def bar(V, xl, xr, yb):
    """scale_cases.bar in BLACK: row yb from xl to xr, ticks in columns xl and xr over rows yb..yb+6."""
    V[yb, xl:xr + 1] = BLACK
    V[yb:yb + 7, xl] = BLACK
    V[yb:yb + 7, xr] = BLACK


def labelled(V, l, t, w, h, lead=2, margin=8):
    """A solid word with a scale bar `lead` rows under its bottom, from `margin` columns left of it to `margin` right of it
    -> (left, top, right, bottom, bar_left, bar_y, bar_right)."""
    box = word(V, l, t, w, h)
    xl, xr, yb = l - margin, l + w - 1 + margin, t + h + lead
    bar(V, xl, xr, yb)
    return box + (xl + 1, yb, xr - 1)


def _frame(size, paint):
    """A map-open frame whose quadrant `paint` fills (an RGB view): scale_cases' synthetic base frame (its brq-embedding helper's)
    up to 2560 x 1440, plain chrome with a red button and flat terrain at 5120 x 2880 (its generator takes a second there)."""
    rx, ry, rw, rh, qw, qh, _ = geometry(size)
    if size == HUGE:
        from oracle import oracle as o
        bx, by, bw, bh = o.button_bounds(*size)
        f = np.empty((size[1], size[0], 4), np.uint8)
        f[..., :3] = 32
        f[..., 3] = 255
        f[by:by + bh, bx:bx + bw, :3] = (49, 67, 217)
        f[ry:ry + rh, rx:rx + rw, :3] = 100
    else:
        f = S._base_frame(size, 0)[0].copy()
    q = f[ry + rh // 2:ry + rh // 2 + qh, rx + rw // 2:rx + rw // 2 + qw, :3]
    paint(q)
    return f


def frame_of(V, size):
    """The BGRA frame whose quadrant is the grey image V."""
    def paint(q):
        q[...] = V[..., None]
    return _frame(size, paint)


def closed_frame(size):
    """A frame with labelled bars in its quadrant whose button is chrome: the map is closed."""
    from oracle import oracle as o
    V = blank(size)
    labelled(V, 40, 40, 12, 6)
    f = frame_of(V, size)
    bx, by, bw, bh = o.button_bounds(*size)
    f[by:by + bh, bx:bx + bw, :3] = 32
    return f


# ---- the strips of the reference's screenshots ------------------------------------------------------------------------------
with open(os.path.join(GOLDEN, "scale_labels.json")) as _f:
    STRIPS = json.load(_f)


def strip_frame(stem):
    """A 2560 x 1440 frame with the map open whose quadrant is GREY above the strip and the screenshot's pixels from its row0."""
    rgb = np.array(Image.open(os.path.join(GOLDEN, stem + ".labels.webp")).convert("RGB"))
    row0 = STRIPS[stem]["row0"]

    def paint(q):
        q[...] = GREY
        assert q.shape[0] == row0 + rgb.shape[0] and q.shape[1] == rgb.shape[1]
        q[row0:] = rgb[..., ::-1]
    return _frame(BIG, paint)


# ---- the synthetic cases -----------------------------------------------------------------------------------------------------
def cases():
    """-> [dict(name, size, V, expect)]"""
    return list(_cases())


@functools.lru_cache(maxsize=None)
def _cases():
    out = []

    def add(name, size, V, **expect):
        V.setflags(write=False)
        out.append(dict(name=name, size=size, V=V, expect=expect))

    # -- runs and connectivity --
    # two 3 x 5 blocks g and g + 1 background columns apart, over one bar: one word, two words
    for size in (SMALL, MID, BIG):
        g = R.gap(geometry(size)[4])
        assert g == {SMALL: 1, MID: 2, BIG: 4}[size]
        for d in (g, g + 1):
            V = blank(size)
            word(V, 60, 50, 3, 5)
            word(V, 63 + d, 50, 3, 5)
            bar(V, 40, 100, 57)
            boxes = [(60, 50, 66 + d, 55)] if d == g else [(60, 50, 63, 55), (63 + d, 50, 66 + d, 55)]
            add("gap_%d_at_g%d_%dx%d" % (d, g, size[0], size[1]), size, V, n_found=len(boxes), n_words=len(boxes), n_runs=5 * len(boxes), boxes=boxes)
    # the same pair of blocks at every column from 50 to 75 and from 116 to 139 (a 64-column boundary, and every 16-column one,
    # falls inside a block, a gap, between them): a pair every second row
    for size, cols in ((SMALL, list(range(50, 76)) + list(range(116, 140))), (BIG, list(range(50, 76)) + list(range(116, 140))),
                       (HUGE, list(range(995, 1045)))):
        g = R.gap(geometry(size)[4])
        for d in (g, g + 1):
            V = blank(size)
            for k, x in enumerate(cols):
                V[10 + 2 * k, x:x + 3] = WHITE
                V[10 + 2 * k, x + 3 + d:x + 6 + d] = WHITE
            n = len(cols) * (1 if d == g else 2)
            add("sweep_gap_%d_%dx%d" % (d, size[0], size[1]), size, V, n_found=0, n_words=n, n_runs=n)
    # a word across the 1024th column of a wide quadrant, with its bar
    V = blank(HUGE)
    lb = labelled(V, 1000, 60, 50, 10, lead=3, margin=12)
    add("word_over_column_1024", HUGE, V, n_found=1, n_words=1, n_runs=10, boxes=[lb[:4]])
    # diagonal contact joins, one more column apart does not (rows differ: the smear does not reach)
    for dx, n in ((0, 1), (1, 2)):
        V = blank(SMALL)
        word(V, 20, 20, 3, 3)
        word(V, 23 + dx, 23, 3, 3)
        add("diagonal_%s" % ("touch" if n == 1 else "apart"), SMALL, V, n_found=0, n_words=n, n_runs=6)
    # a U, its bar under it: the legs meet in the last rows only
    V = blank(SMALL)
    word(V, 30, 30, 2, 12)
    word(V, 50, 30, 2, 12)
    word(V, 30, 42, 22, 2)
    bar(V, 20, 70, 46)
    add("u_shape", SMALL, V, n_found=1, n_words=1, n_runs=26, boxes=[(30, 30, 52, 44)])
    # a comb of 40 one-pixel teeth three columns apart that meet in the last row
    V = blank(SMALL)
    for k in range(40):
        V[100:120, 20 + 3 * k] = WHITE
    V[120, 20:20 + 3 * 39 + 1] = WHITE
    bar(V, 10, 150, 123)
    add("comb_40_teeth", SMALL, V, n_found=1, n_words=1, n_runs=40 * 20 + 1, boxes=[(20, 100, 138, 121)])
    # a rectangular spiral of one-pixel strokes three apart, 30 x 30
    V = blank(SMALL)
    x0, y0, x1, y1 = 40, 150, 69, 179
    while x1 - x0 >= 3 and y1 - y0 >= 3:
        V[y0, x0:x1 + 1] = WHITE
        V[y0:y1 + 1, x1] = WHITE
        V[y1, x0 + 3:x1 + 1] = WHITE
        V[y0 + 3:y1 + 1, x0 + 3] = WHITE
        x0, y0, x1, y1 = x0 + 3, y0 + 3, x1 - 3, y1 - 3
    bar(V, 30, 80, 182)
    add("spiral", SMALL, V, n_found=1, n_words=1, boxes=[(40, 150, 70, 180)])
    # a small word inside a C that it does not touch: two words, two proposals over one bar
    V = blank(SMALL)
    word(V, 30, 200, 30, 2)
    word(V, 30, 200, 2, 20)
    word(V, 30, 218, 30, 2)
    word(V, 40, 207, 6, 6)
    bar(V, 20, 70, 222)
    add("word_inside_c", SMALL, V, n_found=1, n_words=2, boxes=[(30, 200, 60, 220)])   # (the inner word's bottom is 9 rows over the bar)

    # -- box limits --
    for lo, hi, axis in ((2, 3, "w"), (128, 129, "w"), (2, 3, "h"), (32, 33, "h")):
        V = blank(SMALL)
        boxes = []
        for k, side in enumerate((lo, hi)):
            w, h = (side, 6) if axis == "w" else (10, side)
            l, t = 25, 20 + 120 * k
            lb = labelled(V, l, t, w, h, margin=12)
            if 3 <= side <= (128 if axis == "w" else 32):
                boxes.append(lb[:4])
        add("box_%s_%d_%d" % (axis, lo, hi), SMALL, V, n_found=1, n_words=2, boxes=boxes)
    _, _, _, _, qw, qh, off = geometry(SMALL)
    V = blank(SMALL)
    word(V, 0, 50, 12, 6)
    bar(V, 1, 30, 58)                                              # (a tick in column 0 is "not found": the bar starts at 1)
    add("word_at_x0", SMALL, V, n_found=1, n_words=1, boxes=[(0, 50, 12, 56)])
    V = blank(SMALL)
    word(V, qw - 12, 50, 12, 6)
    bar(V, qw - 30, qw - 1, 58)
    add("word_at_last_column", SMALL, V, n_found=1, n_words=1, boxes=[(qw - 12, 50, qw, 56)])
    V = blank(SMALL)
    lb = labelled(V, 40, 0, 12, 6)
    add("word_at_y0", SMALL, V, n_found=1, n_words=1, boxes=[lb[:4]])
    V = blank(SMALL)
    word(V, 40, qh - 6, 12, 6)
    add("word_on_last_row", SMALL, V, n_found=0, n_words=1)          # bottom == qh: the scan has no row
    V = blank(SMALL)
    labelled(V, 40, 0, 12, 3)
    add("anchor_y3", SMALL, V, n_found=0, n_words=1)                # y < 4: None
    V = blank(SMALL)
    lb = labelled(V, 40, 0, 12, 4)
    add("anchor_y4", SMALL, V, n_found=1, n_words=1, boxes=[lb[:4]])

    # -- bars --
    for lead, found in ((0, 1), (off - 1, 1), (off, 0)):
        V = blank(SMALL)
        lb = labelled(V, 40, 50, 12, 6, lead=lead)
        add("bar_%d_rows_down" % lead, SMALL, V, n_found=found, n_words=1, boxes=[lb[:4]] * found)
    for wd, found in ((9, 0), (10, 1)):                            # right - left: the ticks are width + 2 columns apart
        V = blank(SMALL)
        word(V, 42, 50, 5, 6)
        bar(V, 40, 40 + wd + 2, 58)
        add("bar_width_%d" % wd, SMALL, V, n_found=found, n_words=1, boxes=[(42, 50, 47, 56)] * found)
    V = blank(SMALL)
    word(V, 40, 50, 12, 6)
    V[58:70, 30:62] = BLACK                                          # a filled block: right = x - 1, left = x, the width wraps
    add("black_block_wraps", SMALL, V, n_found=0, n_words=1)
    V = blank(SMALL)
    word(V, 40, 50, 12, 6)
    V[49, 39:53] = EDGE                                              # anti-aliased edges: kept next to white ...
    V[50:56, 39] = EDGE
    V[50:56, 56] = EDGE                                              # ... and four columns away from it, dropped
    bar(V, 30, 70, 58)
    add("antialiased_edges", SMALL, V, n_found=1, n_words=1, boxes=[(39, 49, 53, 56)])

    # -- caps --
    V = blank(SMALL)
    boxes = []
    for row in range(3):
        for col in range(3):
            lb = labelled(V, 15 + 58 * col, 22 + 60 * row - col, 10, 6, margin=6)   # (tops fall from left to right: a row sorts right to left)
            boxes.append(lb[:4])
    boxes.sort(key=lambda b: (b[1], b[0]))
    add("nine_labels", SMALL, V, n_found=9, n_words=9, n_runs=54, boxes=boxes)
    # exactly SMHV_LABEL_MAX_RUNS runs and one more: single pixels three columns apart, one labelled word among them
    for extra, flags in ((0, 0), (1, R.RUNS_OVERFLOW)):
        V = blank(SMALL)
        lb = labelled(V, 40, 10, 12, 6)                              # 6 runs
        left = R.MAX_RUNS - 6 + extra
        y = 40
        while left:
            k = min(left, qw // 3)
            V[y, 0:3 * k:3] = WHITE
            left -= k
            y += 1
        if flags:
            add("runs_4097", SMALL, V, n_found=0, n_words=0, n_runs=R.MAX_RUNS + 1, flags=flags)
        else:
            add("runs_4096", SMALL, V, n_found=1, n_words=61, n_runs=R.MAX_RUNS, boxes=[lb[:4]])
    add("empty", SMALL, blank(SMALL), n_found=0, n_words=0, n_runs=0)
    return tuple(out)


def sizes():
    return sorted({c["size"] for c in _cases()})
