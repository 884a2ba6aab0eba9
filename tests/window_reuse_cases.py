"""Crafted masks for the search service's window reuse (tests/test_window_reuse_host.py, tests/test_window_reuse_gpu.py), in the style of
tests/lsd_cases.py, whose frame builder, ROI table, anchors and colours these use.

A wave of k_lsd_service keeps its candidate window from one candidate to the next (smh_lsd_wave.inc, WinTag; k_lsd_service_c, the
kernel of the sizes above 1080p, fills for every candidate and runs the same cases): a window filled for the
candidate at (px, py) lies at word column floor((px - 67) / 32) and row py - 67, is 6 words wide and 135 + E rows tall, and serves a
later candidate of the same frame while it contains [px - 67, px + 67] x [py - 67, py + 67] (csrc/smh_window_place.h; model() below is
the same rule in Python, and the host test holds its constants against the header).  A wrong reuse shows only where the candidate's
verdict rests on mask words OUTSIDE the stale window, so every case ends in a PROBE: a bar of 70 px, accepted as a line, whose first
candidate -- the first pixel of its dilated top row -- sits at a chosen offset from the fill before it.  In front of the probe in raster
order lie DOTS: single seeds, five rejected candidates each, more than max_gap samples from everything else.  Read through a window
that does not hold it the probe loses its line (the words beyond the window are not its mask), or `rounds` moves.

Every case carries what the oracle must say (lines, and the line's first pixel) and what model() must say about the probe's candidate
for E = 0 and for the E the library was built with: True (a fill), False (reuse), or None (not pinned); asserted on the CPU by the host
test before anything runs on a device.

  a  same-row word crossing    dots on one row stepping right, the probe at the last pixel that may reuse, the first that may not, and a
                               word further on
  b  next row further left     the row below starts LEFT of the stored columns
  c  row limits                the probe (a bar pointing DOWN: its rays read the window's last rows) k rows below the dot's first fill,
                               k around every E a build may choose (0, 8, 16, 24), and far below
  d  borders                   dots and probes within 67 px of each border: negative placements (px < 67, py < 67), columns and rows
                               beyond the image
  e  stale across frames       two masks with the same blob, one with a continuation of the blob 10 px to its right that makes it a
                               line: alternated within a submission, order swapped every time.  e_first_*: the blob alone, so that it is
                               the frame's FIRST candidate and lies inside the window the wave's last frame left behind (the OWNER's tag);
                               e_blob_*: behind a block of rejected candidates, so that the frame has asked for help when the scan
                               reaches the blob (a HELPER's tag)
  f  helpers                   a heavy frame (a few hundred rejected candidates in two bands, then probes) among light ones
"""
import collections
import functools
import os
import re

import numpy as np

import lsd_cases as C

R, WORDS, BASE_ROWS = 67, 6, 135
E_CHOICES = (0, 8, 16, 24)
SIZES = (C.SMALL, C.QHD)                                                   # the smallest size lsd_cases uses, and one behind the compact index (k_lsd_service_c)
MAX_GAP = 15

Case = collections.namedtuple("Case", "name family anchor seeds lines probe fill_e0 fill_built")
Ref = collections.namedtuple("Ref", "case lines rounds n_mask_px steps mask")


# ---- the rule, as the device applies it ----------------------------------------------------------------------------------------

def fresh(px, py):
    return (px - R) >> 5, py - R                                           # (Python's >> floors, as the device's arithmetic shift does)


def holds(x0w, y0, rows, px, py):
    return x0w * 32 <= px - R and px + R <= x0w * 32 + 32 * WORDS - 1 and y0 <= py - R and py + R <= y0 + rows - 1


def model(pixels, extra):
    """[(px, py)] in the order ONE wave casts them within a frame -> [True where the window is filled]."""
    tag, out = None, []
    for px, py in pixels:
        if tag is not None and holds(tag[0], tag[1], BASE_ROWS + extra, px, py):
            out.append(False)
        else:
            tag = fresh(px, py)
            out.append(True)
    return out


def header_constants():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "squad-mortar-helper_amd", "csrc", "smh_window_place.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (SMH_WIN_R|SMH_WIN_WORDS) (\d+)", src)}


def built_extra():
    """E of k_lsd_service as the sources set it (SVC_WIN_EXTRA in smh_lsd_seq.inc)."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "squad-mortar-helper_amd", "csrc", "smh_lsd_seq.inc")).read()
    got = re.findall(r"#define SVC_WIN_EXTRA (\d+)u", src)
    assert len(got) == 1, got
    return int(got[0])


def visited(mask, max_gap=MAX_GAP):
    """The pixels the sequential scan casts, in order, with their verdicts: [(px, py, accepted)] (tests/independent_lsd.py's loop)."""
    import independent_lsd as I
    f32 = np.float32
    lines, out = [], []
    ys, xs = np.nonzero(mask == 255)
    for yy, xx in zip(ys.tolist(), xs.tolist()):
        if any(I._near(f32(xx), f32(yy), ln) for ln in lines):
            continue
        cx, cy = I.get_centre(mask, f32(xx), f32(yy))
        line, length = I.find_longest_line(mask, cx, cy, f32(max_gap))
        ok = bool(length > f32(2500))
        if ok:
            ex, ey = I.get_centre(mask, line[2], line[3])
            lines.append(np.array([line[0], line[1], ex, ey], f32))
        out.append((xx, yy, ok))
        if len(lines) == 32:
            break
    return out


# ---- seeds (ROI coordinates relative to the anchor; a seed becomes a plus of five pixels) -----------------------------------------

def dot(x, y):
    return [(x, y)]


def probe_right(x, y, n=70):
    """A bar to the right whose first candidate is (x, y): seeds one row below (the dilated top row starts at the first seed's column)."""
    return C.hbar(x, y + 1, n)


def probe_down(x, y, n=70):
    return C.vbar(x, y + 1, n)


def _squares(x0, y0, nx, dx):
    return [(x0 + i * dx + a, y0 + b) for i in range(nx) for a in (0, 1) for b in (0, 1)]


def _case(name, family, anchor, seeds, lines, probe, e0=None, built=None):
    return Case(name, family, anchor, np.array(sorted(set(seeds)), int).reshape(-1, 2), lines, probe, e0, built)


@functools.lru_cache(maxsize=1)
def cases():
    eb = built_extra()
    cs = []
    # a: dots whose top pixels sit on row 199 at x = 163 (= 96 + 67: the fill lies at word 3, columns 96 .. 287), 182, 201; reuse holds to px = 220
    row = dot(163, 200) + dot(182, 200) + dot(201, 200)
    for name, x, f in (("a_last_reuse", 220, False), ("a_first_refill", 221, True), ("a_word_beyond", 252, True)):
        cs.append(_case(name, "a", "tl", row + probe_right(x, 199), 1, (x, 199), f, f))
    # b: a dot at the right (its middle row's fill: columns 224 ..), then a probe whose top row is the dot's last row and starts at x = 20
    cs.append(_case("b_next_row_left", "b", "tl", dot(300, 100) + probe_right(20, 101), 1, (20, 101), True, True))
    # c: a dot whose first fill is at (170, 100): rows 33 .. 167 + E; the probe's candidate at (210, 100 + k) (same columns: 96 .. 287).
    #    E = 0 refills at the dot's pixels (169, 101) and (170, 102): the probe reuses at k = 2 (the dot's last row) and never below;
    #    E > 0 keeps the first fill through the dot and reuses while 100 + k + 67 <= 167 + E
    for k in (0, 2, 3, 8, 9, 16, 17, 24, 25, 60):
        cs.append(_case("c_rows_%02d" % k, "c", "tl", dot(170, 101) + probe_down(210, 100 + k), 1, (210, 100 + k), k not in (0, 2), (k > eb) if eb else k not in (0, 2)))
    # d: borders.  Top left: a dot at (5, 2) fills at word -2, row -65; probes at px = 30 (reuse: px <= 60) and px = 62 (refill at word -1)
    cs.append(_case("d_top_left_reuse", "d", "tl", dot(5, 3) + probe_right(30, 2), 1, (30, 2), False, False))
    cs.append(_case("d_top_left_refill", "d", "tl", dot(5, 3) + probe_right(62, 2), 1, (62, 2), True, True))
    cs.append(_case("d_left_down", "d", "tl", dot(3, 41) + probe_down(40, 40), 1, (40, 40), False, False))
    # top right: the window's last columns lie beyond the image; a probe pointing down in the image's last columns
    cs.append(_case("d_top_right", "d", "tr", dot(-60, 3) + probe_down(-3, 2), 1, None))
    cs.append(_case("d_right_edge_row", "d", "tr", dot(-150, 201) + dot(-131, 201) + probe_right(-72, 200), 1, None))
    # bottom: the window's last rows lie below the image
    cs.append(_case("d_bottom_left", "d", "bl", dot(4, -6) + probe_right(30, -7), 1, None))
    cs.append(_case("d_bottom_right", "d", "br", dot(-120, -6) + probe_right(-73, -7), 1, None))
    cs.append(_case("d_bottom_down", "d", "bl", dot(100, -79) + probe_down(140, -80), 1, None))
    # e: a blob of 30 px and in one mask its continuation; alone, and behind a block of rejected candidates (so that the frame asks for help)
    block = _squares(40, 20, 12, 24)
    blob = C.hbar(150, 100, 30)
    cs.append(_case("e_first_alone", "e", "tl", blob, 0, None))
    cs.append(_case("e_first_continued", "e", "tl", blob + C.hbar(190, 100, 60), 1, None))
    cs.append(_case("e_blob_alone", "e", "tl", block + blob, 0, None))
    cs.append(_case("e_blob_continued", "e", "tl", block + blob + C.hbar(190, 100, 60), 1, None))
    # f: two bands of 2 x 2 squares (12 rejected candidates each, 24 px apart), then three probes; and light frames
    heavy = _squares(10, 30, 14, 24) + _squares(22, 60, 14, 24) + probe_right(20, 120) + probe_down(200, 150) + probe_right(100, 300)
    cs.append(_case("f_heavy", "f", "tl", heavy, 3, None))
    cs.append(_case("f_light", "f", "tl", probe_right(50, 50), 1, None))
    return tuple(cs)


def frame(case, W, H):
    x, y, rw, rh = C.ROI[(W, H)]
    ax, ay = C.ANCHORS[case.anchor](rw, rh)
    f = C._blank((W, H)).copy()
    xs, ys = case.seeds[:, 0] + ax, case.seeds[:, 1] + ay
    assert xs.min() >= 0 and ys.min() >= 0 and xs.max() < rw and ys.max() < rh, case.name
    f[y + ys, x + xs] = C.COLOURS[[c.name for c in cases()].index(case.name) % 3]
    return f


@functools.lru_cache(maxsize=None)
def reference(size):
    """{name: Ref}: the oracle's record and mask of every case at a frame size.  Shared by a session's tests; nothing may write to it."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o

    def one(c):
        r = o.process_frame(frame(c, *size), stages=0x1, max_gap=MAX_GAP, want_images=True)
        assert r["map_open"] == 1
        r["lsd"].setflags(write=False)
        return Ref(c, r["lines"], r["rounds"], r["n_mask_px"], r["steps"], r["lsd"])

    C._blank(size)
    with ThreadPoolExecutor(8) as ex:
        return {R_.case.name: R_ for R_ in ex.map(one, cases())}
