"""Frame sizes chosen for the LAYOUTS the kernels branch on, not for being screens, and a scene that works at all of them.

The map ROI follows from the frame height alone (rx = w(H) - x(H), rw = W - w(H)), so W and H pick the ROI's offset inside the
4-pixel quad grid (m_xoff = rx % 4), its width and the frame's row pitch independently.  CASES lists one (W, H) per layout with
the derived numbers written out; check_table() holds every row to smh.map_bounds and the whole table to the list of residues and
boundaries it is there for, so a typo in a size fails instead of testing something else.

make_frames() draws, at any accepted geometry: pixels round every threshold (fuzz_scenes.random_frame) in the bottom-right
quadrant, quiet terrain elsewhere, the button open, marker pixels on both sides of every boundary the passes and the line search
split the ROI at, marker lines longer than 50 px, a scale bar with its label anchor, marker colour just OUTSIDE the ROI, and
random alpha bytes in half the frames.  Pure numpy plus the library's host-only bounds helpers; the oracle is imported by
oracle_of() only."""
import functools
from collections import namedtuple

import numpy as np

import squad_mortar_helper_amd as smh
from fuzz_scenes import random_frame

GREEN, PURPLE, TEAL = (0, 255, 64), (217, 117, 192), (181, 232, 93)        # BGR of the three team colours
BUTTON_RED = (49, 67, 217)
MAX_GAP = 15

Case = namedtuple("Case", "W H rw rh m_xoff q_xoff m_quads group why")

# (W, H, rw, rh, m_xoff, q_xoff, m_quads, group, why).  m_xoff = rx % 4, q_xoff = (rx + rw // 2) % 4, m_quads = ceil((rw + m_xoff) / 4).
# Heights 359 / 360 give m_xoff 0, 361 -> 1, 362 -> 2, 363 -> 3 at rh 273..276.
_TABLE = [
    # ---- width group: ~275 rows tall (one at 1440p), the width on a boundary ----
    (319, 360, 8, 274, 0, 0, 2, "width", "rw = 8: the narrowest ROI that is accepted"),
    (343, 361, 31, 275, 1, 0, 8, "width", "rw = 31: one tile column, one short of full"),
    (343, 360, 32, 274, 0, 0, 8, "width", "rw = 32: exactly one tile column"),
    (347, 363, 33, 276, 3, 3, 9, "width", "rw = 33: a second tile column of one pixel; rw + m_xoff = 36"),
    (563, 363, 249, 276, 3, 3, 63, "width", "m_quads = 63 (rw + m_xoff = 252): the last wave one quad short"),
    (567, 362, 254, 276, 2, 1, 64, "width", "m_quads = 64 with m_xoff 2: rw + m_xoff = 256, ui_pitch exactly full"),
    (567, 360, 256, 274, 0, 0, 64, "width", "m_quads = 64 with m_xoff 0: one full wave"),
    (568, 361, 256, 275, 1, 1, 65, "width", "m_quads = 65: a second wave with one active lane, the wave edge at pixel column 255"),
    (1331, 362, 1018, 276, 2, 3, 255, "width", "m_quads = 255: the fourth wave one quad short"),
    (1335, 360, 1024, 274, 0, 0, 256, "width", "m_quads = 256, rw = 1024: four full waves, 32 tile columns"),
    (1336, 361, 1024, 275, 1, 1, 257, "width", "m_quads = 257: a fifth wave with one lane, wave edges at 255 / 511 / 767 / 1023"),
    (2355, 363, 2041, 276, 3, 3, 511, "width", "m_quads = 511"),
    (2359, 361, 2047, 275, 1, 0, 512, "width", "rw = 2047, m_quads = 512: 64 tile columns, the last one short"),
    (2359, 360, 2048, 274, 0, 0, 512, "width", "rw = 2048: exactly 64 tile columns (one chunk of the compact index walk)"),
    (2360, 360, 2049, 274, 0, 0, 513, "width", "rw = 2049: a 65th tile column of one pixel, m_quads = 513"),
    (2361, 362, 2048, 276, 2, 2, 513, "width", "rw = 2048 shifted by m_xoff 2: 65 word columns over 64 tile columns"),
    (3295, 1440, 2049, 1096, 3, 3, 513, "width", "rw = 2049 at 1440 rows: the search service keeps its tiles behind the compact index (above 1080p), 65 tile columns"),
    (2232, 362, 1919, 276, 2, 1, 481, "width", "rw = 1919: tile_idx_pitch 64, one compact group"),
    (2231, 360, 1920, 274, 0, 0, 480, "width", "rw = 1920: the last width with one compact group"),
    (2235, 363, 1921, 276, 3, 3, 481, "width", "rw = 1921: tile_idx_pitch 65, two compact groups"),
    (2233, 361, 1921, 275, 1, 1, 481, "width", "rw = 1921 at m_xoff 1 and W % 4 == 1"),
    (4407, 360, 4096, 274, 0, 0, 1024, "width", "rw + m_xoff = 4096 with m_xoff 0: the widest ROI that is accepted"),
    (4406, 360, 4095, 274, 0, 3, 1024, "width", "rw + m_xoff = 4095"),
    (4407, 361, 4095, 275, 1, 0, 1024, "width", "rw + m_xoff = 4096 with m_xoff 1"),
    (451, 360, 140, 274, 0, 2, 35, "width", "residues: m_xoff 0 with W % 4 == 3 and q_xoff 2"),
    (454, 361, 142, 275, 1, 0, 36, "width", "residues: m_xoff 1 with W % 4 == 2"),
    (453, 362, 140, 276, 2, 0, 36, "width", "residues: m_xoff 2 with W % 4 == 1 and q_xoff 0"),
    (454, 362, 141, 276, 2, 0, 36, "width", "residues: m_xoff 2 with W % 4 == 2, rw % 4 == 1"),
    # ---- height group: ~100 px wide, the height on a boundary ----
    (409, 356, 101, 271, 1, 3, 26, "height", "rh % 8 == 7"),
    (381, 357, 72, 272, 2, 2, 19, "height", "rh % 8 == 0"),
    (401, 359, 90, 273, 0, 1, 23, "height", "rh % 8 == 1"),
    (451, 364, 136, 277, 0, 0, 34, "height", "rh % 8 == 5"),
    (391, 365, 75, 278, 1, 2, 19, "height", "rh % 8 == 6, rw % 4 == 3"),
    (406, 368, 88, 280, 3, 3, 23, "height", "rh = 280 = 5 x 56"),
    (416, 369, 97, 281, 0, 0, 25, "height", "rh = 281 = 5 x 56 + 1"),
    (447, 378, 120, 288, 0, 0, 30, "height", "rh = 288 = 12 x 24"),
    (412, 380, 83, 289, 2, 3, 22, "height", "rh = 289 = 12 x 24 + 1"),
    (491, 441, 110, 336, 1, 0, 28, "height", "rh = 336 = 14 x 24 = 6 x 56"),
    (460, 443, 77, 337, 3, 1, 20, "height", "rh = 337: one row more than both"),
    (1121, 1181, 100, 899, 3, 1, 26, "height", "rh = 899: one below the band rule's limit"),
    (1118, 1182, 96, 900, 0, 0, 24, "height", "rh = 900: the last height with 24-row bands and the tile-major mask"),
    (1152, 1183, 129, 900, 1, 1, 33, "height", "rh = 900 at m_xoff 1"),
    (1097, 1184, 73, 901, 2, 2, 19, "height", "rh = 901: 58-row bands, bit rows only"),
    (1127, 1185, 102, 902, 3, 2, 27, "height", "rh = 902"),
    # ---- real windows with an odd width ----
    (1921, 1081, 986, 823, 3, 0, 248, "real", "a 1080p window one pixel larger each way: rows 4 bytes off a 16-byte boundary"),
    (1281, 721, 657, 549, 3, 3, 165, "real", "720p + 1"),
    (1365, 767, 702, 584, 1, 0, 176, "real", "1366 x 768 - 1: rows 4 bytes off"),
]
CASES = [Case(*t) for t in _TABLE]
IDS = ["%dx%d" % (c.W, c.H) for c in CASES]
WIDTH_GROUP = [c for c in CASES if c.group == "width"]
HEIGHT_EDGE = [c for c in CASES if c.group == "height" and 899 <= c.rh <= 902]
ALIGNED_CASE = next(c for c in CASES if c.W % 4 == 0 and c.m_quads == 65)          # the offset-base-pointer test: W % 4 == 0
# sizes on the wrong side of the limits: (W, H, why)
REFUSED = [(4408, 360, "rw = 4097"), (4408, 361, "rw + m_xoff = 4097"), (4408, 362, "rw + m_xoff = 4097 (m_xoff 2)"), (318, 360, "rw = 7")]


def derive(W, H):
    """The numbers of a table row from the library's own bounds."""
    rx, ry, rw, rh = smh.map_bounds(W, H)
    m_xoff = rx % 4
    return dict(rx=rx, ry=ry, rw=rw, rh=rh, m_xoff=m_xoff, q_xoff=(rx + rw // 2) % 4, m_quads=(rw + m_xoff + 3) // 4)


def check_table(cases=None):
    """Every row states what smh.map_bounds gives, and the table as a whole reaches what it is there for."""
    cases = CASES if cases is None else cases
    for c in cases:
        d = derive(c.W, c.H)
        got = (d["rw"], d["rh"], d["m_xoff"], d["q_xoff"], d["m_quads"])
        assert got == (c.rw, c.rh, c.m_xoff, c.q_xoff, c.m_quads), (c.W, c.H, got, c)
    assert len({(c.W, c.H) for c in cases}) == len(cases)
    have = lambda f: {f(c) for c in cases}                                            # noqa: E731
    assert have(lambda c: (c.m_xoff, c.W % 4)) == {(a, b) for a in range(4) for b in range(4)}
    assert have(lambda c: (c.m_xoff, c.q_xoff)) == {(a, b) for a in range(4) for b in range(4)}
    assert have(lambda c: c.rw % 4) == {0, 1, 2, 3}
    assert have(lambda c: c.m_quads) >= {63, 64, 65, 255, 256, 257, 511, 512, 513}
    assert have(lambda c: c.rw) >= {8, 31, 32, 33, 1919, 1920, 1921, 2047, 2048, 2049}
    assert have(lambda c: c.rw + c.m_xoff) >= {4095, 4096, 256, 1024, 2048}           # (multiples of 64: ui_pitch / bits_pitch_w exactly full)
    assert {(c.rw, c.m_xoff) for c in cases} >= {(4096, 0), (4095, 1)}
    narrow = [c for c in cases if c.group == "height"]
    assert all(72 <= c.rw <= 136 for c in narrow)
    assert {c.rh for c in narrow} >= {899, 900, 901, 902, 280, 281, 288, 289, 336, 337}
    assert any(c.rh % 24 == 0 for c in narrow) and any(c.rh % 56 == 0 for c in narrow)
    assert have(lambda c: c.rh % 8) == set(range(8)) and have(lambda c: (c.rh // 2) % 4) == {0, 1, 2, 3}
    assert sum(c.W % 2 == 1 for c in cases if c.group == "real") >= 3
    assert {(c.W, c.H) for c in cases} >= {(1921, 1081), (1281, 721), (1365, 767)}


# ---- the scene -------------------------------------------------------------------------------------------------------------

def boundaries(c):
    """Pixel columns b (ROI coordinates, 2 <= b <= rw - 2) the kernels split the ROI at: the scene marks columns b - 1 and b.
    256 k - m_xoff: the wave edges of the streaming passes (quad 64 k of the row); 32 j and 32 j - m_xoff next to a listed
    boundary: tile columns of the line search and words of the bit rows; 2048: the 64-column chunk of the compact index walk;
    the quadrant's first column."""
    b = {256 * k - c.m_xoff for k in range(1, 17)}
    for j in {c.rw // 32, (c.rw + c.m_xoff) // 32, 8, 32, 60, 64, 128, 2 * ((c.rw + c.m_xoff) // 64)}:
        b |= {32 * j, 32 * j - c.m_xoff}
    b |= {2048, c.rw // 2}
    return sorted(x for x in b if 2 <= x <= c.rw - 2)


def _quiet(rng, shape):
    """synth's terrain: saturation <= 30, never a marker colour, never near black.  RGB order is immaterial."""
    t = rng.integers(60, 141, size=tuple(shape) + (3,), dtype=np.uint8)
    m = t.max(axis=-1).astype(np.uint16)
    return np.maximum(t, (m - (3 * m) // 10).astype(np.uint8)[..., None])


def scale_bar(c):
    """(left, right, y) of the bar in quadrant coordinates and its (meters, x, y) anchor, or None where qw < 40."""
    qw, qh = c.rw // 2, c.rh // 2
    if qw < 40:
        return None
    yb = qh - 20
    xl, xr = 6, min(qw - 7, 6 + 120)
    reach = int(np.floor(20.0 / 640.0 * qw + 0.5))                  # rows below the anchor find_scale_width looks at
    y = yb - max(min(6, reach - 1), 0)
    return (xl, xr, yb), (100, (xl + xr) // 2, y)


def marker_lines(c):
    """The drawn marker lines in ROI coordinates (x0, y0, x1, y1, thickness), all in the top half.  find_lines skips every pixel
    within 7 px of the INFINITE line through an accepted one, so the lines are slanted apart: no one's extension reaches another.
    rw > 2048: one crosses column 2048, one lies at or right of it."""
    rw, top = c.rw, c.rh // 2 - 8
    lines = []
    if rw >= 160:
        n = min(200, rw - 60)
        lines += [(20, 10, 20 + n, 10 + n // 4, 3)]
    else:
        lines += [(max(rw - 4, 5), 8, max(rw - 4, 5), min(top, 110), 1)]
    if rw >= 600:
        lines += [(rw - 10, 10, rw - 170, 90, 3)]
    if rw > 2048:
        xe = min(rw - 1, 2048 + 70)
        lines += [(xe, 110 - (xe - 1978) // 2, 1978, 110, 3)]
        lines += [(2060, 10, 2060 + min(200, rw - 2070), 10 + min(200, rw - 2070) // 4, 3)] if rw - 2048 >= 80 else [(rw - 1, 8, rw - 1, 60, 1)]
    return lines


def _draw_line(roi, x0, y0, x1, y1, th, colour):
    n = 2 * max(abs(x1 - x0), abs(y1 - y0)) + 1
    xs = np.rint(np.linspace(x0, x1, n)).astype(int)
    ys = np.rint(np.linspace(y0, y1, n)).astype(int)
    h, w = roi.shape[:2]
    for dy in range(-(th // 2), th // 2 + 1):
        for dx in range(-(th // 2), th // 2 + 1):
            roi[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)] = colour


def make_frame(c, seed, open_=True, random_alpha=False):
    """One BGRA frame of case c -> (frame, info).  info: anchors, scales_start_y, marks [(row, col)] single marker pixels whose
    dilation crosses a boundary to (row, col2), lines, bar."""
    W, H = c.W, c.H
    rng = np.random.default_rng(seed)
    rx, ry, rw, rh = smh.map_bounds(W, H)
    bx, by, bw, bh = smh.button_bounds(W, H)
    qw, qh = rw // 2, rh // 2
    f = np.empty((H, W, 4), np.uint8)
    f[..., :3] = 32
    if open_:
        f[by:by + bh, bx:bx + bw, :3] = BUTTON_RED
    # marker colour just outside the ROI on all four sides: the oracle never sees it, a missing edge mask dilates it in
    f[ry - 1:ry + rh + 1, rx - 1:rx + rw + 1, :3] = (GREEN, PURPLE, TEAL)[seed % 3]
    roi = f[ry:ry + rh, rx:rx + rw, :3]
    roi[...] = _quiet(rng, (rh, rw))
    # pixels round every threshold in the quadrant and the four columns / rows before it (the OCR neighbourhood reaches 3)
    y0, x0 = max(qh - 4, 0), max(qw - 4, 0)
    roi[y0:, x0:] = random_frame(rng, rw - x0, rh - y0)[..., :3]
    bar = scale_bar(c)
    anchors, start_y = [], 0
    if bar is not None:
        (xl, xr, yb), anchor = bar
        q = roi[qh:, qw:]
        q[max(anchor[2] - 3, 0):yb + 10, max(xl - 5, 0):xr + 6] = _quiet(rng, (yb + 10 - max(anchor[2] - 3, 0), xr + 6 - max(xl - 5, 0)))
        q[yb, xl:xr + 1] = 0
        q[yb:yb + 7, xl] = 0
        q[yb:yb + 7, xr] = 0
        anchors, start_y = [anchor], anchor[2]
    marks = []                                                     # (row, col of the pixel, col its dilation must reach)
    top = qh - 6                                                   # rows below this are round-threshold noise right of qw - 4
    for i, b in enumerate(boundaries(c)):
        r = 36 + 8 * (i % 10)
        if r + 4 < top:
            roi[r, b - 1] = GREEN; marks.append((r, b - 1, b))
            roi[r + 4, b] = PURPLE; marks.append((r + 4, b, b - 1))
    # the ROI's own edges: columns 0, 1, rw - 2, rw - 1, rows 0 and rh - 1, the quadrant's first row
    for r, col in ((124, 0), (128, 1), (124, rw - 1), (128, rw - 2)):
        roi[min(r, top - 2), col] = TEAL
    roi[0, rw // 3] = GREEN; roi[0, rw - 1] = GREEN; roi[rh - 1, rw // 3] = GREEN; roi[rh - 1, 0] = PURPLE; roi[rh - 1, rw - 1] = PURPLE
    roi[qh - 1, rw // 5] = GREEN; roi[qh, rw // 5 + (4 if rw >= 40 else 0)] = GREEN
    # dotted columns over the whole height, one per phase: at every band and tile-row edge R some column has a pixel at R - 1 and
    # none at R, another the reverse -- the vertical dilation crosses every edge in both directions
    for ph, col in enumerate((3, 7, 11) if qw - 4 > 13 else (3,)):
        roi[ph::3, col] = (GREEN, PURPLE, TEAL)[ph]
    lines = marker_lines(c)
    for k, (xa, ya, xb, yb_, th) in enumerate(lines):
        _draw_line(roi, xa, ya, xb, yb_, th, (GREEN, PURPLE, TEAL)[k % 3])
    # the quadrant's first and last columns and rows in the OCR image: white pixels (kept, black in the image) and greys that are
    # kept only through a white pixel in their 7 x 7 neighbourhood -- which the reference clamps at qw - 3 / qh - 3
    q = roi[qh:2 * qh, qw:2 * qw]
    for (r, col) in ((1, 0), (1, qw - 1), (1, max(qw - 3, 0)), (qh - 1, min(8, qw - 2)), (max(qh - 3, 0), min(12, qw - 1))):
        q[r, col] = 255
    q[2, 0:4] = 135; q[2, max(qw - 6, 0):] = 135; q[max(qh - 6, 0):, min(8, qw - 2)] = 135; q[qh - 1, min(8, qw - 2)] = 255
    f[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8) if random_alpha else 255
    return f, dict(anchors=anchors, scales_start_y=start_y, marks=marks, lines=lines, bar=bar)


def make_frames(c):
    """The case's batch: an open frame with alpha 255, a CLOSED frame (so the frames behind it keep an odd alignment whatever the
    search does with it), an open frame with random alpha -> (uint8 [3, H, W, 4], [info])."""
    base = 1000 * CASES.index(c)
    made = [make_frame(c, base + 1), make_frame(c, base + 2, open_=False, random_alpha=True), make_frame(c, base + 3, random_alpha=True)]
    return np.stack([m[0] for m in made]), [m[1] for m in made]


@functools.lru_cache(maxsize=4)
def oracle_of(c):
    """What the CPU oracle makes of make_frames(c), computed once per case: (frames, infos, refs); refs[i] = process_frame's dict
    with the images (grey ui_map), plus ui_colour and minimap; the closed frame's has map_open 0."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o
    frames, infos = make_frames(c)

    def one(i):
        ref = o.process_frame(frames[i], grayscale=True, max_gap=MAX_GAP, stages=0xF, anchors=infos[i]["anchors"] or None,
                              scales_start_y=infos[i]["scales_start_y"], want_images=True)
        if ref["map_open"]:
            ref["ui_colour"] = o.process_frame(frames[i], grayscale=False, stages=0x2, want_images=True)["ui_map"]
            ref["minimap"] = o.find_minimap(frames[i])
        ref["red_pixels"] = o.button_red_pixels(frames[i])
        return ref
    with ThreadPoolExecutor(len(frames)) as ex:                      # (ctypes releases the GIL inside the oracle)
        refs = list(ex.map(one, range(len(frames))))
    return frames, infos, refs
