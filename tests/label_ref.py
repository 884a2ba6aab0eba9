"""Restatement of the marker labels (include/smh_vision_hip.h, "map view: labels"): the strings, the layout, the placement and
the pixel rule, sequential and in numpy f32 / Python integers.  Shares no code with the library.  The firing numbers are an
INPUT (a dict with meters, alt_delta, mils, bearing, source): the restatement does not recompute them.

A slot is a dict: firing, mid (two f32), dir (two f32), rgba, runs = [(x2, y2, text bytes)]; a line without a label has
runs == [] and mid = dir = (0, 0)."""
import math

import numpy as np

f32 = np.float32
NONE, SCALES, HEIGHTMAP = 0, 1, 2
PLUS_MINUS, DEGREE = b"\xb1", b"\xb0"
GAP = 5                                                           # font units between the two blocks (the reference's 10 px)

# the 27 glyphs, 5 x 7, typed here on their own ('#' = ink)
_ART = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
    "m": (".....", ".....", "##.#.", "#.#.#", "#.#.#", "#...#", "#...#"),
    "i": ("..#..", ".....", ".##..", "..#..", "..#..", "..#..", ".###."),
    "l": (".##..", "..#..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "a": (".....", ".....", ".###.", "....#", ".####", "#...#", ".####"),
    "t": (".#...", ".#...", "###..", ".#...", ".#...", ".#..#", "..##."),
    "R": ("####.", "#...#", "#...#", "####.", "#.#..", "#..#.", "#...#"),
    "A": (".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"),
    "N": ("#...#", "##..#", "#.#.#", "#..##", "#...#", "#...#", "#...#"),
    "G": (".###.", "#...#", "#....", "#.###", "#...#", "#...#", ".####"),
    "E": ("#####", "#....", "#....", "####.", "#....", "#....", "#####"),
    "!": ("..#..", "..#..", "..#..", "..#..", "..#..", ".....", "..#.."),
    "<": ("...#.", "..#..", ".#...", "#....", ".#...", "..#..", "...#."),
    "-": (".....", ".....", ".....", "#####", ".....", ".....", "....."),
    ">": (".#...", "..#..", "...#.", "....#", "...#.", "..#..", ".#..."),
    " ": (".....", ".....", ".....", ".....", ".....", ".....", "....."),
    "\xb1": (".....", "..#..", ".###.", "..#..", ".....", ".###.", "....."),
    "\xb0": (".##..", "#..#.", "#..#.", ".##..", ".....", ".....", "....."),
}


def glyph_rows(ch):
    """The 7 row bytes of byte `ch` (bit 4 = leftmost column), or None for a byte outside the set."""
    art = _ART.get(chr(ch))
    if art is None:
        return None
    return [sum(1 << (4 - c) for c in range(5) if row[c] == "#") for row in art]


GLYPHS = {ord(k): glyph_rows(ord(k)) for k in _ART}
assert len(GLYPHS) == 27


def fmt0(v):
    """Rust's {:.0} of a non-negative f64: round half to even, unsigned decimal."""
    r = int(round(float(v)))                                     # Python's round() of a float: ties to even, exact
    assert r >= 0
    return str(r).encode("latin-1")


def cast_i32(v):
    """Rust's `as i32` of an f64: truncating, saturating, NaN -> 0."""
    v = float(v)
    if v != v:
        return 0
    if v >= 2147483647.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


def _mil(firing, d):
    m = float(firing["mils"][d])
    return b"RANGE!" if m != m else fmt0(m)


def _whole(v):
    return str(int(float(v))).encode("latin-1")


def translate(line, viewport):
    sw, sh, tx, ty = (f32(v) for v in viewport)
    x0, y0, x1, y1 = (f32(v) for v in line)
    with np.errstate(all="ignore"):
        return (f32(x0 * sw) + tx, f32(y0 * sh) + ty), (f32(x1 * sw) + tx, f32(y1 * sh) + ty)


def format_label(line, firing, viewport, rgba):
    """The slot of one line.  line = (x0, y0, x1, y1) in map-ROI coordinates; viewport = (sw, sh, tx, ty)."""
    slot = {"firing": firing, "mid": (f32(0), f32(0)), "dir": (f32(0), f32(0)), "rgba": tuple(int(v) for v in rgba), "runs": []}
    p0, p1 = translate(line, viewport)
    with np.errstate(all="ignore"):
        dx, dy = f32(p0[0] - p1[0]), f32(p0[1] - p1[1])
        len2 = f32(f32(dx * dx) + f32(dy * dy))
    if firing["source"] == NONE:
        return slot
    if not all(math.isfinite(float(v)) for v in (p0[0], p0[1], p1[0], p1[1])):
        return slot
    if len2 == 0:
        return slot
    if not float(firing["meters"]) < 999999.5:
        return slot
    rng = fmt0(firing["meters"]) + b"m"
    b = firing["bearing"]
    runs = []
    if firing["source"] == SCALES:
        mil = _mil(firing, 0)
        rows = [rng, mil if mil == b"RANGE!" else mil + b" mil"]
        if dx >= 0:
            rows += [b"-> " + _whole(b[1]) + DEGREE, b"<- " + _whole(b[0]) + DEGREE]
        else:
            rows += [b"-> " + _whole(b[0]) + DEGREE, b"<- " + _whole(b[1]) + DEGREE]
        w = [6 * len(r) for r in rows]
        W2, W4 = max(w[0], w[1]), max(w)
        for k, r in enumerate(rows):
            runs.append((-W2 + (W4 - w[k]), 18 * k, r))
    else:
        A = abs(cast_i32(firing["alt_delta"]))
        rows = [rng, PLUS_MINUS + str(A).encode("latin-1") + b"m alt"]
        for k, r in enumerate(rows):
            runs.append((-6 * len(r), 18 * k, r))
        fwd = dx > 0 or (dx == 0 and dy < 0)
        a, c = (0, 1) if fwd else (1, 0)
        ma, mc = _mil(firing, a), _mil(firing, c)
        left = [b"<- " + (ma if ma == b"RANGE!" else ma + b" mil"), _whole(b[a]) + DEGREE]
        right = [(mc if mc == b"RANGE!" else mc + b" mil") + b" ->", _whole(b[c]) + DEGREE]
        Wf, Wb = max(6 * len(r) for r in left), max(6 * len(r) for r in right)
        x_block = -(Wf + Wb + GAP)
        for k, r in enumerate(left):
            runs.append((x_block + 2 * (Wf - 6 * len(r)), 36 + 18 * k, r))
        for k, r in enumerate(right):
            runs.append((x_block + 2 * (GAP + Wf), 36 + 18 * k, r))
    assert len(runs) <= 6 and all(len(r[2]) <= 16 for r in runs)
    with np.errstate(all="ignore"):
        mid = (f32(f32(p0[0] + p1[0]) / f32(2)), f32(f32(p0[1] + p1[1]) / f32(2)))
        ln = np.sqrt(len2)
        s = f32(1) if dx > 0 else f32(-1)
        e = (f32(f32(s * dx) / ln), f32(f32(s * dy) / ln))
    slot["mid"], slot["dir"], slot["runs"] = mid, e, runs
    return slot


def pixel_hit(slot, X, Y, S):
    """The pixel rule for ONE pixel of one slot, a scalar operation at a time."""
    if not slot["runs"]:
        return False
    with np.errstate(all="ignore"):
        cx, cy = f32(X) + f32(0.5), f32(Y) + f32(0.5)
        ax, ay = f32(cx - slot["mid"][0]), f32(cy - slot["mid"][1])
        ex, ey = slot["dir"]
        u = f32(f32(f32(ax * ex) + f32(ay * ey)) / f32(S))
        v = f32(f32(f32(ay * ex) - f32(ax * ey)) / f32(S))
        for x2, y2, text in slot["runs"]:
            iu = np.floor(f32(u - f32(f32(x2) * f32(0.5))))
            iv = np.floor(f32(v - f32(f32(y2) * f32(0.5))))
            if 0 <= iu < 6 * len(text) and 0 <= iv < 9:
                iu, iv = int(iu), int(iv)
                col, row = iu % 6, iv - 1
                if col < 5 and 0 <= row <= 6 and (GLYPHS[text[iu // 6]][row] >> (4 - col)) & 1:
                    return True
    return False


def draw(image, slots, S):
    """Paints the slots, in order, onto `image` (H x W x 4 uint8, in place): the pixel rule on every pixel, every step one f32
    operation on the whole image (numpy does not fuse).  Returns the number of pixels whose bytes changed."""
    H, W = image.shape[:2]
    before = image.copy()
    cx = (np.arange(W, dtype=f32) + f32(0.5))[None, :]
    cy = (np.arange(H, dtype=f32) + f32(0.5))[:, None]
    table = np.zeros((256, 7), np.uint8)
    for ch, rows in GLYPHS.items():
        table[ch] = rows
    for slot in slots:
        if not slot["runs"]:
            continue
        with np.errstate(all="ignore"):
            ax = (cx - slot["mid"][0]).astype(f32) + np.zeros((H, 1), f32)
            ay = (cy - slot["mid"][1]).astype(f32) + np.zeros((1, W), f32)
            ex, ey = slot["dir"]
            u = ((ax * ex).astype(f32) + (ay * ey).astype(f32)).astype(f32) / f32(S)
            v = ((ay * ex).astype(f32) - (ax * ey).astype(f32)).astype(f32) / f32(S)
            paint = np.zeros((H, W), bool)
            for x2, y2, text in slot["runs"]:
                iu = np.floor(u - f32(f32(x2) * f32(0.5)))
                iv = np.floor(v - f32(f32(y2) * f32(0.5)))
                hit = (iu >= 0) & (iu < 6 * len(text)) & (iv >= 0) & (iv < 9)
                if not hit.any():
                    continue
                ys, xs = np.nonzero(hit)
                ju, jv = iu[ys, xs].astype(np.int64), iv[ys, xs].astype(np.int64)
                col, row = ju % 6, jv - 1
                ok = (col < 5) & (row >= 0) & (row <= 6)
                chars = np.frombuffer(text, np.uint8)[ju // 6]
                bits = (table[chars, np.clip(row, 0, 6)] >> np.clip(4 - col, 0, 4)) & 1
                on = ok & (bits == 1)
                paint[ys[on], xs[on]] = True
        image[paint] = np.array(list(slot["rgba"][:3]) + [255], np.uint8)
    return int((image != before).any(axis=2).sum())
