"""Restatement of the map view's debug text and the vision debugger (include/smh_vision_hip.h, "map view: debug text and the
vision debugger"): the probe's arithmetic, its string, the window's placement, the item list in paint order and the pixel rules,
in numpy f32 / Python integers, a scalar operation at a time.  Shares no code with the library; the stroke of a rectangle is
render_layers_ref's.

A run is the tuple (x, y, (r, g, b, a), flags, text bytes); a probe is a dict with the fields of smhv_probe (all 0 when it is not
valid).  The marker thresholds are an INPUT (`consts`: the "consts_toml" table of tests/golden/reference_constants.json)."""
import json
import os

import numpy as np

import render_layers_ref as YR

f32 = np.float32
FLT_MAX = f32(np.finfo(np.float32).max)
MAP_COORDS = 1
DRAW_PROBES, MINIMAP_CAPTION = 1, 2
MAX_RUNS, MAX_BYTES, MAX_LINES, MAX_PROBES = 64, 64, 8, 16
CAPTION = b"No minimap bounds detected or we don't need to detect them"
WINDOW_BG, WHITE, BLACK, CAPTION_RED = (15, 15, 15), (255, 255, 255), (0, 0, 0), (255, 0, 0)
TEAMS = ("ALPHA", "BRAVO", "CHARLIE")

# the 97 glyphs, 5 x 7, typed here on their own ('#' = ink), by byte
_ART = {
    0x20: (".....", ".....", ".....", ".....", ".....", ".....", "....."),   # space
    0x21: ("..#..", "..#..", "..#..", "..#..", "..#..", ".....", "..#.."),   # !
    0x22: (".#.#.", ".#.#.", ".#.#.", ".....", ".....", ".....", "....."),   # "
    0x23: (".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#."),   # #
    0x24: ("..#..", ".####", "#.#..", ".###.", "..#.#", "####.", "..#.."),   # $
    0x25: ("##...", "##..#", "...#.", "..#..", ".#...", "#..##", "...##"),   # %
    0x26: (".##..", "#..#.", "#.#..", ".#...", "#.#.#", "#..#.", ".##.#"),   # &
    0x27: ("..##.", "..##.", "..#..", ".#...", ".....", ".....", "....."),   # '
    0x28: ("...#.", "..#..", ".#...", ".#...", ".#...", "..#..", "...#."),   # (
    0x29: (".#...", "..#..", "...#.", "...#.", "...#.", "..#..", ".#..."),   # )
    0x2A: (".....", "..#..", "#.#.#", ".###.", "#.#.#", "..#..", "....."),   # *
    0x2B: (".....", "..#..", "..#..", "#####", "..#..", "..#..", "....."),   # +
    0x2C: (".....", ".....", ".....", ".....", "..##.", "..##.", ".##.."),   # ,
    0x2D: (".....", ".....", ".....", "#####", ".....", ".....", "....."),   # -
    0x2E: (".....", ".....", ".....", ".....", ".....", ".###.", ".###."),   # .
    0x2F: (".....", "....#", "...#.", "..#..", ".#...", "#....", "....."),   # /
    0x30: (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),   # 0
    0x31: ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),   # 1
    0x32: (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),   # 2
    0x33: ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),   # 3
    0x34: ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),   # 4
    0x35: ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),   # 5
    0x36: ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),   # 6
    0x37: ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),   # 7
    0x38: (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),   # 8
    0x39: (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),   # 9
    0x3A: (".....", "..##.", "..##.", ".....", "..##.", "..##.", "....."),   # :
    0x3B: (".....", "..##.", "..##.", ".....", "..##.", "..##.", ".##.."),   # ;
    0x3C: ("...#.", "..#..", ".#...", "#....", ".#...", "..#..", "...#."),   # <
    0x3D: (".....", ".....", "#####", ".....", "#####", ".....", "....."),   # =
    0x3E: (".#...", "..#..", "...#.", "....#", "...#.", "..#..", ".#..."),   # >
    0x3F: (".###.", "#...#", "....#", "...#.", "..#..", ".....", "..#.."),   # ?
    0x40: (".###.", "#...#", "#.###", "#.#.#", "#.###", "#....", ".###."),   # @
    0x41: (".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"),   # A
    0x42: ("####.", "#...#", "#...#", "####.", "#...#", "#...#", "####."),   # B
    0x43: (".###.", "#...#", "#....", "#....", "#....", "#...#", ".###."),   # C
    0x44: ("###..", "#..#.", "#...#", "#...#", "#...#", "#..#.", "###.."),   # D
    0x45: ("#####", "#....", "#....", "####.", "#....", "#....", "#####"),   # E
    0x46: ("#####", "#....", "#....", "####.", "#....", "#....", "#...."),   # F
    0x47: (".###.", "#...#", "#....", "#.###", "#...#", "#...#", ".####"),   # G
    0x48: ("#...#", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"),   # H
    0x49: (".###.", "..#..", "..#..", "..#..", "..#..", "..#..", ".###."),   # I
    0x4A: ("..###", "...#.", "...#.", "...#.", "...#.", "#..#.", ".##.."),   # J
    0x4B: ("#...#", "#..#.", "#.#..", "##...", "#.#..", "#..#.", "#...#"),   # K
    0x4C: ("#....", "#....", "#....", "#....", "#....", "#....", "#####"),   # L
    0x4D: ("#...#", "##.##", "#.#.#", "#.#.#", "#...#", "#...#", "#...#"),   # M
    0x4E: ("#...#", "##..#", "#.#.#", "#..##", "#...#", "#...#", "#...#"),   # N
    0x4F: (".###.", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."),   # O
    0x50: ("####.", "#...#", "#...#", "####.", "#....", "#....", "#...."),   # P
    0x51: (".###.", "#...#", "#...#", "#...#", "#.#.#", "#..#.", ".##.#"),   # Q
    0x52: ("####.", "#...#", "#...#", "####.", "#.#..", "#..#.", "#...#"),   # R
    0x53: (".####", "#....", "#....", ".###.", "....#", "....#", "####."),   # S
    0x54: ("#####", "..#..", "..#..", "..#..", "..#..", "..#..", "..#.."),   # T
    0x55: ("#...#", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."),   # U
    0x56: ("#...#", "#...#", "#...#", "#...#", "#...#", ".#.#.", "..#.."),   # V
    0x57: ("#...#", "#...#", "#...#", "#.#.#", "#.#.#", "#.#.#", ".#.#."),   # W
    0x58: ("#...#", "#...#", ".#.#.", "..#..", ".#.#.", "#...#", "#...#"),   # X
    0x59: ("#...#", "#...#", ".#.#.", "..#..", "..#..", "..#..", "..#.."),   # Y
    0x5A: ("#####", "....#", "...#.", "..#..", ".#...", "#....", "#####"),   # Z
    0x5B: (".###.", ".#...", ".#...", ".#...", ".#...", ".#...", ".###."),   # [
    0x5C: (".....", "#....", ".#...", "..#..", "...#.", "....#", "....."),   # \
    0x5D: (".###.", "...#.", "...#.", "...#.", "...#.", "...#.", ".###."),   # ]
    0x5E: ("..#..", ".#.#.", "#...#", ".....", ".....", ".....", "....."),   # ^
    0x5F: (".....", ".....", ".....", ".....", ".....", ".....", "#####"),   # _
    0x60: (".##..", "..##.", "...#.", ".....", ".....", ".....", "....."),   # `
    0x61: (".....", ".....", ".###.", "....#", ".####", "#...#", ".####"),   # a
    0x62: ("#....", "#....", "#.##.", "##..#", "#...#", "#...#", "####."),   # b
    0x63: (".....", ".....", ".###.", "#....", "#....", "#...#", ".###."),   # c
    0x64: ("....#", "....#", ".##.#", "#..##", "#...#", "#...#", ".####"),   # d
    0x65: (".....", ".....", ".###.", "#...#", "#####", "#....", ".###."),   # e
    0x66: ("..##.", ".#..#", ".#...", "###..", ".#...", ".#...", ".#..."),   # f
    0x67: (".....", ".####", "#...#", "#...#", ".####", "....#", ".###."),   # g
    0x68: ("#....", "#....", "#.##.", "##..#", "#...#", "#...#", "#...#"),   # h
    0x69: ("..#..", ".....", ".##..", "..#..", "..#..", "..#..", ".###."),   # i
    0x6A: ("...#.", ".....", "..##.", "...#.", "...#.", "#..#.", ".##.."),   # j
    0x6B: ("#....", "#....", "#..#.", "#.#..", "##...", "#.#..", "#..#."),   # k
    0x6C: (".##..", "..#..", "..#..", "..#..", "..#..", "..#..", ".###."),   # l
    0x6D: (".....", ".....", "##.#.", "#.#.#", "#.#.#", "#...#", "#...#"),   # m
    0x6E: (".....", ".....", "#.##.", "##..#", "#...#", "#...#", "#...#"),   # n
    0x6F: (".....", ".....", ".###.", "#...#", "#...#", "#...#", ".###."),   # o
    0x70: (".....", ".....", "####.", "#...#", "####.", "#....", "#...."),   # p
    0x71: (".....", ".....", ".##.#", "#..##", ".####", "....#", "....#"),   # q
    0x72: (".....", ".....", "#.##.", "##..#", "#....", "#....", "#...."),   # r
    0x73: (".....", ".....", ".###.", "#....", ".###.", "....#", "####."),   # s
    0x74: (".#...", ".#...", "###..", ".#...", ".#...", ".#..#", "..##."),   # t
    0x75: (".....", ".....", "#...#", "#...#", "#...#", "#..##", ".##.#"),   # u
    0x76: (".....", ".....", "#...#", "#...#", "#...#", ".#.#.", "..#.."),   # v
    0x77: (".....", ".....", "#...#", "#...#", "#.#.#", "#.#.#", ".#.#."),   # w
    0x78: (".....", ".....", "#...#", ".#.#.", "..#..", ".#.#.", "#...#"),   # x
    0x79: (".....", ".....", "#...#", "#...#", ".####", "....#", ".###."),   # y
    0x7A: (".....", ".....", "#####", "...#.", "..#..", ".#...", "#####"),   # z
    0x7B: ("...#.", "..#..", "..#..", ".#...", "..#..", "..#..", "...#."),   # {
    0x7C: ("..#..", "..#..", "..#..", "..#..", "..#..", "..#..", "..#.."),   # |
    0x7D: (".#...", "..#..", "..#..", "...#.", "..#..", "..#..", ".#..."),   # }
    0x7E: (".....", ".....", ".#...", "#.#.#", "...#.", ".....", "....."),   # ~
    0xB0: (".##..", "#..#.", "#..#.", ".##..", ".....", ".....", "....."),   # degree
    0xB1: (".....", "..#..", ".###.", "..#..", ".....", ".###.", "....."),   # plus-minus
}


def glyph_rows(ch):
    """The 7 row bytes of byte `ch` (bit 4 = leftmost column), or None for a byte outside the set."""
    art = _ART.get(ch)
    if art is None:
        return None
    return [sum(1 << (4 - c) for c in range(5) if row[c] == "#") for row in art]


GLYPHS = {k: glyph_rows(k) for k in _ART}
assert len(GLYPHS) == 97


def load_consts():
    """The reference's thresholds as the golden file records them (consts.toml)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_constants.json")) as fh:
        return json.load(fh)["consts_toml"]


def cast_u32(v):
    """Rust's `as u32` of an f32: truncating, saturating, NaN -> 0."""
    v = float(v)
    if v != v or v <= 0.0:
        return 0
    if v >= 4294967296.0:
        return 0xFFFFFFFF
    return int(v)


def hsv(R, G, B):
    """util/src/image.rs:159-187 as the header states it -> (h, s, v) as Python integers."""
    with np.errstate(all="ignore"):
        r, g, b = f32(R) / f32(255.0), f32(G) / f32(255.0), f32(B) / f32(255.0)
        mx, mn = max(r, max(g, b)), min(r, min(g, b))
        d = f32(mx - mn)
        if mx == mn:
            h = f32(0.0)
        elif mx == r:
            h = f32(f32(60.0) * f32(f32(g - b) / d))
        elif mx == g:
            h = f32(f32(60.0) * f32(f32(f32(b - r) / d) + f32(2.0)))
        else:
            h = f32(f32(60.0) * f32(f32(f32(r - g) / d) + f32(4.0)))
        if h < 0:
            h = f32(h + f32(360.0))
        s = f32(f32(f32(100.0) * d) / mx)
        v = f32(f32(100.0) * mx)
    return min(cast_u32(h), 65535), min(cast_u32(s), 255), min(cast_u32(v), 255)


def luma8(R, G, B):
    l = f32(f32(f32(0.2126) * f32(R)) + f32(f32(0.7152) * f32(G))) + f32(f32(0.0722) * f32(B))
    return min(int(f32(l)), 255)


def team_bits(h, s, v, consts):
    tol_h, tol_s, tol_v = consts["FIND_MARKER_HSV_HUE_TOLERANCE"], consts["FIND_MARKER_HSV_SAT_TOLERANCE"], consts["FIND_MARKER_HSV_VIB_TOLERANCE"]
    min_sat, arc = consts["FIND_MARKER_HSV_MIN_SAT"], consts["FIND_MARKER_PLAYER_DIR_ARC_SAT"]
    bits = 0
    for t, name in enumerate(TEAMS):
        mh, ms, mv = consts[name + "_MARKER_COLOR_HSV"]
        if abs(mh - h) <= tol_h:
            bits |= 1 << (3 * t)
        if s >= min_sat and (abs(ms - s) <= tol_s or abs(s - (ms - arc)) <= tol_s):
            bits |= 1 << (3 * t + 1)
        if abs(mv - v) <= tol_v:
            bits |= 1 << (3 * t + 2)
    return bits


ZERO_PROBE = dict(valid=0, px=0, py=0, rgb=(0, 0, 0), luma=0, h=0, s=0, v=0, mono=0, brightness=0, team_bits=0)


def probe(ui, map_open, point, scale, top_left, consts):
    """One probe of one frame: ui = uint8 [h, w, >= 3] (the ui_map as the batch holds it), point = (mx, my) -> dict."""
    mx, my = f32(point[0]), f32(point[1])
    if not map_open or (mx == FLT_MAX and my == FLT_MAX):
        return dict(ZERO_PROBE)
    sw, sh = (f32(1.0) if f32(v) == 0 else f32(v) for v in scale)
    with np.errstate(all="ignore"):
        ix, iy = f32(f32(mx - f32(top_left[0])) / sw), f32(f32(my - f32(top_left[1])) / sh)
    if ix < 0 or iy < 0:                                           # (a NaN passes)
        return dict(ZERO_PROBE)
    px, py = cast_u32(ix), cast_u32(iy)
    h_, w_ = ui.shape[:2]
    if px >= w_ or py >= h_:
        return dict(ZERO_PROBE)
    R, G, B = (int(v) for v in ui[py, px, :3])
    h, s, v = hsv(R, G, B)
    p = (R, G, B)
    return dict(valid=1, px=px, py=py, rgb=p, luma=luma8(R, G, B), h=h, s=s, v=v, mono=sum(abs(p[a] - p[b]) for a in range(3) for b in range(3)),
                brightness=min(p), team_bits=team_bits(h, s, v, consts))


def _bools(bits):
    return "[" + ", ".join("true" if (bits >> k) & 1 else "false" for k in range(3)) + "]"


def probe_text(p):
    """debug.rs:388-403 -> bytes."""
    t = p["team_bits"]
    return ("RGB [%d, %d, %d]\nHSV [%d, %d, %d]\nLuma8 %d\nOCRPixelSimilarity %d\nOCRBrightness %d\nAlphaMarker %s\nBravoMarker %s\nCharlieMarker %s"
            % (p["rgb"] + (p["h"], p["s"], p["v"], p["luma"], p["mono"], p["brightness"], _bools(t), _bools(t >> 3), _bools(t >> 6)))).encode("latin-1")


def window_size(S, C):
    return f32(6 * S * C + 16), f32(34 + 72 * S)


def window_pos(point, S, C, W, H):
    """debug.rs:415-420 -> (wp.x, wp.y, Wd, Hd) as f32."""
    mx, my = f32(point[0]), f32(point[1])
    Wd, Hd = window_size(S, C)
    with np.errstate(all="ignore"):
        wx, wy = f32(mx + f32(15.0)), f32(my + f32(15.0))
        if f32(wx + Wd) > f32(W) or f32(wy + Hd) > f32(H):
            wx, wy = f32(f32(mx - Wd) - f32(5.0)), f32(f32(my - Hd) - f32(5.0))
    return wx, wy, Wd, Hd


def frame_color(rgb):
    r, g, b = (f32(v) for v in rgb)
    return BLACK if f32(f32(f32(r * f32(0.299)) + f32(g * f32(0.587))) + f32(b * f32(0.114))) > f32(186.0) else WHITE


def pixel_frame(point, scale):
    """debug.rs:444-463 -> the two corners (x0, y0, x1, y1) as f32."""
    sw, sh = (f32(1.0) if f32(v) == 0 else f32(v) for v in scale)
    with np.errstate(all="ignore"):
        pw, ph = np.floor(sw), np.floor(sh)
        ax, ay = f32(point[0]), f32(point[1])
        if pw > 1:
            ax = f32(ax - np.fmod(ax, pw))
        if ph > 1:
            ay = f32(ay - np.fmod(ay, ph))
        return f32(ax - pw), f32(ay - ph), f32(ax + ph), f32(ay + ph)


def run_anchor(run, scale, top_left):
    x, y, flags = f32(run[0]), f32(run[1]), run[3]
    if flags & MAP_COORDS:
        sw, sh = (f32(1.0) if f32(v) == 0 else f32(v) for v in scale)
        with np.errstate(all="ignore"):
            return f32(f32(x * sw) + f32(top_left[0])), f32(f32(y * sh) + f32(top_left[1]))
    return x, y


def valid_run(run):
    """What the library accepts in a run."""
    x, y, rgba, flags, text = run
    return (rgba[3] == 255 and not (flags & ~MAP_COORDS) and len(text) <= MAX_BYTES and text.count(b"\n") + 1 <= MAX_LINES
            and all(c == 0x0A or c in GLYPHS for c in text))


def items(ui, map_open, has_minimap, runs, points, flags, S, W, H, scale, top_left, consts):
    """A frame's items in paint order and its probes -> ([("text", (px, py), rgb, [line bytes]) | ("fill", (ax, ay, bx, by), rgb) |
    ("frame", (x0, y0, x1, y1), rgb)], [probe dicts])."""
    probes = [probe(ui, map_open, pt, scale, top_left, consts) for pt in points]
    out = []
    if not map_open:
        return out, probes
    for run in runs:
        out.append(("text", run_anchor(run, scale, top_left), tuple(run[2][:3]), run[4].split(b"\n")))
    if (flags & MINIMAP_CAPTION) and not has_minimap:
        out.append(("text", (f32(10.0), f32(f32(f32(H) - f32(10.0)) - f32(9 * S))), CAPTION_RED, [CAPTION]))
    if flags & DRAW_PROBES:
        for pt, p in zip(points, probes):
            if not p["valid"]:
                continue
            lines = probe_text(p).split(b"\n")
            C = max(len(l) for l in lines)
            wx, wy, Wd, Hd = window_pos(pt, S, C, W, H)
            with np.errstate(all="ignore"):
                out.append(("fill", (wx, wy, f32(wx + Wd), f32(wy + Hd)), WINDOW_BG))
                out.append(("text", (f32(wx + f32(8.0)), f32(wy + f32(26.0))), WHITE, lines))
                out.append(("fill", (f32(wx + f32(8.0)), f32(wy + f32(8.0)), f32(f32(wx + Wd) - f32(8.0)), f32(wy + f32(18.0))), p["rgb"]))
            out.append(("frame", pixel_frame(pt, scale), frame_color(p["rgb"])))
    return out, probes


def text_mask(W, H, anchor, lines, S):
    """The pixel rule of a text run -> bool [H, W]."""
    mask = np.zeros((H, W), bool)
    px, py = f32(anchor[0]), f32(anchor[1])
    if not (np.isfinite(px) and np.isfinite(py)):
        return mask
    table = np.zeros((256, 7), np.uint8)
    for ch, rows in GLYPHS.items():
        table[ch] = rows
    with np.errstate(all="ignore"):
        iu = np.floor(((np.arange(W, dtype=f32) + f32(0.5)) - px).astype(f32) / f32(S))
        iv = np.floor(((np.arange(H, dtype=f32) + f32(0.5)) - py).astype(f32) / f32(S))
    xs = np.nonzero((iu >= 0) & (iu < 6 * MAX_BYTES + 6))[0]
    ju = iu[xs].astype(np.int64)
    for Y in np.nonzero((iv >= 0) & (iv < 9 * len(lines)))[0]:
        jv = int(iv[Y])
        line, row = jv // 9, jv % 9 - 1
        text = np.frombuffer(lines[line], np.uint8)
        if not 0 <= row <= 6 or len(text) == 0:
            continue
        ch, col = ju // 6, ju % 6
        ok = (ch < len(text)) & (col < 5)
        bits = (table[text[np.minimum(ch, len(text) - 1)], row] >> np.clip(4 - col, 0, 4)) & 1
        mask[Y, xs[ok & (bits == 1)]] = True
    return mask


def fill_mask(W, H, box):
    ax, ay, bx, by = (f32(v) for v in box)
    cx = np.arange(W, dtype=f32) + f32(0.5)
    cy = np.arange(H, dtype=f32) + f32(0.5)
    with np.errstate(all="ignore"):
        return np.outer((ay <= cy) & (cy < by), (ax <= cx) & (cx < bx))


def item_mask(W, H, item, S):
    if item[0] == "text":
        return text_mask(W, H, item[1], item[3], S)
    if item[0] == "fill":
        return fill_mask(W, H, item[1])
    return YR.rect_mask(W, H, item[1])


def draw(image, item_list, S):
    """Paints the items, in order, onto `image` (H x W x 4 uint8, in place).  Returns the number of pixels whose bytes changed."""
    H, W = image.shape[:2]
    before = image.copy()
    for item in item_list:
        image[item_mask(W, H, item, S)] = np.array(tuple(item[2][:3]) + (255,), np.uint8)
    return int((image != before).any(axis=2).sum())


def debug_pass(image, ui, map_open, has_minimap, runs, points, flags, S, scale, top_left, consts):
    """The whole pass over one frame's image (in place) -> (pixels changed, probes)."""
    H, W = image.shape[:2]
    S = S or 2
    item_list, probes = items(ui, map_open, has_minimap, runs, points, flags, S, W, H, scale, top_left, consts)
    return draw(image, item_list, S), probes
