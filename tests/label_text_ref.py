"""Independent restatement of "scale labels: text" (include/smh_vision_hip.h; test infrastructure): cut, distance, choice, parse
and the frame's anchors, written from the header's text in plain Python / numpy.  It does not call the library, and it is not
formulated as the library is: glyphs and templates are 2-D bool arrays placed on a common plane, not rows of bits.

A template is (code: str of one character, bitmap: bool[h, w]); an atlas is Atlas(templates, num, den).  `Rule` carries one switch
per rule that tests/test_label_text_host.py changes to show that some case notices.
"""
import struct
from collections import namedtuple

import numpy as np

MAX_GLYPHS, MAX_TEMPLATES, MAX_LABELS, MAX_SCALES = 16, 32, 8, 3
TOO_MANY = 1
NONE16, NONE8 = 0xFFFF, 0xFF
REC_BYTES, ENTRY_BYTES = 960, 112

Atlas = namedtuple("Atlas", "templates num den", defaults=(1, 3))
Rule = namedtuple("Rule", "shifts tie_low accept_on find brk", defaults=(True, True, "template", "rfind", True))
RULE = Rule()


# ---- cut -----------------------------------------------------------------------------------------------------------------------
def cut(cell, box):
    """cell: uint8[32, 128]; box: (left, top, right, bottom, ...) -> [bool[h, w]]: the tight bitmaps of the maximal runs of
    non-empty columns of cell[:bottom - top, :right - left] != 255, left to right."""
    w, h = box[2] - box[0], box[3] - box[1]
    fg = np.asarray(cell)[:h, :w] != 255
    cols = fg.any(axis=0)
    glyphs, x = [], 0
    while x < cols.size:
        if not cols[x]:
            x += 1
            continue
        x1 = x
        while x1 < cols.size and cols[x1]:
            x1 += 1
        g = fg[:, x:x1]
        ys = np.flatnonzero(g.any(axis=1))
        glyphs.append(g[ys[0]:ys[-1] + 1].copy())
        x = x1
    return glyphs


# ---- distance ------------------------------------------------------------------------------------------------------------------
def shift_distance(G, T, dx, dy):
    """Positions of the plane at which G moved by (dx, dy) differs from T; both anchored at their top-left corner."""
    H, W = max(G.shape[0], T.shape[0]) + 2, max(G.shape[1], T.shape[1]) + 2
    a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    a[1 + dy:1 + dy + G.shape[0], 1 + dx:1 + dx + G.shape[1]] = G
    b[1:1 + T.shape[0], 1:1 + T.shape[1]] = T
    return int((a != b).sum())


def distance(G, T, rule=RULE):
    steps = (-1, 0, 1) if rule.shifts else (0,)
    return min(shift_distance(G, T, dx, dy) for dy in steps for dx in steps)


# ---- choice --------------------------------------------------------------------------------------------------------------------
def choose(G, atlas, rule=RULE):
    """-> (character, best, second, template index)"""
    if G.shape[1] > 32:
        return "?", NONE16, NONE16, NONE8
    d = [distance(G, T, rule) for _, T in atlas.templates]
    best = min(d)
    winners = [i for i, v in enumerate(d) if v == best]
    win = winners[0] if rule.tie_low else winners[-1]
    code = atlas.templates[win][0]
    others = [v for v, (c, _) in zip(d, atlas.templates) if c != code]
    second = min(others) if others else NONE16
    fg = int(atlas.templates[win][1].sum()) if rule.accept_on == "template" else int(G.sum())
    ok = ((best * atlas.den) & 0xFFFFFFFF) <= ((atlas.num * fg) & 0xFFFFFFFF)
    return (code if ok else "?"), best, second, win


# ---- text to meters ------------------------------------------------------------------------------------------------------------
def meters_of(text, rule=RULE):
    """rfind('m'), then Rust's u32::from_str on the prefix: an optional single '+', one or more ASCII digits, no overflow."""
    p = text.rfind("m") if rule.find == "rfind" else text.find("m")
    if p < 0:
        return 0
    body = text[:p]
    if body.startswith("+"):
        body = body[1:]
    if not body or any(c not in "0123456789" for c in body):
        return 0
    v = int(body)
    return v if v <= 0xFFFFFFFF else 0


# ---- frame ---------------------------------------------------------------------------------------------------------------------
def anchors_of(labels, meters, rule=RULE):
    """labels: [(left, top, right, bottom, bar_left, bar_y, bar_right, width)] -> (start_y, [(meters, x, y)], mpx, has)"""
    scales, start_y, total = [], None, 0.0
    for lb, m in zip(labels, meters):
        if m == 0:
            continue
        start_y = lb[3] if start_y is None else min(start_y, lb[3])
        if any(s[0] == m for s in scales):
            continue
        if len(scales) == MAX_SCALES:                      # (only reached without the break)
            continue
        scales.append((m, (lb[0] + lb[2]) // 2, lb[3]))
        ratio = float(m) / float(lb[6] - lb[4])
        total = total + ratio if len(scales) > 1 else ratio
        if rule.brk and len(scales) == MAX_SCALES:
            break
    if not scales:
        return 0, [], 0.0, 0
    return start_y, scales, (total if len(scales) == 1 else total / float(len(scales))), 1


def read_label(cell, box, atlas, rule=RULE):
    """-> dict(text, n_glyphs, flags, meters, best, second, tmpl)"""
    glyphs = cut(cell, box)
    if len(glyphs) > MAX_GLYPHS:
        return dict(text="", n_glyphs=len(glyphs), flags=TOO_MANY, meters=0, best=[], second=[], tmpl=[])
    got = [choose(G, atlas, rule) for G in glyphs]
    text = "".join(g[0] for g in got)
    return dict(text=text, n_glyphs=len(glyphs), flags=0, meters=meters_of(text, rule), best=[g[1] for g in got], second=[g[2] for g in got],
                tmpl=[g[3] for g in got])


def read_frame(want, atlas, rule=RULE):
    """want: scale_labels_ref's dict of the frame (None: the map is closed) -> dict(n, has, mpx, start_y, scales, labels=[read_label])"""
    if want is None or want["header"][4] != 0:
        return dict(n=0, has=0, mpx=0.0, start_y=0, scales=[], labels=[])
    labels = [read_label(c, b, atlas, rule) for c, b in zip(want["crops"], want["labels"])]
    start_y, scales, mpx, has = anchors_of(want["labels"], [lb["meters"] for lb in labels], rule)
    return dict(n=len(labels), has=has, mpx=mpx, start_y=start_y, scales=scales, labels=labels)


# ---- the records' bytes ----------------------------------------------------------------------------------------------------------
def pack_anchors(start_y, scales):
    flat = [v for s in scales for v in s] + [0] * (3 * (MAX_SCALES - len(scales)))
    return struct.pack("<2I9I", len(scales), start_y, *flat)


def pack_frame(fr):
    """smhv_label_text_frame, 960 bytes, as the header lays it out."""
    out = struct.pack("<IId", fr["n"], fr["has"], fr["mpx"]) + pack_anchors(fr["start_y"], fr["scales"]) + struct.pack("<I", 0)
    for i in range(MAX_LABELS):
        if i >= fr["n"]:
            out += bytes(ENTRY_BYTES)
            continue
        lb = fr["labels"][i]
        k = len(lb["best"])
        out += lb["text"].encode("latin-1").ljust(MAX_GLYPHS, b"\0") + struct.pack("<4I", lb["n_glyphs"], lb["flags"], lb["meters"], 0)
        out += struct.pack("<16H", *(lb["best"] + [0] * (MAX_GLYPHS - k))) + struct.pack("<16H", *(lb["second"] + [0] * (MAX_GLYPHS - k)))
        out += bytes(lb["tmpl"] + [0] * (MAX_GLYPHS - k))
    assert len(out) == REC_BYTES
    return out


# ---- templates -------------------------------------------------------------------------------------------------------------------
def learn(cell, box, text):
    """The learning helper restated: glyph k of the label pairs with text[k] -> [(code, bitmap)]; None where the helper refuses."""
    glyphs = cut(cell, box)
    if len(glyphs) != len(text) or len(glyphs) > MAX_GLYPHS or any(g.shape[1] > 32 for g in glyphs):
        return None
    if any(not (0x21 <= ord(c) <= 0x7E) or c == "?" for c in text):
        return None
    return list(zip(text, glyphs))


def dedup(templates):
    seen, out = set(), []
    for c, b in templates:
        key = (c, b.shape, b.tobytes())
        if key not in seen and len(out) < MAX_TEMPLATES:
            seen.add(key)
            out.append((c, b))
    return out


def template_rows(bitmap):
    """bool[h, w] -> the 32 row words of a smhv_glyph_template"""
    rows = [0] * 32
    for y in range(bitmap.shape[0]):
        for x in np.flatnonzero(bitmap[y]):
            rows[y] |= 1 << int(x)
    return rows
