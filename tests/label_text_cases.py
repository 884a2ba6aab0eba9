"""Inputs of the label-text tests (tests/test_label_text_host.py, tests/test_label_text_gpu.py): frames whose quadrants carry
scale labels with a text, the atlas each is read against, and what the case is there for.

Every case is dict(name, size, key, atlas, expect): `key` names the frame ("V:<name>" a painted quadrant, "strip:<stem>" a strip
of the reference's screenshots, "closed"), frame_of(case) builds it, want_of(case) is its scale-label restatement
(scale_labels_ref.of_frame, cached by key).  `expect` is said of the text restatement (tests/label_text_ref.py) by hand and
check_expect asserts it: texts, meters, and where the case is about them n_glyphs, flags, single best / second / tmpl values,
has, scales, start_y.

Synthetic labels are painted with the helpers of scale_label_cases.py in glyphs of the project's own csrc/smh_font5x7_ascii.h
at scale 1 and 2, each glyph's tight columns followed by one empty column.  A label has to be ONE word of the scale-label rule,
and at 1024 x 768 (g = 1) two glyphs join only through a row in which both reach the empty column between them ("10" has none):
a case is painted at the smallest of 1024 x 768, 1600 x 1024 (g = 2) and 2560 x 1440 (g = 4) at which its labels are one word
each (fit_size; the choice is a property of the text, not of the code under test).  The strips run at 2560 x 1440.
"""
import functools
import os
import re

import numpy as np

import label_text_ref as LT
import scale_label_cases as SC
import scale_labels_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FONT_H = os.path.join(os.path.dirname(HERE), "squad-mortar-helper_amd", "csrc", "smh_font5x7_ascii.h")
SIZES = (SC.SMALL, SC.MID, SC.BIG)


# ---- the font --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def font():
    """{character: bool[7, 5]} of the printable ASCII glyphs of smh_font5x7_ascii.h."""
    with open(FONT_H) as f:
        rows = re.findall(r"\{((?:0x[0-9A-Fa-f]{2},? ?){7})\}", f.read())
    out = {}
    for i, r in enumerate(rows[:95]):
        vals = [int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]{2}", r)]
        out[chr(0x20 + i)] = np.array([[(v >> (4 - x)) & 1 for x in range(5)] for v in vals], bool)
    assert out["1"].tolist()[1] == [False, True, True, False, False] and out["m"][0].sum() == 0
    return out


def piece(ch, scale=1):
    """The glyph's non-empty columns over all 7 * scale rows of its cell (the rows keep the glyphs on one baseline)."""
    b = font()[ch]
    xs = np.flatnonzero(b.any(axis=0))
    b = b[:, xs[0]:xs[-1] + 1]
    return np.kron(b, np.ones((scale, scale), bool))


def tight(b):
    ys, xs = np.flatnonzero(b.any(axis=1)), np.flatnonzero(b.any(axis=0))
    return b[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].copy()


def template(code, ch=None, scale=1):
    return (code, tight(piece(ch or code, scale)))


CHARS = "0123456789m+"
FONT1 = LT.Atlas([template(c) for c in CHARS])
FONT12 = LT.Atlas([template(c) for c in CHARS] + [template(c, scale=2) for c in CHARS])


def text_pieces(text, scale=1):
    return [piece(c, scale) for c in text]


def compose(pieces, gaps=None):
    """Pieces left to right, gaps[k] empty columns before piece k > 0 (default 1) -> bool[H, W], top rows as painted."""
    gaps = [0] + list(gaps if gaps is not None else [1] * (len(pieces) - 1))
    H = max(p.shape[0] for p in pieces)
    W = sum(p.shape[1] for p in pieces) + sum(gaps)
    img, x = np.zeros((H, W), bool), 0
    for p, g in zip(pieces, gaps):
        x += g
        img[:p.shape[0], x:x + p.shape[1]] = p
        x += p.shape[1]
    return img


def fit_size(images):
    """The smallest frame size at whose gap every image is one word."""
    for size in SIZES:
        g = R.gap(SC.geometry(size)[4])
        if all(len(R.components(R.smear(np.pad(im, 1), g))) == 1 for im in images):
            return size
    raise AssertionError("no size joins the label")


def paint(V, l, t, img, lead=2, margin=8):
    """The label image in WHITE with its top-left pixel at (l, t), a bar under it -> its box (left, top, right, bottom)."""
    ys, xs = np.nonzero(img)
    V[t + ys, l + xs] = SC.WHITE
    box = (l + int(xs.min()), t + int(ys.min()), l + int(xs.max()) + 1, t + int(ys.max()) + 1)
    SC.bar(V, box[0] - margin, box[2] - 1 + margin, box[3] + lead)
    return box


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def cases():
    return list(_cases())


def by_name(name):
    return next(c for c in _cases() if c["name"] == name)


_V = {}


def frame_of(case):
    kind, _, rest = case["key"].partition(":")
    if kind == "strip":
        return SC.strip_frame(rest)
    if kind == "closed":
        return SC.closed_frame(case["size"])
    return SC.frame_of(_V[rest], case["size"])


@functools.lru_cache(maxsize=None)
def _want(key, size):
    return R.of_frame(frame_of(dict(key=key, size=size)))


def want_of(case):
    return _want(case["key"], case["size"])


@functools.lru_cache(maxsize=None)
def strip_atlas(stem):
    """The atlas learned from a strip's labels that read as a number of meters, by the restatement's learning helper."""
    want = _want("strip:" + stem, SC.BIG)
    tpl = []
    for cell, box, text in zip(want["crops"], want["labels"], SC.STRIPS[stem]["texts"]):
        if text.endswith("m"):
            tpl += LT.learn(cell, box, text)
    return LT.Atlas(LT.dedup(tpl))


def check_expect(case, fr):
    """fr: label_text_ref.read_frame of the case (or the same dict decoded from a device record)."""
    e, name = case["expect"], case["name"]
    if "n" in e:
        assert fr["n"] == e["n"], (name, fr["n"])
    if "texts" in e:
        assert [lb["text"] for lb in fr["labels"]] == e["texts"], (name, [lb["text"] for lb in fr["labels"]])
    if "meters" in e:
        assert [lb["meters"] for lb in fr["labels"]] == e["meters"], (name, [lb["meters"] for lb in fr["labels"]])
    for k in ("n_glyphs", "flags"):
        if k in e:
            assert [lb[k] for lb in fr["labels"]] == e[k], (name, k, [lb[k] for lb in fr["labels"]])
    for k in ("best", "second", "tmpl"):
        for (i, j), v in e.get(k, {}).items():
            assert fr["labels"][i][k][j] == v, (name, k, i, j, fr["labels"][i][k])
    for k in ("has", "scales", "start_y"):
        if k in e:
            assert fr[k] == e[k], (name, k, fr[k])
    if "truth" in e:                                           # the strips: the two conditions on every genuine glyph
        codes = {c for c, _ in case["atlas"].templates}
        some = 0
        for lb, truth in zip(fr["labels"], e["truth"]):
            if len(truth) != lb["n_glyphs"]:
                continue
            for j, ch in enumerate(truth):
                if ch in codes:
                    fg = int(case["atlas"].templates[lb["tmpl"][j]][1].sum())
                    assert lb["text"][j] == ch and lb["best"][j] * 1000 <= 214 * fg + 50 and lb["second"][j] - lb["best"][j] >= 5, (name, truth, j, lb, fg)
                    some += 1
                else:
                    assert lb["text"][j] == "?", (name, truth, j, lb)
        assert some >= 6, name


@functools.lru_cache(maxsize=None)
def _cases():
    out = []

    def add(name, size, key, atlas, **expect):
        out.append(dict(name=name, size=size, key=key, atlas=atlas, expect=expect))

    def add_painted(name, images, atlas, place=None, size=None, **expect):
        """images: the labels' images, stacked 30 rows apart from (20, 10) unless place = [(l, t, lead, margin)] says otherwise."""
        size = size or fit_size(images)
        V = SC.blank(size)
        boxes = []
        for k, im in enumerate(images):
            l, t, lead, margin = place[k] if place else (20, 10 + 30 * k, 2, 8)
            boxes.append(paint(V, l, t, im, lead, margin))
        V.setflags(write=False)
        _V[name] = V
        add(name, size, "V:" + name, atlas, boxes=boxes, **expect)

    # -- the four strips, leave one out --
    G = "glorious_png"
    others = [s for s in sorted(SC.STRIPS) if s != G]
    for stem in others:
        texts = SC.STRIPS[stem]["texts"]
        add("strip_%s_by_glorious" % stem, SC.BIG, "strip:" + stem, strip_atlas(G), truth=texts,
            texts=[t if t.endswith("m") else "?" for t in texts], meters=[int(t[:-1]) if t.endswith("m") else 0 for t in texts])
    for stem in others:
        add("strip_glorious_by_%s" % stem, SC.BIG, "strip:" + G, strip_atlas(stem), truth=SC.STRIPS[G]["texts"],
            texts=["?00m", "300m", "900m"], meters=[0, 300, 900], has=1)

    # -- parse --
    for text, m in (("33m", 33), ("100m", 100), ("2700m", 2700), ("4294967295m", 4294967295), ("4294967296m", 0), ("m", 0), ("0m", 0), ("007m", 7),
                    ("+5m", 5), ("300", 0), ("3m0m", 0), ("30m0", 30)):
        add_painted("parse_" + text.replace("+", "plus"), [compose(text_pieces(text))], FONT1, texts=[text], meters=[m], n_glyphs=[len(text)], flags=[0],
                    has=int(m != 0))
    t16 = "000000000000123m"
    add_painted("glyphs_16", [compose(text_pieces(t16))], FONT1, texts=[t16], meters=[123], n_glyphs=[16], flags=[0])
    add_painted("glyphs_17", [compose(text_pieces("0" + t16))], FONT1, texts=[""], meters=[0], n_glyphs=[17], flags=[LT.TOO_MANY], has=0)

    # -- geometry --
    # a stray pixel left of / above the glyph moves its box by one: the glyph reads through the shift (-1 along that axis); a stray
    # pixel on the template's side makes the clean glyph the one that has to move by +1
    three = tight(piece("3"))

    def strayed(b, left, top):
        left, top = int(left), int(top)
        b = np.pad(b, ((top, 0), (left, 0)))
        if left:
            ys = np.flatnonzero(b[:, left])
            b[ys[-1], :left] = True                            # a whisker of `left` pixels on the last row that reaches column 0
        if top:
            xs = np.flatnonzero(b[top])
            b[:top, xs[-1]] = True
        return b
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            g3, t3 = strayed(three, dx < 0, dy < 0), strayed(three, dx > 0, dy > 0)
            atlas = LT.Atlas([("3", t3)] + [t for t in FONT1.templates if t[0] != "3"])
            add_painted("shift_%+d_%+d" % (dx, dy), [compose([g3] + text_pieces("5m"))], atlas, texts=["35m"], meters=[35],
                        best={(0, 0): abs(dx) + abs(dy)}, tmpl={(0, 0): 0})
    for name, (left, top) in (("shift_two_left", (2, 0)), ("shift_two_up", (0, 2))):
        add_painted(name, [compose([strayed(three, left, top)] + text_pieces("5m"))], FONT1, texts=["?5m"], meters=[0])
    # a run of 32 columns reads against its template; 33 columns are unmatched
    zero2 = piece("0", 2)
    for cols in (32, 33):
        wide = np.hstack([zero2, zero2, zero2, np.ones((14, cols - 30), bool)])
        atlas = LT.Atlas(FONT12.templates + [("W", np.hstack([zero2, zero2, zero2, np.ones((14, 2), bool)]))])
        exp = dict(texts=["Wm"], best={(0, 0): 0}, tmpl={(0, 0): 24}) if cols == 32 else dict(texts=["?m"], best={(0, 0): 0xFFFF}, second={(0, 0): 0xFFFF}, tmpl={(0, 0): 0xFF})
        add_painted("run_of_%d_columns" % cols, [compose([wide, piece("m", 2)])], atlas, meters=[0], n_glyphs=[2], **exp)
    # a label 128 columns wide: eleven glyphs at scale 2, two at scale 1; what follows the last m is ignored
    im = compose(text_pieces("2700000000m", 2) + text_pieces("11", 1))
    assert im.shape[1] == 128
    add_painted("label_128_wide", [im], FONT12, texts=["2700000000m11"], meters=[2700000000], n_glyphs=[13])
    # a label box 32 rows high: a bar of 32 x 2 pixels among the glyphs, a template of its own
    atlas = LT.Atlas(FONT1.templates + [("|", np.ones((32, 2), bool))])
    im = compose(text_pieces("3m") + [np.ones((32, 2), bool)])
    add_painted("label_32_high", [im], atlas, texts=["3m|"], meters=[3], best={(0, 2): 0}, tmpl={(0, 2): 12})

    # -- choice --
    zero = tight(piece("0"))
    add_painted("equal_bits_two_codes", [compose(text_pieces("0m"))], LT.Atlas([("O", zero), ("0", zero), template("m")]), texts=["Om"], meters=[0],
                best={(0, 0): 0}, second={(0, 0): 0}, tmpl={(0, 0): 0})

    def flipped(ch, k):
        """The scale-2 glyph with k background pixels of its box turned on, spread over the box."""
        b = tight(piece(ch, 2))
        ys, xs = np.nonzero(~b)
        step = len(ys) // k
        b[ys[::step][:k], xs[::step][:k]] = True
        return b
    nine_fg, three_fg = int(piece("9", 2).sum()), int(piece("3", 2).sum())
    assert nine_fg == 60 and three_fg == 56                    # best * 3 == fg: accepted; best * 3 == fg + 1: not
    add_painted("accept_at_fg", [compose([flipped("9", 20), piece("m", 2)])], FONT12, texts=["9m"], meters=[9], best={(0, 0): 20})
    add_painted("accept_at_fg_plus_1", [compose([flipped("3", 19), piece("m", 2)])], FONT12, texts=["?m"], meters=[0], best={(0, 0): 19}, tmpl={(0, 0): 12 + 3})
    add_painted("accept_1_of_2", [compose([flipped("3", 19), piece("m", 2)])], LT.Atlas(FONT12.templates, 1, 2), texts=["3m"], meters=[3], best={(0, 0): 19})
    add_painted("accept_0_of_1", [compose([flipped("9", 1), piece("m", 2)])], LT.Atlas(FONT12.templates, 0, 1), texts=["?m"], meters=[0], best={(0, 0): 1})
    add_painted("atlas_of_one", [compose(text_pieces("m"))], LT.Atlas([template("m")]), texts=["m"], meters=[0], best={(0, 0): 0}, second={(0, 0): 0xFFFF},
                tmpl={(0, 0): 0})

    # -- frame --
    def labels(texts, scale=1):
        return [compose(text_pieces(t, scale)) for t in texts]
    add_painted("frame_duplicates", labels(["300m", "300m", "900m"]), FONT1, texts=["300m", "300m", "900m"], meters=[300, 300, 900], has=1, start_y=17,
                scales=[(300, 31, 17), (900, 31, 77)])
    # four distinct values side by side: the fourth label's bottom is the lowest, and the loop has left before it
    ims = labels(["100m", "300m", "900m"], 2) + labels(["2700m"], 1)
    add_painted("frame_four_distinct", ims, FONT12, place=[(20, 40, 2, 8), (110, 41, 2, 8), (200, 42, 2, 8), (290, 43, 2, 8)], size=SC.BIG,
                texts=["100m", "300m", "900m", "2700m"], meters=[100, 300, 900, 2700], has=1, start_y=54)
    add_painted("frame_non_label_between", labels(["300m", "8", "900m"]), FONT1, texts=["300m", "8", "900m"], meters=[300, 0, 900], has=1,
                scales=[(300, 31, 17), (900, 31, 77)], start_y=17)
    eight = ["7", "100m", "100m", "33m", "5", "300m", "900m", "2700m"]
    add_painted("frame_eight_labels", labels(eight), FONT1, n=8, texts=eight, meters=[0, 100, 100, 33, 0, 300, 900, 2700], has=1, start_y=47)
    add_painted("frame_no_label", labels(["300", "m"]), FONT1, n=2, texts=["300", "m"], meters=[0, 0], has=0, scales=[], start_y=0)
    # a ladder whose mean depends on the order of its sum: the margins give the bars' widths
    ims = labels(["100m", "300m", "900m"])
    w = [im.shape[1] for im in ims]
    pick = None
    for m0 in range(4, 13):
        for m1 in range(4, 13):
            for m2 in range(4, 13):
                r = [float(v) / float(wd + 2 * mg - 3) for v, wd, mg in zip((100, 300, 900), w, (m0, m1, m2))]
                if pick is None and (r[0] + r[1]) + r[2] != (r[2] + r[1]) + r[0]:
                    pick = (m0, m1, m2)
    assert pick is not None
    add_painted("frame_ladder_order", ims, FONT1, place=[(20, 10 + 30 * k, 2, pick[k]) for k in range(3)], size=SC.MID, texts=["100m", "300m", "900m"],
                meters=[100, 300, 900], has=1, ladder=pick)
    add("frame_closed", SC.SMALL, "closed", FONT1, n=0, has=0, texts=[], scales=[], start_y=0)
    over = next(c for c in SC.cases() if c["name"] == "runs_4097")
    _V["frame_runs_overflow"] = over["V"]
    add("frame_runs_overflow", SC.SMALL, "V:frame_runs_overflow", FONT1, n=0, has=0, texts=[], scales=[], start_y=0)
    add_painted("frame_empty", [], FONT1, size=SC.SMALL, n=0, has=0, texts=[])
    return tuple(out)


# ---- the library's side of a case ------------------------------------------------------------------------------------------------
def lib_templates(atlas):
    """The atlas' templates as the library's GlyphTemplate structs."""
    from squad_mortar_helper_amd import _lib as L
    out = []
    for code, b in atlas.templates:
        t = L.GlyphTemplate()
        t.code, t.w, t.h = ord(code), b.shape[1], b.shape[0]
        for y, v in enumerate(LT.template_rows(b)):
            t.rows[y] = v
        out.append(t)
    return out


def label_frame_bytes(want):
    """scale_labels_ref's dict of a frame as the bytes of a smhv_scale_label_frame and of its eight cells."""
    import struct
    cells = np.full((LT.MAX_LABELS, R.CROP_H, R.CROP_W), 255, np.uint8)
    if want is None:
        return bytes(288), cells.tobytes()
    rec = struct.pack("<8I", *want["header"], 0, 0, 0)
    for i in range(LT.MAX_LABELS):
        rec += struct.pack("<8I", *want["labels"][i]) if i < len(want["labels"]) else bytes(32)
    cells[:len(want["labels"])] = want["crops"]
    return rec, cells.tobytes()
