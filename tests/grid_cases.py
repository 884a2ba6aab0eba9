"""Inputs of the map-grid tests, shared by the host and the device tests.  Every case says what it is for and checks, on the
restatement (grid_ref.py), that it contains it: a case that no longer sits on its boundary fails on the CPU before it reaches a GPU.
`family` names the rule a case guards; tests/test_grid_host.py holds the restatement with that rule changed against the family.

Two geometries carry most cases.  UNIT: a 128 x 64 heightmap on the minimap rectangle (0, 128, 0, 64) with no viewport, so m = c
exactly (both divisions are by powers of two) and with origin_m = (0.5, 0.5) g = X at the centre of pixel X.  TEN: a 1280 x 640
heightmap on the same rectangle, m = 10 c, with origin_m = (5, 5) g = 10 X."""
import collections
import functools
import math

import numpy as np

import grid_ref as G

TW, TH = 64, 16                                                   # k_grid's tile (csrc/smh_kernels.h, SMH_REACH_TW / SMH_REACH_TH)
NO_BOUNDS = ((0, 0), (0, 0))
RECT = (0, 128, 0, 64)                                            # left, right, top, bottom
WINDOW = (97, 66)                                                 # two tiles across with one column in the second, five down with two rows in the last
SMALL = (65, 17)
LINE = ((9, 8, 7, 200), (60, 50, 40, 150), (100, 110, 120, 99), (200, 210, 220, 60))
LABEL = (250, 240, 10, 222)

Case = collections.namedtuple("Case", "name family hm minimap window viewport fit mpx opt lines check")


@functools.lru_cache(maxsize=None)
def heightmap(w, h, bounds=NO_BOUNDS):
    """The grid reads a heightmap's size and bounds alone."""
    return np.zeros((h, w), np.uint16), bounds, (1.0, 1.0, 10.0)


@functools.lru_cache(maxsize=None)
def _restated(name, mutant):
    c = next(k for k in all_cases() if k.name == name)
    return G.grid(c.window, c.viewport, c.minimap, c.hm, c.fit, c.mpx, c.opt, mutant), G.line_refs(c.lines, c.viewport, c.minimap, c.hm, c.fit, c.mpx, c.opt, mutant)


def restate(c, mutant=None, **opt):
    """The case's window restated (computed once per case and mutant and shared: nobody changes it); opt: with these options on top."""
    if not opt:
        return _restated(c.name, mutant)[0]
    return G.grid(c.window, c.viewport, c.minimap, c.hm, c.fit, c.mpx, dict(c.opt, **opt), mutant)


def restate_refs(c, mutant=None):
    return _restated(c.name, mutant)[1]


def checked(c):
    """The case's restatement and its lines' references, after the case's own check."""
    r, refs = restate(c), restate_refs(c)
    c.check(c, r, refs)
    return r, refs


def _lines(window):
    ow, oh = window
    return np.array([[0.5, 0.5, ow / 2.0, oh / 2.0], [ow - 0.75, oh - 0.25, -3.0, 1e9], [ow / 3.0, oh / 5.0, ow + 40.0, 2.0]], np.float32)


def _case(name, family, check, hm=(128, 64), minimap=RECT, window=WINDOW, viewport=None, fit=True, mpx=None, lines=None, bounds=NO_BOUNDS, **opt):
    o = G.options(**dict(dict(line=LINE, label=LABEL), **opt))
    return Case(name, family, heightmap(hm[0], hm[1], bounds) if hm else None, minimap, window, viewport, fit, mpx, o,
                _lines(window) if lines is None else np.asarray(lines, np.float32).reshape(-1, 4), check)


def _levels(r):
    return set(int(v) for v in np.unique(r["level"]))


# ---- checks
def _check_on_the_line(c, r, refs):
    ow, oh = c.window
    assert np.array_equal(r["gx"], np.arange(ow)) and np.array_equal(r["gy"], np.arange(oh)) and r["ld"] == 3
    # the pixel on the line belongs to the new cell; its left neighbour carries the line, of the coarsest level that differs
    assert r["col"][26] == 0 and r["col"][27] == 1 and r["row1"][26] == 1 and r["row1"][27] == 2
    assert r["level"][0, 26] == 0 and r["level"][0, 27] == 3 and r["level"][0, 8] == 1 and r["level"][0, 2] == 2 and r["level"][26, 30] == 0
    assert _levels(r) == {0, 1, 2, 3, 4} and (r["level"][:64] < 4).all() and (r["level"][64:] == 4).all()   # (rows 64 and 65 lie below the rectangle)
    assert int(r["cells"][0, 0]) == 0 | 1 << 10 | 7 << 20 | 7 << 24 | 7 << 28 and int(r["cells"][26, 26]) == 0 | 1 << 10 | 3 << 20 | 3 << 24 | 3 << 28


def _check_exact(values):
    def check(c, r, refs):
        for X, g in values:
            assert r["gx"][X] == g and r["gy"][min(X, c.window[1] - 1)] == min(X, c.window[1] - 1) * 10.0, (c.name, X, float(r["gx"][X]))
        assert r["ld"] == c.opt["levels"] and r["valid"] and G.summary(r)["n_cell"] == c.window[0] * 64
        assert r["lit"].any() and len(_levels(r)) == c.opt["levels"] + 2
    return check


def _check_negative(c, r, refs):
    assert r["col"][39] == -1 and r["col"][40] == 0 and r["row1"][19] == -1 and r["row1"][20] == 1
    assert r["gx"][39] == -1.0 and not r["bytes"][:, :40].any() and not r["bytes"][:20].any() and r["bytes"][20:64, 40:].all()
    assert int(r["cells"][20, 40]) == 0 | 1 << 10 | 7 << 20 | 7 << 24 | 7 << 28


def _check_names(col_pair, row_pair):
    def check(c, r, refs):
        assert (int(r["col"][19]), int(r["col"][20])) == col_pair and (int(r["row1"][9]), int(r["row1"][10])) == row_pair, (c.name, r["col"][18:22], r["row1"][8:12])
        lit = r["lit"]
        for (x0, x1, cc) in ((0, 20, col_pair[0]), (20, 60, col_pair[1])):
            for (y0, y1, rr) in ((0, 10, row_pair[0]), (10, 50, row_pair[1])):
                n = 0 if cc < 0 or rr < 0 else len(G.letters(cc) + str(rr))
                box = lit[y0:y1, x0:x1]
                assert n or not box.any(), (c.name, cc, rr)
                if n and x1 - x0 == 40 and y1 - y0 == 40:       # a whole cell: the label's extent is its length
                    cols = np.flatnonzero(box.any(axis=0))
                    assert 3 <= cols.min() <= 4 and 6 * n - 1 <= cols.max() <= 6 * n + 1 and np.flatnonzero(box.any(axis=1)).tolist() == list(range(3, 10)), (c.name, cols)
    return check


def _check_ld(want, labels=None):
    def check(c, r, refs):
        assert r["ld"] == want, (c.name, r["ld"], want)
        assert _levels(r) == set(range(want + 1)) | {4}
        if labels is not None:
            assert bool(r["lit"].any()) == labels, c.name
    return check


def _check_tile_borders(c, r, refs):
    lit = r["lit"]
    assert r["col"][59] == 0 and r["col"][60] == 1 and r["row1"][11] == 1 and r["row1"][12] == 2
    box = lit[15:22, 63:74]
    assert box.any() and lit[:, :TW].any() and lit[:, TW:].any() and lit[:TH].any() and lit[TH:].any()
    assert box[:, :1].any() and box[:, 1:].any() and box[:1].any() and box[1:].any()      # "B2" straddles column 64 and row 16


def _check_partial(c, r, refs):
    assert r["col"][0] == 0 and r["row1"][0] == 1 and r["gx"][0] == 10.0
    lit = r["lit"]
    assert lit[:5, :4].any() and not lit[5:50, :50].any() and not lit[:5, 4:50].any()     # the rest of "A1" lies outside the window
    assert restate(c, "window")["lit"][:5, :4].tolist() != lit[:5, :4].tolist()


def _check_clipped(c, r, refs):
    assert r["col"][20] == 26 and r["row1"][10] == 10 and r["col"][40] == 27
    cell = r["lit"][10:30, 20:40]
    assert cell[:, 15:].any() and cell.any(axis=0).sum() < 4 * 5      # "AA10" needs 26 columns, the cell has 20: the last glyph is cut
    assert not r["lit"][10:30, 40:43].any()


def _check_source(source, cells, ends=None):
    def check(c, r, refs):
        s = G.summary(r)
        assert (r["valid"], r["source"]) == (int(source != G.NONE), source) and (s["n_cell"] > 0) == cells, (c.name, s)
        assert refs[0] == source and any(p["valid"] for p in refs[1]) == (cells if ends is None else ends)
        if not cells:
            assert not r["bytes"].any() and not r["cells"].any()
    return check


def _check_offset(c, r, refs):
    _check_source(G.HEIGHTMAP, True)(c, r, refs)
    other = G.grid(c.window, c.viewport, c.minimap, c.hm, True, c.mpx, c.opt)
    assert not np.array_equal(other["cells"], r["cells"]) and r["ax"]["r0"] != other["ax"]["r0"]
    assert r["ax"]["mul"] == 100.0 and r["ay"]["mul"] == 40.0


def _check_mpx_zero(c, r, refs):
    s = G.summary(r)
    assert r["source"] == G.SCALES and s["n_cell"] > 0 and s["n_line"] == (0, 0, 0, 0) and s["n_label"] == 0 and r["ld"] == c.opt["levels"]
    assert (s["col_first"], s["col_last"], s["row_first"], s["row_last"]) == (0, 0, 1, 1)


def _check_ends(c, r, refs):
    source, p = refs
    assert source == G.HEIGHTMAP
    assert (p[0]["x_m"], p[0]["y_m"], p[0]["text"].rstrip(b"\0"), p[0]["valid"]) == (27.0, 54.0, b"B3-7-7-7", 1)          # exactly on a cell corner
    assert (p[1]["x_m"], p[1]["text"].rstrip(b"\0")) == (26.75, b"A2-3-3-3")
    assert [q["valid"] for q in p[2:8]] == [0] * 6 and p[2]["x_m"] == 199.5 and p[3]["y_m"] == -5.5                       # outside the rectangle
    assert (p[4]["x_m"], p[4]["y_m"]) == (0.0, 0.5) and (p[5]["x_m"], p[6]["y_m"]) == (0.0, 0.0)                          # not finite
    assert p[8]["text"].rstrip(b"\0") == b"E3-6-7-8" and p[9]["text"].rstrip(b"\0") == b"A1-7-7-7"


def _up(v, d):
    return v if d == 0 else math.nextafter(v, math.inf if d > 0 else -math.inf)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    out.append(_case("pixel centres on the lines", "ceil", _check_on_the_line, origin_m=(0.5, 0.5), cell_m=27.0, levels=3, min_px=0.0))
    ten = dict(hm=(1280, 640), origin_m=(5.0, 5.0), min_px=0.0, label_min_px=30.0)
    out.append(_case("cell 300, levels 3", "per_level", _check_exact([(50, 500.0), (90, 900.0)]), cell_m=300.0, levels=3, **ten))
    out.append(_case("cell 300, levels 2", "per_level", _check_exact([(90, 900.0)]), cell_m=300.0, levels=2, **ten))
    out.append(_case("cell 256, levels 3", "top123", _check_exact([(64, 640.0)]), cell_m=256.0, levels=3, **dict(ten, label_min_px=25.0)))
    out.append(_case("the origin inside the window", "trunc", _check_negative, origin_m=(40.5, 20.5), cell_m=27.0, levels=3, min_px=0.0))
    # letters and rows: cells of 40 pixels, a column boundary at X = 20 and a row boundary at Y = 10
    for name, cols, rows in (("Z | AA, 9 | 10", (25, 26), (9, 10)), ("ZZ | none, 99 | 100", (701, -1), (99, 100)), ("Y | Z, 999 | 1000", (24, 25), (999, -1))):
        ox, oy = 20.5 - 40.0 * (cols[0] + 1), 10.5 - 40.0 * rows[0]
        out.append(_case(name, "letters", _check_names(cols, rows), origin_m=(ox, oy), cell_m=40.0, levels=1, label_min_px=40.0))
    # the drawn levels: size_k * ppm with ppm = 0.1, min_px at it and one ulp either side
    for k in range(4):
        v = float((np.float64(300.0) / np.float64(G.P3[k])) * (np.float64(128.0) / np.float64(1280.0)))
        for d in (-1, 0, 1):
            out.append(_case("min_px %s size_%d * ppm" % (("below", "at", "above")[d + 1], k), "ld", _check_ld(k if d <= 0 else k - 1), window=SMALL,
                             cell_m=300.0, levels=3, **dict(ten, min_px=_up(v, d), label_min_px=-1.0)))
    for d in (-1, 0, 1):
        out.append(_case("label_min_px %s size_0 * ppm" % ("below", "at", "above")[d + 1], "ld", _check_ld(1, d <= 0), window=SMALL,
                         cell_m=300.0, levels=1, **dict(ten, label_min_px=_up(30.0, d))))
    out.append(_case("x and y disagree on the drawn levels", "ld", _check_ld(1), hm=(64, 64), minimap=(0, 64, 0, 64), viewport=(2.0, 1.0, 0.0, 0.0),
                     origin_m=(0.25, 0.5), cell_m=27.0, levels=3, min_px=5.0))
    # labels
    out.append(_case("a label across the tile borders", "labels", _check_tile_borders, origin_m=(0.5, -47.5), cell_m=60.0, levels=0))
    out.append(_case("a cell that begins left of and above the window", "window", _check_partial, origin_m=(-9.5, -4.5), cell_m=60.0, levels=0))
    out.append(_case("a cell narrower than its label", "labels", _check_clipped, origin_m=(20.5 - 20.0 * 26, 10.5 - 20.0 * 9), cell_m=20.0, levels=0,
                     label_min_px=20.0))
    # both sources
    out.append(_case("bounds offset, a non-square heightmap", "source", _check_offset, hm=(100, 40), bounds=((7, -5), (0, 0)), minimap=(10, 110, 5, 60), fit=False,
                     cell_m=25.0, levels=2, min_px=0.0, label_min_px=20.0))
    scales = dict(hm=None, minimap=(3, 120, 2, 60), viewport=(1.25, 0.75, -4.0, 2.5), cell_m=20.0, levels=2, min_px=2.0, label_min_px=15.0)
    out.append(_case("the scales branch", "source", _check_source(G.SCALES, True), mpx=0.75, **scales))
    out.append(_case("the scales branch, an origin", "source", _check_source(G.SCALES, True, False), mpx=1.0 / 3.0, **dict(scales, origin_m=(-7.3, 11.9))))
    out.append(_case("mpx 0", "source", _check_mpx_zero, mpx=0.0, **scales))
    for name, v in (("negative", -0.75), ("infinite", math.inf), ("NaN", math.nan)):
        out.append(_case("mpx " + name, "source", _check_source(G.SCALES, False), mpx=v, **scales))
    out.append(_case("no metres per pixel and no heightmap", "source", _check_source(G.NONE, False), **scales))
    out.append(_case("no minimap rectangle", "source", _check_source(G.NONE, False), minimap=None, cell_m=27.0))
    out.append(_case("no minimap rectangle, the scales branch", "source", _check_source(G.NONE, False), **dict(scales, minimap=None, mpx=0.75)))
    out.append(_case("a minimap of zero width", "source", _check_source(G.HEIGHTMAP, False), minimap=(50, 50, 2, 60), cell_m=27.0))
    out.append(_case("a minimap of zero width, the scales branch", "source", _check_source(G.SCALES, False), **dict(scales, minimap=(50, 50, 2, 60), mpx=0.75)))
    nan, inf = math.nan, math.inf
    out.append(_case("line ends", "ends", _check_ends, origin_m=(0.5, 0.5), cell_m=27.0, levels=3, min_px=0.0, window=SMALL,
                     lines=[[27.5, 54.5, 27.25, 53.5], [200.0, 10.0, -5.0, -5.0], [nan, 1.0, inf, 2.0], [3.0, -inf, 64.0, 64.0], [127.5, 63.5, 0.5, 0.5]]))
    assert len(set(c.name for c in out)) == len(out)
    return tuple(out)


def family(name):
    return [c for c in all_cases() if c.family == name]
