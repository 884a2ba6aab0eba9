"""Restatement of the map grid for the tests (never imported by the product package): the header's "map grid" in numpy and plain
Python, written from its text.  The rectangle is reach_ref's (f32, unfused); everything else is numpy float64, where -, *, / and
floor are correctly rounded, and Python integers, so the device has to agree bit for bit.  Whole windows at once: the columns
X = 0 .. out_w and the rows Y = 0 .. out_h (the +1 are the neighbours outside the window); Xfirst by looking at every column the
header allows, X - 32 .. X, through the forward rule.  The font is the library's own, read through smhv_text_font.

`mutant` changes one rule at a time (tests/test_grid_host.py holds every one against the case family named for its rule):
  "ceil"       ceil for floor in qf                      "top123"     1 2 3 on the keypad's top row
  "per_level"  a division per level, no integer hierarchy "trunc"      truncating division by 3
  "finest"     a pair crosses at its finest differing level, not its coarsest
  "window"     Xfirst / Yfirst sought inside the window only"""
import ctypes as C
import functools

import numpy as np

import reach_ref as RR
import relief_ref as RELIEF

F32 = np.float32
F64 = np.float64
PAINT, BYTES, CELLS = 1, 2, 4
HAS_CELL, LABEL = 1, 0x10
NONE, SCALES, HEIGHTMAP = 0, 1, 2
MAX_COLS, MAX_ROWS = 702, 999
SPAN = 32                                                        # columns left of a pixel that can decide its label
P3 = (1, 3, 9, 27)
# smhv_grid_defaults
DEFAULTS = dict(cell_m=300.0, levels=2, origin_m=(0.0, 0.0), min_px=12.0, label_min_px=48.0,
                line=((0, 0, 0, 170), (0, 0, 0, 110), (0, 0, 0, 70), (0, 0, 0, 45)), label=(0, 0, 0, 200))
MUTANTS = ("ceil", "top123", "per_level", "trunc", "finest", "window")


def options(**kw):
    """The library's defaults with `kw` on top."""
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


@functools.lru_cache(maxsize=None)
def font():
    """{character: its seven row bytes, bit 4 = the leftmost column}, from the library (a host function)."""
    import squad_mortar_helper_amd as smh
    lib = smh._lib.load()
    rows, out = (C.c_uint8 * 7)(), {}
    for ch in "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ":
        assert lib.smhv_text_font(ord(ch), rows) == 0
        out[ch] = tuple(rows)
    return out


def letters(col):
    """Bijective base 26: A .. Z, AA .. ZZ."""
    assert 0 <= col < MAX_COLS
    return chr(65 + col) if col < 26 else chr(65 + (col - 26) // 26) + chr(65 + (col - 26) % 26)


def ref_text(col, row1, digits=()):
    return letters(col) + str(int(row1)) + "".join("-%d" % d for d in digits)


def frame(viewport, minimap, hm, fit, mpx, opt):
    """The frame's source and its two axes -> (source, ax, ay); an axis = dict(r0, r1 f32, den, mul, ppm, rlen, origin, cell_m, L)."""
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    sw = F32(1.0) if sw == 0 else sw
    sh = F32(1.0) if sh == 0 else sh
    source = NONE if minimap is None else HEIGHTMAP if hm is not None else SCALES if mpx is not None else NONE
    if source == NONE:
        return NONE, None, None
    L, cell = int(opt["levels"]), F64(opt["cell_m"])
    with np.errstate(all="ignore"):
        if source == HEIGHTMAP:
            H, W = hm[0].shape
            rl, rt, rr, rb = RR.hm_rect(minimap, hm[0].shape, hm[1], fit, sw, sh, tx, ty)
        else:
            rl, rt, rr, rb = RR.hm_rect(minimap, (1, 1), ((0, 0), (0, 0)), True, sw, sh, tx, ty)    # no bounds offset on the scales branch
        axes = []
        for r0, r1, n, s, org in ((rl, rr, W if source == HEIGHTMAP else 0, sw, opt["origin_m"][0]), (rt, rb, H if source == HEIGHTMAP else 0, sh, opt["origin_m"][1])):
            rlen = F64(F32(r1 - r0))
            if source == HEIGHTMAP:
                den, mul, ppm = rlen, F64(n), rlen / F64(n)
            else:
                den, mul, ppm = F64(s), F64(mpx), F64(s) / F64(mpx)
            axes.append(dict(r0=F32(r0), r1=F32(r1), den=den, mul=mul, ppm=ppm, rlen=rlen, origin=F64(org), cell_m=cell, L=L))
    return source, axes[0], axes[1]


def _div3(v, mutant):
    if mutant == "trunc":
        return np.where(v < 0, -((-v) // 3), v // 3)
    return v // 3                                                 # numpy's integer // floors


def entries(ax, c, mutant=None):
    """The axis entries of the f32 coordinates c -> dict(g, inn, has, idx = [idx_0 .. idx_L] as int64 arrays (0 where has is not set))."""
    c = np.asarray(c, F32)
    L = ax["L"]
    with np.errstate(all="ignore"):
        m = ((c.astype(F64) - F64(ax["r0"])) / ax["den"]) * ax["mul"]
        g = m - ax["origin"]
        fin = np.isfinite(g)
        inn = (ax["r0"] <= c) & (c < ax["r1"]) & fin
        rnd = np.ceil if mutant == "ceil" else np.floor

        def level(k):
            qf = rnd(g / (ax["cell_m"] / F64(P3[k])))
            ok = fin & (qf >= -2.0 ** 31) & (qf < 2.0 ** 31)
            return ok, np.where(ok, qf, 0.0).astype(np.int64)
        has, top = level(L)
        idx = [None] * (L + 1)
        idx[L] = top
        for k in range(L - 1, -1, -1):
            idx[k] = level(k)[1] if mutant == "per_level" else _div3(idx[k + 1], mutant)
    return dict(g=g, inn=inn, has=has, idx=idx)


def _axis_cell(e, limit):
    return e["inn"] & e["has"] & (e["idx"][0] >= 0) & (e["idx"][0] < limit)


def drawn_levels(ax, ay, opt):
    ld = -1
    with np.errstate(all="ignore"):
        for k in range(ax["L"] + 1):
            size = ax["cell_m"] / F64(P3[k])
            if size * ax["ppm"] >= F64(opt["min_px"]) and size * ay["ppm"] >= F64(opt["min_px"]):
                ld = k
    return ld


def labels_drawn(ax, ay, ld, opt):
    with np.errstate(all="ignore"):
        return bool(ld >= 0 and int(opt["label"][3]) != 0 and ax["rlen"] > 0 and ay["rlen"] > 0 and
                    ax["cell_m"] * ax["ppm"] >= F64(opt["label_min_px"]) and ax["cell_m"] * ay["ppm"] >= F64(opt["label_min_px"]))


def _first(ax, n, own0, mutant):
    """Xfirst of the columns 0 .. n - 1: the least column of X - 32 .. X whose entry has the column's own idx_0."""
    out = np.zeros(n, np.int64)
    for X in range(n):
        cand = np.arange(0 if mutant == "window" else X - SPAN, X + 1)
        e = entries(ax, cand.astype(F32) + F32(0.5), mutant)
        same = e["has"] & (e["idx"][0] == own0[X])
        out[X] = cand[np.argmax(same)] if same.any() else X
    return out


def _cross(ia, ib, both, ld, mutant):
    """The level at which the entries a and b (lists of idx_k arrays) cross -> int array, 4 = none."""
    lvl = np.full(ia[0].shape, 4, np.int64)
    order = range(0, ld + 1) if mutant == "finest" else range(ld, -1, -1)     # the last assignment stands
    for k in order:
        lvl = np.where(both & (ia[k] != ib[k]), k, lvl)
    return lvl


def grid(window, viewport, minimap, hm, fit=True, mpx=None, opt=None, mutant=None):
    """window = (out_w, out_h); viewport = (sw, sh, tx, ty) or None; minimap = (left, right, top, bottom) or None (a closed frame is the
    same); hm = (data u16 [h, w], bounds, scale) or None: the scales branch with mpx (None: the frame has none); opt = options().
    -> dict(valid, source, ld, bytes u8 [out_h, out_w], cells u32, level (4: none), lit, col, row1 (per column / row, -1: none))."""
    assert mutant is None or mutant in MUTANTS, mutant
    o = opt or DEFAULTS
    ow, oh = window
    source, ax, ay = frame(viewport, minimap, hm, fit, mpx, o)
    if source == NONE:
        return dict(valid=0, source=NONE, ld=-1, bytes=np.zeros((oh, ow), np.uint8), cells=np.zeros((oh, ow), np.uint32),
                    level=np.full((oh, ow), 4), lit=np.zeros((oh, ow), bool))
    L = ax["L"]
    ex = entries(ax, np.arange(ow + 1).astype(F32) + F32(0.5), mutant)
    ey = entries(ay, np.arange(oh + 1).astype(F32) + F32(0.5), mutant)
    okx, oky = _axis_cell(ex, MAX_COLS), _axis_cell(ey, MAX_ROWS)
    has = oky[:oh, None] & okx[None, :ow]
    ld = drawn_levels(ax, ay, o)
    # lines: the right and the down pair
    xl = _cross([i[:ow] for i in ex["idx"]], [i[1:] for i in ex["idx"]], okx[:ow] & okx[1:], ld, mutant)
    yl = _cross([i[:oh] for i in ey["idx"]], [i[1:] for i in ey["idx"]], oky[:oh] & oky[1:], ld, mutant)
    level = np.where(has, np.minimum(xl[None, :], yl[:, None]), 4)
    # the cell words
    col, row1 = ex["idx"][0][:ow], ey["idx"][0][:oh] + 1
    cells = col[None, :] | (row1[:, None] << 10)
    for k in range(1, L + 1):
        cx, cy = ex["idx"][k][:ow] % 3, ey["idx"][k][:oh] % 3       # (numpy's % is non-negative)
        digit = (cy[:, None] * 3 + cx[None, :] + 1) if mutant == "top123" else ((2 - cy[:, None]) * 3 + cx[None, :] + 1)
        cells = cells | (digit << (16 + 4 * k))
    cells = np.where(has, cells, 0).astype(np.uint32)
    # the labels
    lit = np.zeros((oh, ow), bool)
    if labels_drawn(ax, ay, ld, o):
        glyphs = font()
        xf, yf = _first(ax, ow, ex["idx"][0], mutant), _first(ay, oh, ey["idx"][0], mutant)
        for Y in range(oh):
            oy = Y - int(yf[Y]) - 3
            if not oky[Y] or not 0 <= oy <= 6:
                continue
            for X in range(ow):
                ox = X - int(xf[X]) - 3
                if not okx[X] or ox < 0 or ox % 6 >= 5:
                    continue
                text = letters(int(col[X])) + str(int(row1[Y]))
                if ox // 6 < len(text):
                    lit[Y, X] = bool((glyphs[text[ox // 6]][oy] >> (4 - ox % 6)) & 1)
    b = np.where(has, HAS_CELL | np.where(level < 4, (level + 1) << 1, 0) | np.where(lit, LABEL, 0), 0).astype(np.uint8)
    return dict(valid=1, source=source, ld=ld, bytes=np.ascontiguousarray(b), cells=np.ascontiguousarray(cells), level=level, lit=lit & has,
                col=np.where(okx[:ow], col, -1), row1=np.where(oky[:oh], row1, -1), gx=ex["g"][:ow], gy=ey["g"][:oh], ax=ax, ay=ay)


def summary(r):
    """The smhv_grid_result of a restated window -> dict."""
    out = dict(valid=int(r["valid"]), source=int(r["source"]), drawn_levels=int(r["ld"]) + 1 if r["valid"] else 0, n_cell=0, n_line=(0, 0, 0, 0), n_label=0,
               col_first=0, col_last=0, row_first=0, row_last=0)
    b = r["bytes"]
    has = (b & HAS_CELL) != 0
    if r["valid"] and has.any():
        c = r["cells"][has]
        out.update(n_cell=int(has.sum()), n_line=tuple(int((((b >> 1) & 7) == k + 1).sum()) for k in range(4)), n_label=int(((b & LABEL) != 0).sum()),
                   col_first=int((c & 1023).min()), col_last=int((c & 1023).max()), row_first=int(((c >> 10) & 1023).min()), row_last=int(((c >> 10) & 1023).max()))
    return out


def paint(img, r, opt=None):
    """SMHV_GRID_PAINT over img (uint8 [h, w, 4], changed in place): line[k] on a pixel of line level k, then label on a lit pixel."""
    o = opt or DEFAULTS
    for k in range(4):
        RELIEF._blend(img, r["level"] == k, o["line"][k][:3], o["line"][k][3])
    RELIEF._blend(img, r["lit"], o["label"][:3], o["label"][3])
    return img


def point_ref(ax, ay, px, py, mutant=None):
    """The reference of a translated point (f32) -> dict(x_m, y_m, col, row1, digit (3), valid, text bytes [16])."""
    ex, ey = entries(ax, [px], mutant), entries(ay, [py], mutant)
    gx, gy = float(ex["g"][0]), float(ey["g"][0])
    out = dict(x_m=gx if np.isfinite(gx) else 0.0, y_m=gy if np.isfinite(gy) else 0.0, col=0, row1=0, digit=(0, 0, 0), valid=0, text=bytes(16))
    if not (_axis_cell(ex, MAX_COLS)[0] and _axis_cell(ey, MAX_ROWS)[0]):
        return out
    L = ax["L"]
    digits = []
    for k in range(1, L + 1):
        cx, cy = int(ex["idx"][k][0]) % 3, int(ey["idx"][k][0]) % 3
        digits.append(cy * 3 + cx + 1 if mutant == "top123" else (2 - cy) * 3 + cx + 1)
    col, row1 = int(ex["idx"][0][0]), int(ey["idx"][0][0]) + 1
    out.update(col=col, row1=row1, digit=tuple(digits + [0] * (3 - L)), valid=1, text=ref_text(col, row1, digits).encode("ascii").ljust(16, b"\0"))
    return out


def line_refs(lines, viewport, minimap, hm, fit=True, mpx=None, opt=None, mutant=None):
    """The references of the ends of lines (float32 [n, 4], map-ROI coordinates) -> (source, [2 n dicts])."""
    o = opt or DEFAULTS
    source, ax, ay = frame(viewport, minimap, hm, fit, mpx, o)
    ln = np.asarray(lines, F32).reshape(-1, 4)
    zero = dict(x_m=0.0, y_m=0.0, col=0, row1=0, digit=(0, 0, 0), valid=0, text=bytes(16))
    if source == NONE:
        return NONE, [dict(zero) for _ in range(2 * len(ln))]
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    sw = F32(1.0) if sw == 0 else sw
    sh = F32(1.0) if sh == 0 else sh
    out = []
    with np.errstate(all="ignore"):
        for x0, y0, x1, y1 in ln:
            for x, y in ((x0, y0), (x1, y1)):
                out.append(point_ref(ax, ay, F32(F32(x * sw) + tx), F32(F32(y * sh) + ty), mutant))
    return source, out
