"""Restatement of the terrain relief for the tests (never imported by the product package): the header's "terrain relief" in numpy.
The rectangle is reach_ref's (f32, unfused); everything else is numpy float64, where +, -, *, /, floor and sqrt are correctly
rounded, so the device has to agree bit for bit.  One pixel rule, relief(), feeds every output: the flag bytes, the shades, the
heights, the paint and the summary.  Whole windows at once on a grid of (out_h + 1) x (out_w + 2) pixels: X = -1 .. out_w and Y =
0 .. out_h -- the +1 row and column are the neighbours outside the window, and column -1 exists for a mutant's sake alone.

`mutant` changes one rule at a time (tests/test_relief_host.py holds every one against the case family named for its rule):
  "nearest"   the nearest texel for the bilinear height        "round_l"   round for floor in L
  "trunc"     truncating division in the MAJOR rule            "left"      the neighbour (X - 1, Y) for (X + 1, Y)
  "clamp"     neighbours outside the window clamped into it    "den"       1.0 + (p * p + q * q) for (1.0 + p * p) + q * q
  "no_half"   the shade without its + 0.5"""
import numpy as np

import reach_ref as RR

F32 = np.float32
F64 = np.float64
HAS_HEIGHT, CONTOUR, MAJOR = 1, 2, 4
PAINT, BYTES, SHADES, HEIGHTS, NEAREST = 1, 2, 4, 8, 16
# smhv_relief_defaults
DEFAULTS = dict(interval_m=10.0, base_m=0.0, major_every=5, exaggeration=1.0, light=(-0.5, -0.5, float.fromhex("0x1.6a09e667f3bcdp-1")),
                contour=(60, 40, 20, 110), major=(60, 40, 20, 200), shade_weight=96, nearest=False)
MUTANTS = ("nearest", "round_l", "trunc", "left", "clamp", "den", "no_half")


def options(**kw):
    """The library's defaults with `kw` on top."""
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def _axis(n_px, r0, rlen, n):
    """One axis of the pixels -1 .. n_px -> (p f64, inside, i0, i1, f, the rounded coordinate clamped)."""
    with np.errstate(all="ignore"):
        c = np.arange(-1, n_px + 1).astype(F32) + F32(0.5)
        p = ((c.astype(F64) - F64(r0)) / F64(rlen)) * F64(n)
        ri = RR._round_i32(p)
        inside = (ri >= 0) & (ri < n)
        fl = np.floor(p)
        f = p - fl
        i = np.where(np.isfinite(fl), fl, 0.0).astype(np.int64)
    return p, inside, np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), f, np.clip(ri, 0, n - 1)


def relief(window, viewport, minimap, hm, fit_to_minimap=True, opt=None, mutant=None):
    """window = (out_w, out_h); viewport = (sw, sh, tx, ty) or None; minimap = (left, right, top, bottom) or None (a frame without
    relief: a closed one is the same); hm = (data u16 [h, w], bounds, scale); opt = options().
    -> dict(valid, bytes u8 [out_h, out_w], shades u8, heights f32, z f64 (NaN: no height), level f64, px, py (the window's))."""
    assert mutant is None or mutant in MUTANTS, mutant
    o = opt or DEFAULTS
    ow, oh = window
    if minimap is None:
        return dict(valid=0, bytes=np.zeros((oh, ow), np.uint8), shades=np.zeros((oh, ow), np.uint8), heights=np.zeros((oh, ow), F32),
                    z=np.full((oh, ow), np.nan), level=np.full((oh, ow), np.nan), px=np.full(ow, np.nan), py=np.full(oh, np.nan))
    data, bounds, scale = hm
    H, W = data.shape
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    sw = F32(1.0) if sw == 0 else sw
    sh = F32(1.0) if sh == 0 else sh
    nearest = bool(o["nearest"]) or mutant == "nearest"
    with np.errstate(all="ignore"):
        rl, rt, rr, rb = RR.hm_rect(minimap, data.shape, bounds, fit_to_minimap, sw, sh, tx, ty)
        rw, rh = F64(F32(rr - rl)), F64(F32(rb - rt))
        px, in_x, i0, i1, fx, rx = _axis(ow, rl, rw, W)
        py, in_y, j0, j1, fy, ry = _axis(oh, rt, rh, H)
        py, in_y, j0, j1, fy, ry = py[1:], in_y[1:], j0[1:], j1[1:], fy[1:], ry[1:]          # rows 0 .. out_h
        d = data.astype(F64)
        if nearest:
            v = d[ry[:, None], rx[None, :]]
        else:
            gx, gy = F64(1.0) - fx, F64(1.0) - fy
            top = d[j0[:, None], i0[None, :]] * gx[None, :] + d[j0[:, None], i1[None, :]] * fx[None, :]
            bot = d[j1[:, None], i0[None, :]] * gx[None, :] + d[j1[:, None], i1[None, :]] * fx[None, :]
            v = top * gy[:, None] + bot * fy[:, None]
        zs = F64(F32(scale[2])) / F64(0.1953125)
        z = (v / F64(65535.0)) * zs
        has = in_y[:, None] & in_x[None, :] & np.isfinite(z)
        z = np.where(has, z, np.nan)
        # the pixel, its right and its down neighbour
        cols = np.arange(1, ow + 1)
        rcols, drows = cols + (-1 if mutant == "left" else 1), np.arange(1, oh + 1)
        if mutant == "clamp":
            rcols, drows = np.minimum(rcols, ow), np.minimum(drows, oh - 1)
        own, right, down = z[:oh][:, cols], z[:oh][:, rcols], z[drows][:, cols]
        bits = np.where(np.isnan(own), 0, HAS_HEIGHT).astype(np.uint8)
        level = np.full(own.shape, np.nan)
        if o["interval_m"] > 0.0:
            rnd = (lambda a: np.floor(a + 0.5)) if mutant == "round_l" else np.floor
            lv = rnd((z - F64(o["base_m"])) / F64(o["interval_m"]))
            level = lv[:oh][:, cols]
            M = int(o["major_every"])
            for other in (lv[:oh][:, rcols], lv[drows][:, cols]):
                cross = np.isfinite(level) & np.isfinite(other) & (level != other)
                bits |= np.where(cross, CONTOUR, 0).astype(np.uint8)
                if M >= 1:
                    lo, hi = np.minimum(level, other), np.maximum(level, other)
                    step = np.trunc if mutant == "trunc" else np.floor
                    bits |= np.where(cross & (step(hi / F64(M)) != step(lo / F64(M))), MAJOR, 0).astype(np.uint8)
        mx, my = F64(W) / rw, F64(H) / rh
        ex = F64(o["exaggeration"])
        lx, ly, lz = (F64(c) for c in o["light"])
        p = np.where(np.isnan(right), 0.0, ((right - own) * ex) / mx)
        q = np.where(np.isnan(down), 0.0, ((down - own) * ex) / my)
        t = (lz - p * lx) - q * ly
        den = np.sqrt(F64(1.0) + (p * p + q * q)) if mutant == "den" else np.sqrt((F64(1.0) + p * p) + q * q)
        s = t / den
        s = np.where(s > 0.0, s, 0.0)
        s = np.where(s > 1.0, 1.0, s)
        shades = np.where(np.isnan(own), 0.0, np.floor(s * 255.0 + (0.0 if mutant == "no_half" else 0.5))).astype(np.uint8)
        heights = np.where(np.isnan(own), 0.0, own).astype(F32)
    return dict(valid=1, bytes=np.ascontiguousarray(bits), shades=np.ascontiguousarray(shades), heights=np.ascontiguousarray(heights), z=own,
                level=level, px=px[1:ow + 1], py=py[:oh], den=den, s=s)


def summary(r):
    """The smhv_relief_result of a restated window -> dict(valid, n_height, n_contour, n_major, z_min, z_max)."""
    has = (r["bytes"] & HAS_HEIGHT) != 0
    if not r["valid"] or not has.any():
        return dict(valid=int(r["valid"]), n_height=0, n_contour=0, n_major=0, z_min=0.0, z_max=0.0)
    z = r["z"][has]
    return dict(valid=1, n_height=int(has.sum()), n_contour=int(((r["bytes"] & CONTOUR) != 0).sum()), n_major=int(((r["bytes"] & MAJOR) != 0).sum()),
                z_min=float(z.min()), z_max=float(z.max()))


def _blend(img, sel, rgb, a):
    """reach_ref's blend with a colour per pixel: rgb = three arrays or ints."""
    for ch in range(3):
        c = img[..., ch].astype(np.int64)
        img[..., ch] = np.where(sel, (c * (255 - int(a)) + np.asarray(rgb[ch], np.int64) * int(a) + 127) // 255, c).astype(np.uint8)


def paint(img, r, opt=None):
    """SMHV_RELIEF_PAINT over img (uint8 [h, w, 4], changed in place): the shade, then the contour's or the index contour's colour, on
    pixels with a height; alpha untouched."""
    o = opt or DEFAULTS
    b = r["bytes"]
    has = (b & HAS_HEIGHT) != 0
    sh = r["shades"].astype(np.int64)
    _blend(img, has, (sh, sh, sh), o["shade_weight"])
    _blend(img, has & ((b & CONTOUR) != 0) & ((b & MAJOR) == 0), o["contour"][:3], o["contour"][3])
    _blend(img, has & ((b & CONTOUR) != 0) & ((b & MAJOR) != 0), o["major"][:3], o["major"][3])
    return img
