"""Restatement of the reach map for the tests (never imported by the product package): the header's "reach map" in numpy, with the
f32 / f64 semantics of firing_ref.py -- every f32 operation on numpy float32 (IEEE single, unfused), every f64 operation on numpy
float64; +, -, *, / and sqrt are correctly rounded in both, so the device has to agree bit for bit.  Whole windows at once: the
arrays are (out_h + 1) x (out_w + 1), the +1 row and column being the ring rule's neighbours outside the window."""
import numpy as np

import firing_ref as FR

F32 = np.float32
F64 = np.float64
NONE, SCALES, HEIGHTMAP = FR.NONE, FR.SCALES, FR.HEIGHTMAP
OUT_OF_RANGE, BAND0, RING = 1, 2, 0x80
# tan(mils * pi / 3200) for mils = 900 .. 1500, as the header prints them
THRESHOLDS = [float.fromhex(h) for h in ("0x1.37efd8d87607ep+0", "0x1.7f218e25a745fp+0", "0x1.def13b73c1408p+0", "0x1.3504f333f9de6p+1",
                                         "0x1.a5f59e90600d8p+1", "0x1.41bfee2424769p+2", "0x1.44e6c595afdc2p+3")]
MILS = [900, 1000, 1100, 1200, 1300, 1400, 1500]
# smhv_reach_defaults' palette
DEFAULT_PALETTE = dict(out_of_range=(200, 30, 30, 96), ring=(255, 255, 255, 160),
                       band=[(40, 90, 255, 72), (0, 170, 255, 72), (0, 220, 200, 72), (0, 230, 110, 72), (120, 235, 0, 72), (220, 230, 0, 72),
                             (255, 180, 0, 72), (255, 120, 40, 72)])


def _round_i32(x):
    """Rust `f64.round() as i32` on an array: half away from zero, saturating, NaN -> 0 -> int64 array."""
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        t = np.trunc(x)
        t = np.where(np.abs(x - t) >= 0.5, t + np.copysign(1.0, x), t)
        t = np.where(np.isnan(t), 0.0, t)
        t = np.clip(t, -2147483648.0, 2147483647.0)
    return t.astype(np.int64)


def hm_rect(minimap, hm_shape, bounds, fit, sw, sh, tx, ty):
    """firing_ref.firing_line's rectangle -> (rl, rt, rr, rb) as float32."""
    H, W = hm_shape
    left, right, top, bottom = (int(v) for v in minimap)
    off0 = off1 = F32(0.0)
    if not fit:
        b0x, b0y = F32(bounds[0][0]), F32(bounds[0][1])
        mmw, mmh = F32((right - left) & 0xFFFFFFFF), F32((bottom - top) & 0xFFFFFFFF)
        with np.errstate(all="ignore"):
            off0 = F32(F32(b0x * F32(mmw / F32(F32(W) + b0x))) * sw)
            off1 = F32(F32(b0y * F32(mmh / F32(F32(H) + b0y))) * sh)
    rl = F32(F32(F32(F32(left) * sw) + tx) + off0)
    rt = F32(F32(F32(F32(top) * sh) + ty) + off1)
    rr = F32(F32(F32(right) * sw) + tx)
    rb = F32(F32(F32(bottom) * sh) + ty)
    return rl, rt, rr, rb


def _axis(n_px, o, s, t, use_hm, r0, rlen, n):
    """One axis of the window's pixels 0 .. n_px (the last one is the neighbour outside) -> dict(dh, ds, ix, fin)."""
    o, s, t = F32(o), F32(s), F32(t)
    with np.errstate(all="ignore"):
        c = np.arange(n_px + 1).astype(F32) + F32(0.5)
        tg = (c - t) / s                                          # inverse_xy
        assert tg.dtype == F32
        p1 = tg * s + t                                           # translate_xy
        p0 = F32(F32(o * s) + t)
        fin = np.isfinite(tg)
        ds = F64(o) - tg.astype(F64)
        dh = np.zeros(n_px + 1, F64)
        ix = np.full(n_px + 1, -1, np.int64)
        if use_hm:
            c0 = ((F64(p0) - F64(r0)) / F64(rlen)) * F64(n)
            c1 = ((p1.astype(F64) - F64(r0)) / F64(rlen)) * F64(n)
            dh = c0 - c1
            i0, i1 = int(_round_i32(c0)), _round_i32(c1)
            if 0 <= i0 < n:
                ix = np.where((i1 >= 0) & (i1 < n), i1, -1)
    return dict(dh=dh, ds=ds, ix=ix, fin=fin)


def _origin_texel(o, s, t, r0, rlen, n):
    with np.errstate(all="ignore"):
        p0 = F32(F32(F32(o) * F32(s)) + F32(t))
        i0 = int(_round_i32(((F64(p0) - F64(r0)) / F64(rlen)) * F64(n)))
    return i0 if 0 <= i0 < n else -1


def reach(origin, window, viewport=None, minimap=None, mpx=None, hm=None, fit_to_minimap=True, ring_m=0.0):
    """origin = (x, y) map-ROI coordinates or None (no origin); window = (out_w, out_h); viewport = (sw, sh, tx, ty) or None; minimap =
    (left, right, top, bottom) or None; mpx = meters per pixel or None; hm = (data u16 [h, w], bounds, scale) or None.
    -> dict(classes uint8 [out_h, out_w], source uint8 [out_h, out_w] (NONE where the class is 0), meters f64 [out_h, out_w],
    alt f64 [out_h, out_w], valid)."""
    ow, oh = window
    zero = dict(classes=np.zeros((oh, ow), np.uint8), source=np.zeros((oh, ow), np.uint8), meters=np.zeros((oh, ow)), alt=np.zeros((oh, ow)), valid=0,
                origin=(0.0, 0.0))
    if origin is None or not (np.isfinite(F32(origin[0])) and np.isfinite(F32(origin[1]))):
        return zero
    ox, oy = F32(origin[0]), F32(origin[1])
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    sw = F32(1.0) if sw == 0 else sw
    sh = F32(1.0) if sh == 0 else sh
    use_hm = minimap is not None and hm is not None
    rl = rt = F32(0.0)
    rw = rh = 0.0
    W = H = 0
    if use_hm:
        data, bounds, scale = hm
        H, W = data.shape
        rl, rt, rr, rb = hm_rect(minimap, data.shape, bounds, fit_to_minimap, sw, sh, tx, ty)
        rw, rh = F64(F32(rr - rl)), F64(F32(rb - rt))
    col = _axis(ow, ox, sw, tx, use_hm, rl, rw, W)
    row = _axis(oh, oy, sh, ty, use_hm, rt, rh, H)
    with np.errstate(all="ignore"):
        hmok = (row["ix"][:, None] >= 0) & (col["ix"][None, :] >= 0)
        dx = np.where(hmok, col["dh"][None, :], col["ds"][None, :])
        dy = np.where(hmok, row["dh"][:, None], row["ds"][:, None])
        ln = np.sqrt(dx * dx + dy * dy)
        m = np.where(hmok, ln, ln * F64(mpx if mpx is not None else 0.0))
        src = np.where(hmok, HEIGHTMAP, SCALES if mpx is not None else NONE).astype(np.uint8)
        src[~(row["fin"][:, None] & col["fin"][None, :]) | np.isnan(m)] = NONE
        alt = np.zeros_like(m)
        if use_hm and hmok.any():
            ix0, iy0 = _origin_texel(ox, sw, tx, rl, rw, W), _origin_texel(oy, sh, ty, rt, rh, H)
            assert ix0 >= 0 and iy0 >= 0                           # (hmok needs the origin inside)
            zs = F64(F32(scale[2])) / F64(0.1953125)
            h0 = (F64(data[iy0, ix0]) / F64(65535.0)) * zs
            tex = data[np.clip(row["ix"], 0, H - 1)[:, None], np.clip(col["ix"], 0, W - 1)[None, :]]
            alt = np.where(hmok, (tex.astype(F64) / F64(65535.0)) * zs - h0, 0.0)
        disc = FR.V4 - FR.G * (FR.G * (m * m) + 2.0 * alt * FR.V2)
        q = (FR.V2 + np.sqrt(disc)) / (FR.G * m)
        k = np.zeros(m.shape, np.uint8)
        for T in THRESHOLDS:
            k += (q >= T).astype(np.uint8)
        cls = np.where(disc >= 0.0, BAND0 + k, OUT_OF_RANGE).astype(np.uint8)
        cls[src == NONE] = 0
        if ring_m > 0.0:
            b = np.floor(m / F64(ring_m))
            own_s, own_b = src[:-1, :-1], b[:-1, :-1]
            edge = ((src[:-1, 1:] == own_s) & (b[:-1, 1:] != own_b)) | ((src[1:, :-1] == own_s) & (b[1:, :-1] != own_b))
            cls[:-1, :-1] |= np.where(edge & (cls[:-1, :-1] != 0), RING, 0).astype(np.uint8)
    return dict(classes=np.ascontiguousarray(cls[:-1, :-1]), source=np.ascontiguousarray(src[:-1, :-1]), meters=m[:-1, :-1], alt=alt[:-1, :-1], valid=1,
                origin=(float(ox), float(oy)))


def summary(r):
    """The smhv_reach_result of a restated window -> dict(valid, source_mask, origin, count [9], ring)."""
    if not r["valid"]:
        return dict(valid=0, source_mask=0, origin=(0.0, 0.0), count=[0] * 9, ring=0)
    c7 = r["classes"] & 0x7F
    mask = 0
    if (c7 == 0).any():
        mask |= 1
    for s in (SCALES, HEIGHTMAP):
        if ((c7 != 0) & (r["source"] == s)).any():
            mask |= 1 << s
    return dict(valid=1, source_mask=mask, origin=r["origin"], count=[int((c7 == c).sum()) for c in range(1, 10)], ring=int(((r["classes"] & RING) != 0).sum()))


def _blend(img, sel, rgba):
    a = int(rgba[3])
    for ch in range(3):
        c = img[..., ch].astype(np.int64)
        img[..., ch] = np.where(sel, (c * (255 - a) + int(rgba[ch]) * a + 127) // 255, c).astype(np.uint8)


def paint(img, classes, palette=None):
    """SMHV_REACH_PAINT over img (uint8 [h, w, 4], changed in place): the class's colour, then the ring's; alpha untouched."""
    p = palette or DEFAULT_PALETTE
    c7 = classes & 0x7F
    _blend(img, c7 == OUT_OF_RANGE, p["out_of_range"])
    for k in range(8):
        _blend(img, c7 == BAND0 + k, p["band"][k])
    _blend(img, (classes & RING) != 0, p["ring"])
    return img


def sample_line(r, viewport, x, y):
    """The line (origin, target of window pixel (x, y)) as smhv_firing_solutions takes it: the header's t in f32."""
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    sw = F32(1.0) if sw == 0 else sw
    sh = F32(1.0) if sh == 0 else sh
    t0 = F32(F32(F32(x) + F32(0.5)) - tx) / sw
    t1 = F32(F32(F32(y) + F32(0.5)) - ty) / sh
    return (F32(r["origin"][0]), F32(r["origin"][1]), F32(t0), F32(t1))
