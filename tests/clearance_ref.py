"""Restatement of the terrain clearance for the tests (never imported by the product package): the header's "terrain clearance" in
numpy, written from its text.  Every f32 operation runs on numpy float32, every f64 operation on numpy float64; +, -, *, / and sqrt
are correctly rounded in both, so the device has to agree bit for bit.  sample_rule() is the rule's steps 1 to 4, sequential over the
samples k and vectorised over whatever it is given -- the lines of a call or the pixels of a window; lines() and clearance_map() only
differ in where the end points come from."""
import numpy as np

import firing_ref as FR
import reach_ref as RR

F32 = np.float32
F64 = np.float64
MAX_SAMPLES = 256
PROFILE = MAX_SAMPLES + 1
NONE, OUT_OF_RANGE, CLEAR, BLOCKED, LOS_BLOCKED = 0, 1, 2, 3, 0x80
# smhv_clearance_defaults' palette
DEFAULT_PALETTE = dict(out_of_range=(0, 0, 0, 0), clear=(0, 0, 0, 0), blocked=(230, 40, 40, 110), los=(0, 0, 0, 70))
_round_i32 = RR._round_i32


def _zscale(scale):
    return F64(F32(scale[2])) / F64(0.1953125)


def _height(v, zs):
    return (np.asarray(v).astype(F64) / F64(65535.0)) * zs


def arc_height(d, q, x):
    """The arc over the origin at ground distance x (step 3's a), for the hand-worked tests."""
    d, q, x = F64(d), F64(q), F64(x)
    return x * q - ((FR.G * (x * x)) * (1.0 + q * q)) / (2.0 * FR.V2)


def high_angle(d, alt):
    """Steps 1 and 2 -> (disc, q)."""
    with np.errstate(all="ignore"):
        d, alt = np.asarray(d, F64), np.asarray(alt, F64)
        disc = FR.V4 - FR.G * (FR.G * (d * d) + 2.0 * alt * FR.V2)
        q = (FR.V2 + np.sqrt(disc)) / (FR.G * d)
    return disc, q


def sample_rule(x0, y0, x1, y1, h0, alt, d, data, zs, S, margin, want_heights=False):
    """The rule for lines from (x0, y0) to (x1, y1) in heightmap coordinates (arrays that broadcast against each other; h0, alt, d
    have the full shape) -> dict(status, first_blocked, n_blocked, los_blocked, min_margin, min_at[, heights: S - 1 arrays]).  The
    caller masks what has no verdict."""
    H, W = data.shape
    S = int(S)
    with np.errstate(all="ignore"):
        d, alt, h0 = np.asarray(d, F64), np.asarray(alt, F64), np.asarray(h0, F64)
        x0, y0, x1, y1 = (np.asarray(v, F64) for v in (x0, y0, x1, y1))
        shape = d.shape
        disc, q = high_angle(d, alt)
        oor, none = ~(disc >= 0.0), d == 0.0
        live = ~oor & ~none
        qq1 = 1.0 + q * q
        best = np.full(shape, np.inf)
        at = np.zeros(shape, np.int64)
        first = np.full(shape, S, np.int64)
        nb, nl = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        heights = []
        for k in range(1, S):
            t = F64(k) / F64(S)
            ix = np.clip(_round_i32(x0 + (x1 - x0) * t), 0, W - 1)
            iy = np.clip(_round_i32(y0 + (y1 - y0) * t), 0, H - 1)
            hgt = np.broadcast_to(_height(data[iy, ix], zs), shape)
            if want_heights:
                heights.append(hgt)
            z = hgt - h0
            x = d * t
            a = x * q - ((FR.G * (x * x)) * qq1) / (2.0 * FR.V2)
            m = a - z
            blk = live & (m < F64(margin))
            los = ~none & ((alt * t) < z)
            first = np.where(blk & (first == S), k, first)
            nb += blk
            nl += los
            upd = live & (m < best)
            best = np.where(upd, m, best)
            at = np.where(upd, k, at)
        status = np.where(oor, OUT_OF_RANGE, np.where(nb > 0, BLOCKED, CLEAR))
        min_margin = np.where(oor | none | (S == 1), 0.0, best)
    out = dict(status=status, first_blocked=first, n_blocked=nb, los_blocked=nl, min_margin=min_margin, min_at=at)
    if want_heights:
        out["heights"] = heights
    return out


def _view(viewport):
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    return (F32(1.0) if sw == 0 else sw), (F32(1.0) if sh == 0 else sh), tx, ty


def _coord(p, r0, rlen, n):
    """A translated f32 coordinate -> the heightmap coordinate in f64."""
    with np.errstate(all="ignore"):
        return ((np.asarray(p).astype(F64) - F64(r0)) / F64(rlen)) * F64(n)


def _inside(c, n):
    i = _round_i32(c)
    return i, (i >= 0) & (i < n)


_ZERO_DIR = dict(status=0, first_blocked=0, n_blocked=0, los_blocked=0, min_margin=0.0, min_at=0)


def lines(lns, S, margin=0.0, minimap=None, hm=None, fit_to_minimap=True, viewport=None):
    """lns: [n, 4] (x0, y0, x1, y1) in map-ROI coordinates; minimap = (left, right, top, bottom) or None; hm = (data u16 [h, w],
    bounds, scale) or None; viewport = (sw, sh, tx, ty) or None -> (records: a list of n (dir0, dir1), each a dict of the six fields,
    profiles float32 [n, PROFILE])."""
    ln = np.asarray(lns, F32).reshape(-1, 4)
    n = len(ln)
    prof = np.zeros((n, PROFILE), F32)
    if n == 0 or minimap is None or hm is None:
        return [(dict(_ZERO_DIR), dict(_ZERO_DIR)) for _ in range(n)], prof
    data, bounds, scale = hm
    H, W = data.shape
    sw, sh, tx, ty = _view(viewport)
    zs = _zscale(scale)
    with np.errstate(all="ignore"):
        p0x, p0y = ln[:, 0] * sw + tx, ln[:, 1] * sh + ty           # (float32 arrays: IEEE single, unfused)
        p1x, p1y = ln[:, 2] * sw + tx, ln[:, 3] * sh + ty
        assert p0x.dtype == F32
        rl, rt, rr, rb = RR.hm_rect(minimap, data.shape, bounds, fit_to_minimap, sw, sh, tx, ty)
        rw, rh = F64(F32(rr - rl)), F64(F32(rb - rt))
        x0, y0, x1, y1 = _coord(p0x, rl, rw, W), _coord(p0y, rt, rh, H), _coord(p1x, rl, rw, W), _coord(p1y, rt, rh, H)
        dx, dy = x0 - x1, y0 - y1
        d = np.sqrt(dx * dx + dy * dy)
        (ix0, a), (iy0, b), (ix1, c), (iy1, e) = _inside(x0, W), _inside(y0, H), _inside(x1, W), _inside(y1, H)
        ok = a & b & c & e
        v0 = data[np.where(ok, iy0, 0), np.where(ok, ix0, 0)]
        v1 = data[np.where(ok, iy1, 0), np.where(ok, ix1, 0)]
        h0, h1 = _height(v0, zs), _height(v1, zs)
        alt = h1 - h0
    fwd = sample_rule(x0, y0, x1, y1, h0, alt, d, data, zs, S, margin, want_heights=True)
    bck = sample_rule(x1, y1, x0, y0, h1, -alt, d, data, zs, S, margin)
    recs = []
    for i in range(n):
        if not ok[i]:
            recs.append((dict(_ZERO_DIR), dict(_ZERO_DIR)))
            continue
        recs.append(tuple(dict(status=int(r["status"][i]), first_blocked=int(r["first_blocked"][i]), n_blocked=int(r["n_blocked"][i]),
                               los_blocked=int(r["los_blocked"][i]), min_margin=float(r["min_margin"][i]), min_at=int(r["min_at"][i])) for r in (fwd, bck)))
        prof[i, 0], prof[i, S] = F32(h0[i]), F32(h1[i])
        for k in range(1, int(S)):
            prof[i, k] = F32(fwd["heights"][k - 1][i])
    return recs, prof


def _axis(n_px, o, s, t, r0, rlen, n):
    """One axis of the window's pixels -> (the origin's heightmap coordinate, the targets' [n_px], both rounded inside [n_px])."""
    o, s, t = F32(o), F32(s), F32(t)
    with np.errstate(all="ignore"):
        c = np.arange(n_px).astype(F32) + F32(0.5)
        tg = (c - t) / s                                          # inverse_xy
        p1 = tg * s + t                                           # translate_xy
        p0 = F32(F32(o * s) + t)
        assert tg.dtype == F32 and p1.dtype == F32
        c0, c1 = _coord(p0, r0, rlen, n), _coord(p1, r0, rlen, n)
        i0, in0 = _inside(c0, n)
        i1, in1 = _inside(c1, n)
    return F64(c0), c1, int(i0), i1, bool(in0) & in1


def clearance_map(origin, window, S, margin=0.0, viewport=None, minimap=None, hm=None, fit_to_minimap=True):
    """origin = (x, y) map-ROI coordinates or None (no origin); window = (out_w, out_h) -> dict(bytes uint8 [out_h, out_w], valid,
    origin)."""
    ow, oh = window
    zero = dict(bytes=np.zeros((oh, ow), np.uint8), valid=0, origin=(0.0, 0.0))
    if origin is None or not (np.isfinite(F32(origin[0])) and np.isfinite(F32(origin[1]))):
        return zero
    ox, oy = F32(origin[0]), F32(origin[1])
    out = dict(zero, valid=1, origin=(float(ox), float(oy)))
    if minimap is None or hm is None:
        return out
    data, bounds, scale = hm
    H, W = data.shape
    sw, sh, tx, ty = _view(viewport)
    zs = _zscale(scale)
    rl, rt, rr, rb = RR.hm_rect(minimap, data.shape, bounds, fit_to_minimap, sw, sh, tx, ty)
    rw, rh = F64(F32(rr - rl)), F64(F32(rb - rt))
    c0x, c1x, i0x, i1x, okx = _axis(ow, ox, sw, tx, rl, rw, W)
    c0y, c1y, i0y, i1y, oky = _axis(oh, oy, sh, ty, rt, rh, H)
    verdict = oky[:, None] & okx[None, :]
    if not verdict.any():
        return out
    with np.errstate(all="ignore"):
        h0 = _height(data[i0y, i0x], zs)
        tex = data[np.clip(i1y, 0, H - 1)[:, None], np.clip(i1x, 0, W - 1)[None, :]]
        alt = _height(tex, zs) - h0
        dx, dy = (c0x - c1x)[None, :], (c0y - c1y)[:, None]
        d = np.sqrt(dx * dx + dy * dy)
    r = sample_rule(c0x, c0y, c1x[None, :], c1y[:, None], np.full(d.shape, h0), alt, d, data, zs, S, margin)
    b = r["status"].astype(np.uint8) | np.where(r["los_blocked"] > 0, LOS_BLOCKED, 0).astype(np.uint8)
    out["bytes"] = np.where(verdict, b, 0).astype(np.uint8)
    return out


def summary(r):
    """The smhv_clearance_map_result of a restated window -> dict(valid, origin, count [3], los_blocked)."""
    if not r["valid"]:
        return dict(valid=0, origin=(0.0, 0.0), count=[0, 0, 0], los_blocked=0)
    s = r["bytes"] & 0x7F
    return dict(valid=1, origin=r["origin"], count=[int((s == c).sum()) for c in (1, 2, 3)], los_blocked=int(((r["bytes"] & LOS_BLOCKED) != 0).sum()))


def paint(img, b, palette=None):
    """SMHV_CLEAR_PAINT over img (uint8 [h, w, 4], changed in place): the status's colour, then the LOS entry; alpha untouched."""
    p = palette or DEFAULT_PALETTE
    s = b & 0x7F
    RR._blend(img, s == OUT_OF_RANGE, p["out_of_range"])
    RR._blend(img, s == CLEAR, p["clear"])
    RR._blend(img, s == BLOCKED, p["blocked"])
    RR._blend(img, (b & LOS_BLOCKED) != 0, p["los"])
    return img
