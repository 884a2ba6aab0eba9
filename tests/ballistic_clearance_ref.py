"""Restatement of "ballistic clearance" for the tests (never imported by the product package): the header's section in numpy f64,
written from its text.  +, -, *, / and sqrt are correctly rounded in numpy as on the device, so everything here has to agree with the
device bit for bit.  The end points, the texels and the heights are "terrain clearance"'s (tests/clearance_ref.py's helpers), the
weapon's terms, roots and status bits "ballistics"' (tests/ballistics_ref.py).  sample_rule() is the one rule, sequential over the
samples k and vectorised over whatever it is given -- the lines of a call or the pixels of a window; lines() and clearance_map() only
differ in where the end points come from and in what they keep of its answer.

Every function takes `mut`, a set of switches that each change ONE rule (tests/test_ballistic_clearance_host.py holds every one of
them against the cases named for it):
  swap_arcs         the high and the low arc swapped
  qq1_other         1 + T * T taken from the other arc
  skip_unusable     the march skipped for an arc whose bal is not 0
  class_precedence  the map's classes 2 (unusable) and 4 (blocked) in the other order
  choice_no_bal     choice ignoring bal
  los_not_oor       the LOS bit left unset on out-of-range pixels
  margin_le         <= in place of < at the margin"""
import numpy as np

import ballistics_ref as B
import clearance_ref as CR
import reach_ref as RR

F32 = np.float32
F64 = np.float64
MUTANTS = ("swap_arcs", "qq1_other", "skip_unusable", "class_precedence", "choice_no_bal", "los_not_oor", "margin_le")
HIGH, LOW = B.HIGH, B.LOW
S_OUT_OF_RANGE, S_CLEAR, S_BLOCKED = CR.OUT_OF_RANGE, CR.CLEAR, CR.BLOCKED      # an arc's status in a line record
C_NONE, C_OUT_OF_RANGE, C_UNUSABLE, C_CLEAR, C_BLOCKED, C_LOS = 0, 1, 2, 3, 4, 0x80   # an arc's class in the map's byte
MAX_SAMPLES = CR.MAX_SAMPLES
# smhv_ballistic_clearance_defaults' palette
DEFAULT_PALETTE = dict(pal=[(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (230, 40, 40, 110)], switch_arc=(240, 190, 40, 110), los=(0, 0, 0, 70))


def arc_height(k, d, T, x):
    """The arc over the origin at ground distance x, for the hand-worked cases."""
    d, T, x = F64(d), F64(T), F64(x)
    return x * T - ((k["g"] * (x * x)) * (1.0 + T * T)) / (2.0 * k["v2"])


def texels(x0, y0, x1, y1, h0, data, zs, shape):
    """terrain(k, t) of lines from (x0, y0) to (x1, y1) in heightmap coordinates (arrays that broadcast to `shape`): the texel of sample
    k, rounded and clamped, as metres over the origin's h0."""
    H, W = data.shape
    x0, y0, x1, y1 = (np.asarray(v, F64) for v in (x0, y0, x1, y1))
    h0 = np.asarray(h0, F64)

    def terrain(kk, t):
        ix = np.clip(RR._round_i32(x0 + (x1 - x0) * t), 0, W - 1)
        iy = np.clip(RR._round_i32(y0 + (y1 - y0) * t), 0, H - 1)
        return np.broadcast_to(CR._height(data[iy, ix], zs), shape) - h0
    return terrain


def sample_rule(k, d, alt, S, margin, terrain, mut=()):
    """The rule for lines of range d and altitude difference alt (arrays of one shape), k = ballistics_ref.rule(weapon), terrain(k, t) =
    the terrain z over the origin at sample k -> dict(arc=[high, low], each dict(status, first_blocked, n_blocked, min_margin, min_at, bal,
    T); los_blocked, disc).  The caller masks what has no verdict."""
    S = int(S)
    with np.errstate(all="ignore"):
        d, alt = np.asarray(d, F64), np.asarray(alt, F64)
        shape = d.shape
        disc, gm, t_hi, t_lo = B.roots(k, d, alt)
        T = [t_lo, t_hi] if "swap_arcs" in mut else [t_hi, t_lo]
        qq1 = [1.0 + t * t for t in T]
        if "qq1_other" in mut:
            qq1 = qq1[::-1]
        bal = [B.status(k, disc, d, t) for t in T]
        oor, none = ~(disc >= 0.0), d == 0.0
        live = [~oor & ~none & ~((b != 0) & ("skip_unusable" in mut)) for b in bal]
        den = 2.0 * k["v2"]
        best = [np.full(shape, np.inf) for _ in T]
        at = [np.zeros(shape, np.int64) for _ in T]
        first = [np.full(shape, S, np.int64) for _ in T]
        nb = [np.zeros(shape, np.int64) for _ in T]
        nl = np.zeros(shape, np.int64)
        for kk in range(1, S):
            t = F64(kk) / F64(S)
            z = terrain(kk, t)
            x = d * t
            gxx = k["g"] * (x * x)
            nl += ~none & ((alt * t) < z)
            for a in (HIGH, LOW):
                m = (x * T[a] - (gxx * qq1[a]) / den) - z
                blk = live[a] & ((m <= F64(margin)) if "margin_le" in mut else (m < F64(margin)))
                first[a] = np.where(blk & (first[a] == S), kk, first[a])
                nb[a] += blk
                upd = live[a] & (m < best[a])
                best[a] = np.where(upd, m, best[a])
                at[a] = np.where(upd, kk, at[a])
        arcs = []
        for a in (HIGH, LOW):
            status = np.where(oor, S_OUT_OF_RANGE, np.where(nb[a] > 0, S_BLOCKED, S_CLEAR))
            arcs.append(dict(status=status, first_blocked=first[a], n_blocked=nb[a], min_margin=np.where(np.isinf(best[a]) & (best[a] > 0), 0.0, best[a]),
                             min_at=at[a], bal=bal[a], T=T[a]))
    return dict(arc=arcs, los_blocked=nl, disc=disc)


def choice(own, status, bal, mut=()):
    """1 + the arc to fire, or 0 (scalars)."""
    for a in (own, 1 - own):
        if status[a] == S_CLEAR and (bal[a] == 0 or "choice_no_bal" in mut):
            return 1 + a
    return 0


def _record(w, r, i, d, alt, mut=()):
    """Element i of sample_rule()'s answer as a direction's record."""
    arcs = [dict(status=int(r["arc"][a]["status"][i]), first_blocked=int(r["arc"][a]["first_blocked"][i]), n_blocked=int(r["arc"][a]["n_blocked"][i]),
                 bal=int(r["arc"][a]["bal"][i]), min_margin=float(r["arc"][a]["min_margin"][i]), min_at=int(r["arc"][a]["min_at"][i])) for a in (HIGH, LOW)]
    return dict(arc=arcs, meters=float(d), alt_delta=float(alt), los_blocked=int(r["los_blocked"][i]),
                choice=choice(w.arc, [x["status"] for x in arcs], [x["bal"] for x in arcs], mut))


def march(w, d, alt, S, margin, z, mut=()):
    """One direction of one line over a given terrain: z[k - 1] = metres over the origin at sample k -> the direction's record."""
    z = np.asarray(z, F64)
    r = sample_rule(B.rule(w), np.array([d], F64), np.array([alt], F64), S, margin, lambda kk, t: z[kk - 1:kk], mut)
    return _record(w, r, 0, d, alt, mut)


def lines(w, lns, S, margin=0.0, minimap=None, hm=None, fit_to_minimap=True, viewport=None, mut=()):
    """w = a ballistics_ref.Weapon; the rest as clearance_ref.lines takes it -> a list of n (dir0, dir1), each None (no verdict: a record
    of zeros) or dict(arc=[high, low] of dict(status, first_blocked, n_blocked, bal, min_margin, min_at), meters, alt_delta, los_blocked,
    choice)."""
    ln = np.asarray(lns, F32).reshape(-1, 4)
    n = len(ln)
    if n == 0 or minimap is None or hm is None:
        return [(None, None) for _ in range(n)]
    k = B.rule(w)
    data, bounds, scale = hm
    H, W = data.shape
    sw, sh, tx, ty = CR._view(viewport)
    zs = CR._zscale(scale)
    with np.errstate(all="ignore"):
        p0x, p0y = ln[:, 0] * sw + tx, ln[:, 1] * sh + ty           # (float32 arrays: IEEE single, unfused)
        p1x, p1y = ln[:, 2] * sw + tx, ln[:, 3] * sh + ty
        assert p0x.dtype == F32
        rl, rt, rr, rb = RR.hm_rect(minimap, data.shape, bounds, fit_to_minimap, sw, sh, tx, ty)
        rw, rh = F64(F32(rr - rl)), F64(F32(rb - rt))
        x0, y0, x1, y1 = CR._coord(p0x, rl, rw, W), CR._coord(p0y, rt, rh, H), CR._coord(p1x, rl, rw, W), CR._coord(p1y, rt, rh, H)
        dx, dy = x0 - x1, y0 - y1
        d = np.sqrt(dx * dx + dy * dy)
        (ix0, a), (iy0, b), (ix1, c), (iy1, e) = CR._inside(x0, W), CR._inside(y0, H), CR._inside(x1, W), CR._inside(y1, H)
        ok = a & b & c & e
        v0 = data[np.where(ok, iy0, 0), np.where(ok, ix0, 0)]
        v1 = data[np.where(ok, iy1, 0), np.where(ok, ix1, 0)]
        h0, h1 = CR._height(v0, zs), CR._height(v1, zs)
        alt = h1 - h0
    fwd = sample_rule(k, d, alt, S, margin, texels(x0, y0, x1, y1, h0, data, zs, d.shape), mut)
    bck = sample_rule(k, d, -alt, S, margin, texels(x1, y1, x0, y0, h1, data, zs, d.shape), mut)
    recs = []
    for i in range(n):
        if not ok[i]:
            recs.append((None, None))
            continue
        pair = []
        for r, al in ((fwd, alt[i]), (bck, -alt[i])):
            pair.append(_record(w, r, i, d[i], al, mut))
        recs.append(tuple(pair))
    return recs


def arc_class(r, a, none, mut=()):
    """The class of arc a of sample_rule()'s answer, for pixels with a verdict."""
    oor = ~(r["disc"] >= 0.0)
    blocked, unus = ~none & (r["arc"][a]["n_blocked"] > 0), r["arc"][a]["bal"] != 0
    if "class_precedence" in mut:
        c = np.where(blocked, C_BLOCKED, np.where(unus, C_UNUSABLE, C_CLEAR))
    else:
        c = np.where(unus, C_UNUSABLE, np.where(blocked, C_BLOCKED, C_CLEAR))
    return np.where(oor, C_OUT_OF_RANGE, c).astype(np.uint8)


def clearance_map(w, origin, window, S, margin=0.0, viewport=None, minimap=None, hm=None, fit_to_minimap=True, mut=()):
    """origin = (x, y) map-ROI coordinates or None (no origin); window = (out_w, out_h)
    -> dict(bytes uint8 [out_h, out_w], margin float32 [out_h, out_w], valid, origin)."""
    ow, oh = window
    zero = dict(bytes=np.zeros((oh, ow), np.uint8), margin=np.full((oh, ow), np.nan, F32), valid=0, origin=(0.0, 0.0))
    if origin is None or not (np.isfinite(F32(origin[0])) and np.isfinite(F32(origin[1]))):
        return zero
    ox, oy = F32(origin[0]), F32(origin[1])
    out = dict(zero, valid=1, origin=(float(ox), float(oy)))
    if minimap is None or hm is None:
        return out
    k = B.rule(w)
    data, bounds, scale = hm
    H, W = data.shape
    sw, sh, tx, ty = CR._view(viewport)
    zs = CR._zscale(scale)
    rl, rt, rr, rb = RR.hm_rect(minimap, data.shape, bounds, fit_to_minimap, sw, sh, tx, ty)
    rw, rh = F64(F32(rr - rl)), F64(F32(rb - rt))
    c0x, c1x, i0x, i1x, okx = CR._axis(ow, ox, sw, tx, rl, rw, W)
    c0y, c1y, i0y, i1y, oky = CR._axis(oh, oy, sh, ty, rt, rh, H)
    verdict = oky[:, None] & okx[None, :]
    if not verdict.any():
        return out
    with np.errstate(all="ignore"):
        h0 = CR._height(data[i0y, i0x], zs)
        tex = data[np.clip(i1y, 0, H - 1)[:, None], np.clip(i1x, 0, W - 1)[None, :]]
        alt = CR._height(tex, zs) - h0
        dx, dy = (c0x - c1x)[None, :], (c0y - c1y)[:, None]
        d = np.sqrt(dx * dx + dy * dy)
    r = sample_rule(k, d, alt, S, margin, texels(c0x, c0y, c1x[None, :], c1y[:, None], h0, data, zs, d.shape), mut)
    none, oor = d == 0.0, ~(r["disc"] >= 0.0)
    own, oth = arc_class(r, w.arc, none, mut), arc_class(r, 1 - w.arc, none, mut)
    los = (r["los_blocked"] > 0) & ~(oor & ("los_not_oor" in mut))
    b = own | (oth << 3) | np.where(los, C_LOS, 0).astype(np.uint8)
    out["bytes"] = np.where(verdict, b, 0).astype(np.uint8)
    with np.errstate(all="ignore"):
        mm = np.where(none | (int(S) == 1), 0.0, r["arc"][w.arc]["min_margin"]).astype(F32)
    out["margin"] = np.where(verdict & (own >= C_CLEAR), mm, F32(np.nan)).astype(F32)
    return out


def split(b):
    """The map's bytes -> (own class, other class, LOS, switch)."""
    own, oth = b & 7, (b >> 3) & 7
    return own, oth, (b & C_LOS) != 0, ((own == C_UNUSABLE) | (own == C_BLOCKED)) & (oth == C_CLEAR)


def summary(r):
    """The smhv_ballistic_clearance_map_result of a restated window -> dict(valid, origin, own [4], other [4], los_blocked, switch_arc)."""
    if not r["valid"]:
        return dict(valid=0, origin=(0.0, 0.0), own=[0] * 4, other=[0] * 4, los_blocked=0, switch_arc=0)
    own, oth, los, sw = split(r["bytes"])
    return dict(valid=1, origin=r["origin"], own=[int((own == c).sum()) for c in (1, 2, 3, 4)], other=[int((oth == c).sum()) for c in (1, 2, 3, 4)],
                los_blocked=int(los.sum()), switch_arc=int(sw.sum()))


def paint(img, b, palette=None):
    """SMHV_BCLR_PAINT over img (uint8 [h, w, 4], changed in place): the own class's colour, then the switch's, then the LOS entry."""
    p = palette or DEFAULT_PALETTE
    own, _, los, sw = split(b)
    for c in (1, 2, 3, 4):
        RR._blend(img, own == c, p["pal"][c - 1])
    RR._blend(img, sw, p["switch_arc"])
    RR._blend(img, los, p["los"])
    return img
