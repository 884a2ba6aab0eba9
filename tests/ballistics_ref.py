"""Restatement of "ballistics" for the tests (never imported by the product package): the header's section in numpy f64, written from
its text.  +, -, *, /, sqrt, floor and fabs are correctly rounded in numpy as on the device, so everything here has to agree with
the device and with the host entry points bit for bit -- except the elevation, whose atan is the C library's (math.atan); pow and tan
of the weapon's terms are the C library's too (math.pow, math.tan), as the header says.  A pixel's source, range and altitude are the
reach map's (tests/reach_ref.py); a line's are the firing solutions' (tests/firing_ref.py).

Every function takes `mut`, a set of switches that each change ONE rule (tests/test_ballistics_host.py holds every one of them
against the cases of the family named for it):
  swap_arcs       the high and the low arc swapped
  mils6000        6000 in place of 6400
  limit_gt        a limit compared with > in place of >=
  no_min_range    the minimum range ignored
  iso_left        the isochrone taken from the left neighbour, not the right one
  tof_other_root  the time of flight from the other root
  apex_no_clamp   the apex without the T <= 0 clamp"""
import math
from dataclasses import dataclass

import numpy as np

import firing_ref as FR
import reach_ref as R

F64 = np.float64
MUTANTS = ("swap_arcs", "mils6000", "limit_gt", "no_min_range", "iso_left", "tof_other_root", "apex_no_clamp")
HIGH, LOW = 0, 1
MILS6400, MILS6000, DEGREES = 0, 1, 2
OUT_OF_RANGE, BELOW_MIN_RANGE, ELEV_LOW, ELEV_HIGH = 1, 2, 4, 8       # status bits
C_OUT_OF_RANGE, C_BELOW_MIN_RANGE, C_ELEV_LOW, C_ELEV_HIGH, C_BAND0, C_ISO = 1, 2, 3, 4, 5, 0x80   # the class byte
NONE, SCALES, HEIGHTMAP = R.NONE, R.SCALES, R.HEIGHTMAP
RAD_PER_DEG = float.fromhex("0x1.1df46a2529d39p-6")
QUARTER_TURN = float.fromhex("0x1.921fb54442d18p+0")
DEG_PER_RAD = 180.0 / math.pi
# smhv_ballistic_defaults' palette
DEFAULT_PALETTE = dict(pal=[(200, 30, 30, 96), (120, 120, 120, 96), (150, 60, 160, 96), (90, 60, 200, 96)] + R.DEFAULT_PALETTE["band"], iso=(255, 255, 255, 160))


@dataclass(frozen=True)
class Weapon:
    """smhv_weapon; the defaults are smhv_weapon_defaults' (the reference's mortar)."""
    velocity: float = 109.890938
    gravity: float = 9.8
    arc: int = HIGH
    unit: int = MILS6400
    elev_min: float = 0.0
    elev_max: float = 1600.0
    range_min: float = 0.0
    dispersion: float = 0.0


def unit_deg(unit, mut=()):
    if unit == MILS6400:
        return 360.0 / (6000.0 if "mils6000" in mut else 6400.0)
    return 360.0 / 6000.0 if unit == MILS6000 else 1.0


def tanlim(e, ud):
    r = (e * ud) * RAD_PER_DEG
    if r >= QUARTER_TURN:
        return math.inf
    if r <= -QUARTER_TURN:
        return -math.inf
    return math.tan(r)


def rule(w, mut=()):
    """smhv_weapon_thresholds -> dict(v, g, v2, v4, t_min, t_max, band [7], t_disp, range_min, unit_deg, arc)."""
    ud = unit_deg(w.unit, mut)
    band = [tanlim(w.elev_min + ((w.elev_max - w.elev_min) * float(j + 1)) / 8.0, ud) for j in range(7)]
    return dict(v=w.velocity, g=w.gravity, v2=math.pow(w.velocity, 2.0), v4=math.pow(w.velocity, 4.0), t_min=tanlim(w.elev_min, ud),
                t_max=tanlim(w.elev_max, ud), band=band, t_disp=math.tan(w.dispersion), range_min=w.range_min, unit_deg=ud,
                arc=(1 - w.arc) if "swap_arcs" in mut else w.arc)


def roots(k, m, alt):
    """-> (disc, gm, T_hi, T_lo) of arrays m, alt."""
    m, alt = np.asarray(m, F64), np.asarray(alt, F64)
    with np.errstate(all="ignore"):
        disc = k["v4"] - k["g"] * (k["g"] * (m * m) + 2.0 * alt * k["v2"])
        s = np.sqrt(disc)
        gm = k["g"] * m
        return disc, gm, (k["v2"] + s) / gm, (k["v2"] - s) / gm


def status(k, disc, m, T, mut=()):
    with np.errstate(all="ignore"):
        oor = ~(disc >= 0.0)
        below = (m < k["range_min"]) & ("no_min_range" not in mut)
        if "limit_gt" in mut:
            low, high = ~(T > k["t_min"]), ~(k["t_max"] > T)
        else:
            low, high = ~(T >= k["t_min"]), ~(k["t_max"] >= T)
        st = np.where(below, BELOW_MIN_RANGE, 0) | np.where(oor, OUT_OF_RANGE, 0)
        return (st | np.where(~oor & low, ELEV_LOW, 0) | np.where(~oor & high, ELEV_HIGH, 0)).astype(np.uint32)


def band(k, T):
    with np.errstate(all="ignore"):
        return sum((T >= b).astype(np.uint32) for b in k["band"])


def tof(k, m, T):
    with np.errstate(all="ignore"):
        return (m * np.sqrt(1.0 + T * T)) / k["v"]


def arc(k, m, gm, disc, T, T_other, mut=()):
    """One smhv_ballistic_arc of arrays -> dict of arrays."""
    m = np.asarray(m, F64)
    with np.errstate(all="ignore"):
        tt = T * T
        elev = (np.vectorize(math.atan, otypes=[F64])(T) * DEG_PER_RAD) / k["unit_deg"]
        apex = (k["v2"] * tt) / ((1.0 + tt) * (2.0 * k["g"]))
        if "apex_no_clamp" not in mut:
            apex = np.where(T <= 0.0, 0.0, apex)
        fall = (gm * (1.0 + tt)) / k["v2"] - T
        along = np.abs(((m * (1.0 - (gm * T) / k["v2"])) * (1.0 + tt)) / fall) * k["t_disp"]
        return dict(elevation=elev, tof=tof(k, m, T_other if "tof_other_root" in mut else T), apex=apex, fall=fall, along=along,
                    status=status(k, disc, m, T, mut), band=band(k, T))


def solve(w, m, alt, mut=()):
    """smhv_ballistic_solve of arrays (or scalars) -> dict(meters, alt_delta, cross, arc=[high, low]); arc[i] as arc() gives it."""
    k = rule(w, mut)
    m, alt = np.asarray(m, F64), np.asarray(alt, F64)
    disc, gm, t_hi, t_lo = roots(k, m, alt)
    if "swap_arcs" in mut:
        t_hi, t_lo = t_lo, t_hi
    with np.errstate(all="ignore"):
        cross = m * k["t_disp"]
    return dict(meters=m, alt_delta=alt, cross=cross, arc=[arc(k, m, gm, disc, t_hi, t_lo, mut), arc(k, m, gm, disc, t_lo, t_hi, mut)])


def line(w, ln, minimap=None, mpx=None, hm=None, fit_to_minimap=True, viewport=None, mut=()):
    """smhv_ballistic_lines of one line -> [dir 0, dir 1], each None (source NONE: a record of zeros) or solve()'s dict + source."""
    meters = FR.record_meters(ln, mpx) if mpx is not None else None
    f = FR.firing_line(ln, minimap, meters, hm, fit_to_minimap, viewport)
    if f["source"] == NONE:
        return [None, None]
    out = []
    for a in (f["alt_delta"], -f["alt_delta"]):
        d = solve(w, f["meters"], a, mut)
        d["source"] = f["source"]
        out.append(d)
    return out


def classes_of(k, src, m, alt, mut=()):
    """The class byte without the isochrone bit, the f64 time of flight and T of arrays of pixels."""
    disc, gm, t_hi, t_lo = roots(k, m, alt)
    T, other = (t_hi, t_lo) if k["arc"] == HIGH else (t_lo, t_hi)
    st = status(k, disc, m, T, mut)
    cls = np.where(st & OUT_OF_RANGE, C_OUT_OF_RANGE, np.where(st & BELOW_MIN_RANGE, C_BELOW_MIN_RANGE, np.where(
        st & ELEV_LOW, C_ELEV_LOW, np.where(st & ELEV_HIGH, C_ELEV_HIGH, C_BAND0 + band(k, T))))).astype(np.uint8)
    cls[src == NONE] = 0
    t = tof(k, m, other if "tof_other_root" in mut else T)
    return cls, t, T


def ballistic_map(w, origin, window, viewport=None, minimap=None, mpx=None, hm=None, fit_to_minimap=True, iso_s=0.0, mut=()):
    """origin, window, viewport, minimap, mpx, hm, fit_to_minimap as reach_ref.reach takes them
    -> dict(classes uint8 [out_h, out_w], tof float32 [out_h, out_w], tof64, T, source, meters, alt, valid, origin)."""
    ow, oh = window
    g = R.reach(origin, (ow + 1, oh + 1), viewport, minimap, mpx, hm, fit_to_minimap)   # (the +1 row and column: the isochrone rule's neighbours)
    if not g["valid"]:
        nan = np.full((oh, ow), np.nan)
        return dict(classes=np.zeros((oh, ow), np.uint8), tof=nan.astype(np.float32), tof64=nan, T=nan, source=np.zeros((oh, ow), np.uint8),
                    meters=np.zeros((oh, ow)), alt=np.zeros((oh, ow)), valid=0, origin=(0.0, 0.0))
    k = rule(w, mut)
    src, m, alt = g["source"], g["meters"], g["alt"]
    cls, t, T = classes_of(k, src, m, alt, mut)
    t = np.where(cls == 0, np.nan, t)
    if iso_s > 0.0:
        with np.errstate(all="ignore"):
            b = np.floor(t / F64(iso_s))
        own_s, own_b = src[:-1, :-1], b[:-1, :-1]
        if "iso_left" in mut:
            side_s = np.concatenate([np.full((oh, 1), 255, np.uint8), src[:-1, :-2]], axis=1)
            side_b = np.concatenate([np.full((oh, 1), np.nan), b[:-1, :-2]], axis=1)
        else:
            side_s, side_b = src[:-1, 1:], b[:-1, 1:]
        edge = ((side_s == own_s) & ~np.isnan(side_b) & (side_b != own_b)) | ((src[1:, :-1] == own_s) & ~np.isnan(b[1:, :-1]) & (b[1:, :-1] != own_b))
        cls[:-1, :-1] |= np.where(edge & ~np.isnan(own_b) & (cls[:-1, :-1] != 0), C_ISO, 0).astype(np.uint8)
    cut = lambda a: np.ascontiguousarray(a[:-1, :-1])
    with np.errstate(all="ignore"):
        t32 = cut(t).astype(np.float32)
    return dict(classes=cut(cls), tof=t32, tof64=cut(t), T=cut(T), source=cut(src), meters=cut(m), alt=cut(alt), valid=1, origin=g["origin"])


def summary(r):
    """The smhv_ballistic_map_result of a restated window -> dict(valid, source_mask, origin, count [12], iso, n_tof, tof_min, tof_max)."""
    if not r["valid"]:
        return dict(valid=0, source_mask=0, origin=(0.0, 0.0), count=[0] * 12, iso=0, n_tof=0, tof_min=0.0, tof_max=0.0)
    c7 = r["classes"] & 0x7F
    mask = 0
    if (c7 == 0).any():
        mask |= 1
    for s in (SCALES, HEIGHTMAP):
        if ((c7 != 0) & (r["source"] == s)).any():
            mask |= 1 << s
    timed = (c7 >= C_BAND0) & ~np.isnan(r["tof64"])
    n = int(timed.sum())
    return dict(valid=1, source_mask=mask, origin=r["origin"], count=[int((c7 == c).sum()) for c in range(1, 13)], iso=int(((r["classes"] & C_ISO) != 0).sum()),
                n_tof=n, tof_min=float(r["tof64"][timed].min()) if n else 0.0, tof_max=float(r["tof64"][timed].max()) if n else 0.0)


def paint(img, classes, palette=None):
    """SMHV_BMAP_PAINT over img (uint8 [h, w, 4], changed in place): the class's colour, then the isochrone's; alpha untouched."""
    p = palette or DEFAULT_PALETTE
    c7 = classes & 0x7F
    for c in range(1, 13):
        R._blend(img, c7 == c, p["pal"][c - 1])
    R._blend(img, (classes & C_ISO) != 0, p["iso"])
    return img


def ulps(a, b):
    """The distance of two f64 in units in the last place (NaN to NaN: 0; a NaN to a number, or opposite signs: a huge number)."""
    a, b = float(a), float(b)
    if a != a or b != b:
        return 0 if (a != a and b != b) else 1 << 62
    ia, ib = (np.array([v], F64).view(np.int64)[0] for v in (a, b))
    if (ia < 0) != (ib < 0):
        return 0 if a == b else 1 << 62
    return abs(int(ia) - int(ib))
