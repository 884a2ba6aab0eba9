"""Restatement of the firing solutions for the tests (never imported by the product package): src/ui/markers.rs:25-112,131,141,
164,192, src/squadex/milliradians.rs and Heightmap::height (heightmap-ripper/src/lib.rs:22-25) with Rust's f32 / f64
semantics, one line at a time.  f32 arithmetic goes through numpy float32 scalars (IEEE single, unfused), f64 through Python
floats; atan2f is the host libm's (numpy float32 arctan2), atan glibc's (math.atan)."""
import math

import numpy as np

F32 = np.float32
G = 9.8
V = 109.890938
V2 = math.pow(V, 2)              # what LLVM folds VELOCITY.powi(2) / powi(4) to (the host's pow)
V4 = math.pow(V, 4)
PIS_IN_180_F32 = F32(57.2957795130823208767981548141051703)
NONE, SCALES, HEIGHTMAP = 0, 1, 2


def fdiv(a, b):
    """IEEE f64 division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def fsqrt(x):
    return math.sqrt(x) if x >= 0.0 else (x if x != x else float("nan"))


def calc(meters, alt_delta):
    """squadex::milliradians::calc in f64 (NaN = out of range)."""
    p1 = fsqrt(V4 - G * (G * (meters * meters) + 2.0 * alt_delta * V2))
    a1 = math.atan(fdiv(V2 + p1, G * meters))
    return a1 * (180.0 / math.pi) / (360.0 / 6400.0)


def roundf(x):
    """f32::round: half away from zero (not numpy's half to even)."""
    x = F32(x)
    if not np.isfinite(x):
        return x
    t = F32(np.trunc(x))
    if abs(F32(x - t)) >= F32(0.5):
        t = F32(t + F32(math.copysign(1.0, float(x))))
    return t


def round_f64(x):
    if not math.isfinite(x):
        return x
    t = float(np.trunc(x))
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return t


def as_i32(x):
    """Rust `f64 as i32`: saturating, NaN -> 0."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def bearings_from_degrees(d):
    """markers.rs:100-109 from `angle.to_degrees()` -> (fwd, bck) as float32."""
    d = F32(d)
    if d > F32(0.0):
        d = F32(d - F32(90.0))
        if d < F32(0.0):
            d = F32(d + F32(360.0))
    else:
        d = F32(d + F32(270.0))
    fwd = F32(np.fmod(roundf(d), F32(360.0)))
    bck = F32(np.fmod(roundf(F32(fwd + F32(180.0))), F32(360.0)))
    return fwd, bck


def atan2f(y, x):
    return F32(np.arctan2(F32(y), F32(x)))


def bearings(p0x, p0y, p1x, p1y, angle=None):
    """(fwd, bck) of a translated line; angle overrides atan2f (the device's atan2f may differ from the host's by an ulp)."""
    a = atan2f(F32(p0y - p1y), F32(p0x - p1x)) if angle is None else F32(angle)
    return bearings_from_degrees(F32(a * PIS_IN_180_F32))


def height(data, scale_z, x, y):
    return (float(data[y, x]) / 65535.0) * (float(F32(scale_z)) / 0.1953125)


def record_meters(line, mpx):
    """Marker::new's meters (src/ui/mod.rs:131-140) as the record holds them."""
    ax = float(F32(line[0])) - float(F32(line[2]))
    ay = float(F32(line[1])) - float(F32(line[3]))
    return math.sqrt(ax * ax + ay * ay) * mpx


def firing_line(line, minimap=None, meters=None, hm=None, fit_to_minimap=True, viewport=None):
    """One line (x0, y0, x1, y1) in map-ROI coordinates.  minimap = (left, right, top, bottom) or None; meters = the record's
    meters or None (no m/px); hm = (data u16 [h, w], bounds ((b00, b01), (b10, b11)), scale (x, y, z)) or None; viewport =
    (sw, sh, tx, ty) or None.  -> dict(meters, alt_delta, mils (2), bearing (2), source, p (translated end points))."""
    sw, sh, tx, ty = (F32(1.0), F32(1.0), F32(0.0), F32(0.0)) if viewport is None else tuple(F32(v) for v in viewport)
    sw = F32(1.0) if sw == 0 else sw
    sh = F32(1.0) if sh == 0 else sh
    x0, y0, x1, y1 = (F32(v) for v in line)
    p0x, p0y = F32(F32(x0 * sw) + tx), F32(F32(y0 * sh) + ty)
    p1x, p1y = F32(F32(x1 * sw) + tx), F32(F32(y1 * sh) + ty)
    hm_m, alt = None, None
    if minimap is not None and hm is not None:
        data, bounds, scale = hm
        H, W = data.shape
        left, right, top, bottom = (int(v) for v in minimap)
        if fit_to_minimap:
            off0 = off1 = F32(0.0)
        else:
            b0x, b0y = F32(bounds[0][0]), F32(bounds[0][1])
            mmw, mmh = F32((right - left) & 0xFFFFFFFF), F32((bottom - top) & 0xFFFFFFFF)
            with np.errstate(all="ignore"):
                off0 = F32(F32(b0x * F32(mmw / F32(F32(W) + b0x))) * sw)
                off1 = F32(F32(b0y * F32(mmh / F32(F32(H) + b0y))) * sh)
        rl = F32(F32(F32(F32(left) * sw) + tx) + off0)
        rt = F32(F32(F32(F32(top) * sh) + ty) + off1)
        rr = F32(F32(F32(right) * sw) + tx)
        rb = F32(F32(F32(bottom) * sh) + ty)
        rw, rh = float(F32(rr - rl)), float(F32(rb - rt))
        ax0 = fdiv(float(p0x) - float(rl), rw) * W
        ay0 = fdiv(float(p0y) - float(rt), rh) * H
        ax1 = fdiv(float(p1x) - float(rl), rw) * W
        ay1 = fdiv(float(p1y) - float(rt), rh) * H
        dx, dy = ax0 - ax1, ay0 - ay1
        hm_m = fsqrt(dx * dx + dy * dy)
        i0, j0, i1, j1 = (as_i32(round_f64(v)) for v in (ax0, ay0, ax1, ay1))
        if 0 <= i0 < W and 0 <= j0 < H and 0 <= i1 < W and 0 <= j1 < H:
            alt = height(data, scale[2], i1, j1) - height(data, scale[2], i0, j0)
        else:
            hm_m = None
    fwd, bck = bearings(p0x, p0y, p1x, p1y)
    out = dict(bearing=(fwd, bck), p=(p0x, p0y, p1x, p1y))
    if hm_m is not None:
        out.update(meters=hm_m, alt_delta=alt, mils=(calc(hm_m, alt), calc(hm_m, -alt)), source=HEIGHTMAP)
    elif meters is not None:
        out.update(meters=meters, alt_delta=0.0, mils=(calc(meters, 0.0), calc(meters, 0.0)), source=SCALES)
    else:
        out.update(meters=0.0, alt_delta=0.0, mils=(0.0, 0.0), source=NONE)
    return out


def firing_frame(rec, hm=None, fit_to_minimap=True, viewport=None):
    """The firing slab entry of one frame from its record (a results_to_dicts entry) -> list of firing_line dicts."""
    mm = rec["minimap"]
    out = []
    for l in range(rec["n_lines"]):
        met = float(rec["meters"][l]) if rec["mpx"] is not None else None
        out.append(firing_line(tuple(float(v) for v in rec["lines"][l]), mm, met, hm, fit_to_minimap, viewport))
    return out


def color_map(data):
    """color_map_heightmap (src/ui/heightmaps.rs:169-207) in f64 with Rust's f64::max (NaN drops out) -> uint8 [h, w, 4]."""
    d = np.asarray(data, np.uint16)
    mx, mn = int(d.max()), int(d.min())
    with np.errstate(all="ignore"):
        h = (d.astype(np.float64) - float(mn)) / float(mx - mn)
        hm5 = h - 0.5
        r = np.where(np.isnan(hm5), 0.0, np.maximum(hm5, 0.0)) / 0.5
        bb = (1.0 - h) - 0.5
        b = np.where(np.isnan(bb), 0.0, np.maximum(bb, 0.0)) / 0.5
        g = 1.0 - np.where(h > 0.5, r, b)
    out = np.empty(d.shape + (4,), np.uint8)
    out[..., 0] = (r * 255.0).astype(np.uint8)
    out[..., 1] = (g * 255.0).astype(np.uint8)
    out[..., 2] = (b * 255.0).astype(np.uint8)
    out[..., 3] = 255
    transparent = (d == 0) & (mn != 0)
    out[transparent] = 0
    return out
