"""A numpy float32 restatement of the map view as include/smh_vision_hip.h pins it (src/ui/map.rs:21-77, 209-273,
src/ui/heightmaps.rs:794-826, src/ui/markers.rs:28-30): every operation one IEEE f32 operation, left to right, unfused.  Shares no
code with the library; the overlay's taps and blend constants come from overlay_ref, the colour map from firing_ref, the
heightmap's rectangle through the viewport is restated here on its own."""
import numpy as np

import firing_ref as R
import overlay_ref as O

f32 = np.float32
MAX_ZOOM = f32(4.0)
ZOOM_LEVELS = f32(10.0)
HEIGHTMAP, MARKERS, BOUNDS_OFFSET = 1, 2, 4


def viewport_calc(region_w, region_h, map_w, map_h, zoom=0, zoom_pos=(0.0, 0.0), pan_pos=(0.0, 0.0)):
    """MapViewport::calc -> (quad (left, top, right, bottom), scale (w, h), top_left (x, y)), all np.float32."""
    rw, rh, mw, mh = f32(region_w), f32(region_h), f32(map_w), f32(map_h)
    with np.errstate(all="ignore"):
        map_ar = mw / mh
        win_ar = rw / rh
        if win_ar > map_ar:
            size = [rh * map_ar, rh]
        else:
            inv = mh / mw
            size = [rw, rw * inv]
        tl = [(rw - size[0]) / f32(2.0), (rh - size[1]) / f32(2.0)]
        if zoom != 0:
            amount = min(f32(min(int(zoom), 255)) / ZOOM_LEVELS, f32(1.0)) * MAX_ZOOM
            tl[0] = tl[0] - f32(zoom_pos[0]) * size[0] * amount
            tl[1] = tl[1] - f32(zoom_pos[1]) * size[1] * amount
            tl[0] = tl[0] + f32(pan_pos[0]) * (size[0] / mw)
            tl[1] = tl[1] + f32(pan_pos[1]) * (size[1] / mh)
            amount = amount + f32(1.0)
            size[0] = size[0] * amount
            size[1] = size[1] * amount
        quad = (f32(tl[0]), f32(tl[1]), f32(tl[0] + size[0]), f32(tl[1] + size[1]))
        scale = (f32(size[0] / mw), f32(size[1] / mh))
    return quad, scale, (f32(tl[0]), f32(tl[1]))


def identity(w, h):
    return (f32(0), f32(0), f32(w), f32(h)), (f32(1), f32(1)), (f32(0), f32(0))


def hm_rect(mm, W, H, b00, b01, fit_to_minimap, scale, top_left):
    """The heightmap's rectangle through the viewport -> (left, top, right, bottom) as np.float32."""
    left, right, top, bottom = [int(v) for v in mm]
    sw, sh = f32(scale[0]), f32(scale[1])
    tx, ty = f32(top_left[0]), f32(top_left[1])
    offx = offy = f32(0.0)
    with np.errstate(all="ignore"):
        if not fit_to_minimap:
            b00, b01 = f32(b00), f32(b01)
            offx = b00 * (f32((right - left) & 0xFFFFFFFF) / (f32(W) + b00)) * sw
            offy = b01 * (f32((bottom - top) & 0xFFFFFFFF) / (f32(H) + b01)) * sh
        return (f32(left) * sw + tx) + offx, (f32(top) * sh + ty) + offy, f32(right) * sw + tx, f32(bottom) * sh + ty


def _nearest(n_out, lo, hi, n_src):
    """Step 1 along one axis -> (covered output indices, their source texel indices)."""
    c = np.arange(n_out, dtype=np.float32) + f32(0.5)
    with np.errstate(all="ignore"):
        cov = np.nonzero((lo <= c) & (c < hi))[0]
        cc = c[cov]
        u = ((cc - lo) / (hi - lo)) * f32(n_src)
        idx = np.clip(np.floor(u).astype(np.int64), 0, n_src - 1)
    return cov, idx


def line_color(i, n):
    f = f32(i + 1) / f32(n)
    return np.array([np.uint8((f32(1.0) - f) * f32(255.0) + f32(0.5)), np.uint8(f * f32(255.0) + f32(0.5)), 0, 255], np.uint8)


def line_mask(out_w, out_h, line, scale, top_left):
    """Step 3 for one line (x0, y0, x1, y1) in map-ROI coordinates -> bool [out_h, out_w]: the pixels it paints."""
    sw, sh = f32(scale[0]), f32(scale[1])
    tx, ty = f32(top_left[0]), f32(top_left[1])
    with np.errstate(all="ignore"):
        p0x, p0y = f32(line[0]) * sw + tx, f32(line[1]) * sh + ty
        p1x, p1y = f32(line[2]) * sw + tx, f32(line[3]) * sh + ty
        dx, dy = f32(p1x - p0x), f32(p1y - p0y)
        len2 = f32(dx * dx + dy * dy)
        if not (len2 > 0):
            return np.zeros((out_h, out_w), bool)
        # (evaluated inside the segment's bounding box grown by 3 px when that box is finite and of pixel-scale coordinates -- no
        # centre outside it is within 1.0 of the segment -- and over the whole window otherwise)
        xa, xb, ya, yb = 0, out_w, 0, out_h
        ends = np.array([p0x, p0y, p1x, p1y], np.float64)
        if np.all(np.isfinite(ends)) and np.all(np.abs(ends) < 1e5):
            xa, xb = max(0, int(np.floor(min(p0x, p1x))) - 3), min(out_w, int(np.ceil(max(p0x, p1x))) + 4)
            ya, yb = max(0, int(np.floor(min(p0y, p1y))) - 3), min(out_h, int(np.ceil(max(p0y, p1y))) + 4)
        mask = np.zeros((out_h, out_w), bool)
        if xa >= xb or ya >= yb:
            return mask
        cx = (np.arange(xa, xb, dtype=np.float32) + f32(0.5))[None, :]
        cy = (np.arange(ya, yb, dtype=np.float32) + f32(0.5))[:, None]
        ax, ay = cx - p0x, cy - p0y
        t = ax * dx + ay * dy
        c = ax * dy - ay * dx
        mask[ya:yb, xa:xb] = (f32(0.0) <= t) & (t <= len2) & (c * c <= len2)
        return mask


def render(ui, map_open, minimap, lines, out_w, out_h, quad, scale=(1.0, 1.0), top_left=(0.0, 0.0), flags=0, colors=None, b00=0, b01=0,
           background=(0, 0, 0, 255)):
    """ui: uint8 [h, w, 4]; minimap: (left, right, top, bottom) or None; lines: [n, 4] or None; colors: the heightmap's colour map
    uint8 [H, W, 4] (needed with HEIGHTMAP) -> uint8 [out_h, out_w, 4]."""
    out = np.empty((out_h, out_w, 4), np.uint8)
    out[...] = np.array(background, np.uint8)
    if not map_open:
        return out
    scale = tuple(f32(1.0) if f32(v) == 0 else f32(v) for v in scale)
    h, w = ui.shape[:2]
    ql, qt, qr, qb = [f32(v) for v in quad]
    xs, ix = _nearest(out_w, ql, qr, w)
    ys, iy = _nearest(out_h, qt, qb, h)
    if len(xs) and len(ys):
        px = ui[np.ix_(iy, ix)].copy()
        px[..., 3] = 255
        out[np.ix_(ys, xs)] = px
    if (flags & HEIGHTMAP) and minimap is not None:
        H, W = colors.shape[:2]
        x0, y0, r, b = hm_rect(minimap, W, H, b00, b01, not (flags & BOUNDS_OFFSET), scale, top_left)
        with np.errstate(all="ignore"):
            sx, sy = f32(r - x0), f32(b - y0)
            x1, y1 = f32(x0 + sx), f32(y0 + sy)
        oxs, oys = O.covered(out_w, x0, x1), O.covered(out_h, y0, y1)
        if len(oxs) and len(oys):
            ia, ib, fx, gx = O.taps(oxs, x0, sx, W)
            ja, jb, fy, gy = O.taps(oys, y0, sy, H)
            def tap(j, i):                                        # the taps' colours as f32 (gathered first: the map may be large)
                return colors[np.ix_(j, i)][..., :3].astype(np.float32)
            fx, gx = fx[None, :, None], gx[None, :, None]
            fy, gy = fy[:, None, None], gy[:, None, None]
            top = tap(ja, ia) * gx + tap(ja, ib) * fx
            bot = tap(jb, ia) * gx + tap(jb, ib) * fx
            c = top * gy + bot * fy
            u = out[np.ix_(oys, oxs)][..., :3].astype(np.float32)
            o = c * O.A + u * O.B
            px = np.empty((len(oys), len(oxs), 4), np.uint8)
            px[..., :3] = np.minimum(o + f32(0.5), f32(255.0)).astype(np.uint8)
            px[..., 3] = 255
            out[np.ix_(oys, oxs)] = px
    if (flags & MARKERS) and lines is not None and len(lines):
        n = len(lines)
        for i, ln in enumerate(lines):
            out[line_mask(out_w, out_h, ln, scale, top_left)] = line_color(i, n)
    return out


def render_heightmap(ui, map_open, minimap, lines, out_w, out_h, quad, scale, top_left, flags, data, bounds, background=(0, 0, 0, 255)):
    """The same from the heightmap's texels and bounds ((b00, b01), (b10, b11)); data None: no heightmap."""
    if data is None:
        return render(ui, map_open, minimap, lines, out_w, out_h, quad, scale, top_left, flags & ~HEIGHTMAP, background=background)
    (b00, b01), _ = bounds
    return render(ui, map_open, minimap, lines, out_w, out_h, quad, scale, top_left, flags, R.color_map(data), b00, b01, background)
