"""A numpy float32 restatement of the map view's layers as include/smh_vision_hip.h pins them ("map view: layers"; src/ui/draw.rs:135-198,
src/ui/debug.rs:286-345, src/ui/map.rs:210): every operation one IEEE f32 operation, left to right, unfused.  Steps 0 to 2 and the
stroke of a line are render_ref's, imported and not edited; a debug view that is the map enters as the `ui` argument.

A prim is the tuple (x0, y0, x1, y1, (r, g, b, a), kind) in map-ROI coordinates, kind as the header's SMHV_PRIM_*."""
import numpy as np

import render_ref as RR

f32 = np.float32
LINE, RECT, FOREGROUND, SHIFT1 = 0, 1, 0x100, 0x200
BOUNDS_COLOR = (0, 255, 0, 255)
_ONE = (f32(1.0), f32(1.0))
_ZERO = (f32(0.0), f32(0.0))


def ends(p, scale, top_left, shift1=False):
    """A prim's end points through the viewport -> (P0.x, P0.y, P1.x, P1.y) as np.float32; shift1 adds 1.0f to all four."""
    sw, sh = f32(scale[0]), f32(scale[1])
    tx, ty = f32(top_left[0]), f32(top_left[1])
    with np.errstate(all="ignore"):
        e = [f32(p[0]) * sw + tx, f32(p[1]) * sh + ty, f32(p[2]) * sw + tx, f32(p[3]) * sh + ty]
        if shift1:
            e = [v + f32(1.0) for v in e]
    return tuple(f32(v) for v in e)


def rect_mask(out_w, out_h, e):
    """SMHV_PRIM_RECT for translated corners e -> bool [out_h, out_w]: the outer box without the inner one."""
    with np.errstate(all="ignore"):
        ax, ay = np.fmin(e[0], e[2]), np.fmin(e[1], e[3])         # (a NaN operand yields the other one)
        bx, by = np.fmax(e[0], e[2]), np.fmax(e[1], e[3])
        cx = np.arange(out_w, dtype=np.float32) + f32(0.5)
        cy = np.arange(out_h, dtype=np.float32) + f32(0.5)
        in_x, in_y = (ax <= cx) & (cx < bx), (ay <= cy) & (cy < by)
        inner_x = (f32(ax + f32(1.0)) <= cx) & (cx < f32(bx - f32(1.0)))
        inner_y = (f32(ay + f32(1.0)) <= cy) & (cy < f32(by - f32(1.0)))
    return np.outer(in_y, in_x) & ~np.outer(inner_y, inner_x)


def prim_mask(out_w, out_h, prim, scale, top_left):
    """The pixels a prim paints -> bool [out_h, out_w]."""
    e = ends(prim[:4], scale, top_left, bool(prim[5] & SHIFT1))
    if (prim[5] & 0xFF) == RECT:
        return rect_mask(out_w, out_h, e)
    # the map view's stroke on the translated end points (v * 1.0f + 0.0f is v)
    return RR.line_mask(out_w, out_h, e, _ONE, _ZERO)


def bounds_prim(minimap):
    """SMHV_LAYER_MINIMAP_BOUNDS of a record's rectangle (left, right, top, bottom)."""
    left, right, top, bottom = [int(v) for v in minimap]
    return (f32(left), f32(top), f32(right), f32(bottom), BOUNDS_COLOR, RECT | FOREGROUND | SHIFT1)


def render(ui, map_open, minimap, lines, out_w, out_h, quad, scale=(1.0, 1.0), top_left=(0.0, 0.0), flags=0, prims=(), minimap_bounds=False,
           colors=None, b00=0, b01=0, background=(0, 0, 0, 255)):
    """render_ref.render with the layers: `ui` is step 1's texture (the ui_map or a debug view, at its own size); prims in list
    order -> uint8 [out_h, out_w, 4]."""
    out = RR.render(ui, map_open, minimap, None, out_w, out_h, quad, scale, top_left, flags & ~RR.MARKERS, colors, b00, b01, background)
    if not map_open:
        return out
    scale = tuple(f32(1.0) if f32(v) == 0 else f32(v) for v in scale)

    def paint(p):
        out[prim_mask(out_w, out_h, p, scale, top_left)] = np.array(tuple(p[4][:3]) + (255,), np.uint8)
    for p in prims:
        if not (p[5] & FOREGROUND):
            paint(p)
    if (flags & RR.MARKERS) and lines is not None and len(lines):
        n = len(lines)
        for i, ln in enumerate(lines):
            out[RR.line_mask(out_w, out_h, ln, scale, top_left)] = RR.line_color(i, n)
    for p in prims:
        if p[5] & FOREGROUND:
            paint(p)
    if minimap_bounds and minimap is not None:
        paint(bounds_prim(minimap))
    return out
