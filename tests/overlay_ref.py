"""A numpy float32 restatement of the heightmap overlay as include/smh_vision_hip.h pins it (src/ui/map.rs:250-256,
src/ui/heightmaps.rs:794-826 at viewport scale 1): every operation one IEEE f32 operation, left to right, unfused.  Shares no code
with the library; the colour map comes from firing_ref.color_map."""
import numpy as np

import firing_ref as R

f32 = np.float32
A = f32(64.0) / f32(255.0)                  # imgui's tint alpha as it stores it: (u8)(0.25f * 255 + 0.5) = 64
B = f32(1.0) - A


def quad(mm, W, H, b00=0, b01=0, fit_to_minimap=True):
    """Steps 1-2 -> (x0, y0, x1, y1, sx, sy) as np.float32."""
    left, right, top, bottom = [int(v) for v in mm]
    offx = offy = f32(0.0)
    with np.errstate(all="ignore"):
        if not fit_to_minimap:
            b00, b01 = f32(b00), f32(b01)
            offx = b00 * (f32((right - left) & 0xFFFFFFFF) / (f32(W) + b00))
            offy = b01 * (f32((bottom - top) & 0xFFFFFFFF) / (f32(H) + b01))
        x0 = f32(left) + offx
        y0 = f32(top) + offy
        sx = f32(right) - x0
        sy = f32(bottom) - y0
        x1 = x0 + sx
        y1 = y0 + sy
    return x0, y0, x1, y1, sx, sy


def covered(n, lo, hi):
    """Step 3 along one axis: pixel indices 0..n-1 whose centre lies in [lo, hi) (NaN compares false)."""
    c = np.arange(n, dtype=np.float32) + f32(0.5)
    with np.errstate(all="ignore"):
        return np.nonzero((lo <= c) & (c < hi))[0]


def taps(idx, lo, size, n):
    """Step 4 along one axis for pixels idx -> (tap a, tap b, f, g): s = ((c - lo) / size) * n - 0.5, i = floor(s)."""
    c = idx.astype(np.float32) + f32(0.5)
    with np.errstate(all="ignore"):
        s = ((c - lo) / size) * f32(n) - f32(0.5)
        i = np.floor(s)
        fr = s - i
        g = f32(1.0) - fr
    ii = i.astype(np.int64)
    return np.clip(ii, 0, n - 1), np.clip(ii + 1, 0, n - 1), fr, g


def overlay(ui, minimap, colors, b00=0, b01=0, fit_to_minimap=True):
    """ui: uint8 [h, w, 4] RGBA; minimap: (left, right, top, bottom) or None; colors: the colour map uint8 [H, W, 4] (opaque);
    b00, b01: bounds[0] of the heightmap -> uint8 [h, w, 4]."""
    out = np.array(ui, np.uint8, copy=True)
    if minimap is None:
        return out
    H, W = colors.shape[:2]
    h, w = out.shape[:2]
    x0, y0, x1, y1, sx, sy = quad(minimap, W, H, b00, b01, fit_to_minimap)
    xs, ys = covered(w, x0, x1), covered(h, y0, y1)
    if len(xs) == 0 or len(ys) == 0:
        return out
    ia, ib, fx, gx = taps(xs, x0, sx, W)
    ja, jb, fy, gy = taps(ys, y0, sy, H)
    C = colors[..., :3].astype(np.float32)
    fx, gx = fx[None, :, None], gx[None, :, None]
    fy, gy = fy[:, None, None], gy[:, None, None]
    top = C[ja][:, ia] * gx + C[ja][:, ib] * fx
    bot = C[jb][:, ia] * gx + C[jb][:, ib] * fx
    c = top * gy + bot * fy
    u = out[np.ix_(ys, xs)][..., :3].astype(np.float32)
    o = c * A + u * B
    px = np.empty((len(ys), len(xs), 4), np.uint8)
    px[..., :3] = np.minimum(o + f32(0.5), f32(255.0)).astype(np.uint8)
    px[..., 3] = 255
    out[np.ix_(ys, xs)] = px
    return out


def overlay_heightmap(ui, minimap, data, bounds, fit_to_minimap=True):
    """The same from the heightmap's texels and bounds ((b00, b01), (b10, b11))."""
    (b00, b01), _ = bounds
    return overlay(ui, minimap, R.color_map(data), b00, b01, fit_to_minimap)
