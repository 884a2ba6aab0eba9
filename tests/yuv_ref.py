"""The 4:2:0 -> BGRA conversion of include/smh_vision_hip.h (SMHV_PIXELS_NV12 / _I420) restated in numpy int32, formula by formula
from the header's text.  Shares no code with the library.  Plus a test-only FORWARD converter (float RGB -> 4:2:0 planes with
box-filtered chroma) that makes video frames out of BGRA ones.

Planes are passed apart: Y uint8[h, w], U and V uint8[ch, cw] with cw = (w + 1) // 2, ch = (h + 1) // 2.  pack() lays them out
as the library takes them (tight, or with pitches and gaps), unpack-free: the tests only ever build sources."""
import numpy as np

# (matrix, full_range) -> cy, yoff, rv, gu, gv, bu
TABLE = {
    ("709", False): (298, 16, 459, 55, 136, 541),
    ("601", False): (298, 16, 409, 100, 208, 516),
    ("709", True): (256, 0, 403, 48, 120, 475),
    ("601", True): (256, 0, 359, 88, 183, 454),
}
ROWS = list(TABLE)
# the real matrices: (Kr, Kb)
K = {"709": (0.2126, 0.0722), "601": (0.299, 0.114)}


def chroma_dims(w, h):
    return (w + 1) // 2, (h + 1) // 2


def tight_bytes(w, h):
    cw, ch = chroma_dims(w, h)
    return w * h + 2 * cw * ch


def _clip8(v):
    return np.minimum(np.maximum(v, 0), 255)


def convert(Y, U, V, matrix="709", full_range=False):
    """int arrays of one shape (U, V already per pixel) -> uint8[..., 4] B, G, R, A."""
    cy, yoff, rv, gu, gv, bu = TABLE[(matrix, bool(full_range))]
    Y = np.asarray(Y, np.int32); U = np.asarray(U, np.int32); V = np.asarray(V, np.int32)
    c = cy * (Y - yoff)
    d = U - 128
    e = V - 128
    r = _clip8((c + rv * e + 128) >> 8)
    g = _clip8((c - gu * d - gv * e + 128) >> 8)
    b = _clip8((c + bu * d + 128) >> 8)
    return np.stack([b, g, r, np.full_like(b, 255)], axis=-1).astype(np.uint8)


def upsample(P, w, h, chroma="nearest"):
    """A chroma plane uint8[ch, cw] -> its per-pixel values int32[h, w]."""
    P = np.asarray(P, np.int32)
    ch, cw = P.shape
    assert (cw, ch) == chroma_dims(w, h)
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    cx, cy_ = x >> 1, y >> 1
    if chroma == "nearest":
        return P[cy_, cx]
    assert chroma == "bilinear"
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    ny = np.clip(cy_ + np.where(y & 1, 1, -1), 0, ch - 1)
    return (9 * P[cy_, cx] + 3 * P[cy_, nx] + 3 * P[ny, cx] + P[ny, nx] + 8) >> 4


def to_bgra(Y, U, V, matrix="709", full_range=False, chroma="nearest"):
    """Planes of one frame -> uint8[h, w, 4]."""
    h, w = Y.shape
    return convert(Y, upsample(U, w, h, chroma), upsample(V, w, h, chroma), matrix, full_range)


def to_bgra_pixel_by_pixel(Y, U, V, matrix="709", full_range=False, chroma="nearest"):
    """The same in plain Python integers, one pixel at a time (Python's >> is the arithmetic shift): the check on the vectorised form."""
    cy, yoff, rv, gu, gv, bu = TABLE[(matrix, bool(full_range))]
    h, w = Y.shape
    cw, ch = chroma_dims(w, h)
    out = np.zeros((h, w, 4), np.uint8)
    clip8 = lambda v: 0 if v < 0 else 255 if v > 255 else v            # noqa: E731
    for y in range(h):
        for x in range(w):
            cx, cy_ = x >> 1, y >> 1
            if chroma == "nearest":
                u, v = int(U[cy_][cx]), int(V[cy_][cx])
            else:
                nx = min(max(cx + (1 if x & 1 else -1), 0), cw - 1)
                ny = min(max(cy_ + (1 if y & 1 else -1), 0), ch - 1)
                u = (9 * int(U[cy_][cx]) + 3 * int(U[cy_][nx]) + 3 * int(U[ny][cx]) + int(U[ny][nx]) + 8) >> 4
                v = (9 * int(V[cy_][cx]) + 3 * int(V[cy_][nx]) + 3 * int(V[ny][cx]) + int(V[ny][nx]) + 8) >> 4
            c, d, e = cy * (int(Y[y][x]) - yoff), u - 128, v - 128
            out[y, x] = (clip8((c + bu * d + 128) >> 8), clip8((c - gu * d - gv * e + 128) >> 8), clip8((c + rv * e + 128) >> 8), 255)
    return out


def float_rgb(Y, U, V, matrix, full_range):
    """The real matrix in float64 -> rounded, clipped (R, G, B) int arrays: what the integer table approximates."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    Y = np.asarray(Y, np.float64); U = np.asarray(U, np.float64); V = np.asarray(V, np.float64)
    if full_range:
        yy, pb, pr = Y / 255.0, (U - 128.0) / 255.0, (V - 128.0) / 255.0
    else:
        yy, pb, pr = (Y - 16.0) / 219.0, (U - 128.0) / 224.0, (V - 128.0) / 224.0
    r = yy + 2.0 * (1.0 - kr) * pr
    b = yy + 2.0 * (1.0 - kb) * pb
    g = (yy - kr * r - kb * b) / kg
    q = lambda v: np.clip(np.floor(v * 255.0 + 0.5), 0, 255).astype(np.int32)   # noqa: E731
    return q(r), q(g), q(b)


def pack(Y, U, V, layout, y_pitch=0, uv_pitch=0, gap=0, fill=0xA5):
    """One frame's planes as the bytes the library reads: (uint8[...], dict of smhv_yuv_layout members without frame_stride).
    Pitches 0 = tight; gap = bytes between the planes.  Padding holds `fill`."""
    h, w = Y.shape
    ch, cw = U.shape
    row = 2 * cw if layout == "nv12" else cw
    yp, up = y_pitch or w, uv_pitch or row
    assert yp >= w and up >= row
    u_off = yp * h + gap
    if layout == "nv12":
        total = u_off + up * (ch - 1) + row
        v_off = 0
    else:
        v_off = u_off + up * ch + gap
        total = v_off + up * (ch - 1) + row
    buf = np.full(total + up, fill, np.uint8)                      # (room for the strided views below; cut to `total`)
    for r in range(h):
        buf[r * yp:r * yp + w] = Y[r]
    for r in range(ch):
        if layout == "nv12":
            buf[u_off + r * up:u_off + r * up + row:2] = U[r]
            buf[u_off + r * up + 1:u_off + r * up + row:2] = V[r]
        else:
            buf[u_off + r * up:u_off + r * up + cw] = U[r]
            buf[v_off + r * up:v_off + r * up + cw] = V[r]
    return buf[:total], dict(y_pitch=yp, uv_pitch=up, u_offset=u_off, v_offset=v_off)


def pack_tight(Y, U, V, layout):
    buf, _ = pack(Y, U, V, layout)
    assert buf.size == tight_bytes(Y.shape[1], Y.shape[0])
    return buf


def forward(bgra, matrix="709", full_range=False):
    """Test-only: a BGRA frame -> (Y, U, V) planes, float64 matrix, chroma box-filtered over its (up to) 2 x 2 pixels."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    f = np.asarray(bgra, np.float64)
    b, g, r = f[..., 0] / 255.0, f[..., 1] / 255.0, f[..., 2] / 255.0
    yy = kr * r + kg * g + kb * b
    pb = (b - yy) / (2.0 * (1.0 - kb))
    pr = (r - yy) / (2.0 * (1.0 - kr))
    h, w = yy.shape
    cw, ch = chroma_dims(w, h)

    def box(p):
        q = np.pad(p, ((0, 2 * ch - h), (0, 2 * cw - w)), mode="edge")
        return q.reshape(ch, 2, cw, 2).mean(axis=(1, 3))
    if full_range:
        Y, U, V = yy * 255.0, box(pb) * 255.0 + 128.0, box(pr) * 255.0 + 128.0
    else:
        Y, U, V = yy * 219.0 + 16.0, box(pb) * 224.0 + 128.0, box(pr) * 224.0 + 128.0
    q8 = lambda v: np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)   # noqa: E731
    return q8(Y), q8(U), q8(V)
