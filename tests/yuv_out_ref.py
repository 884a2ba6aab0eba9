"""The RGBA / BGRA -> 4:2:0 conversion of include/smh_vision_hip.h ("video frames OUT") restated in numpy int32, formula by formula
from the header's text.  Shares no code with the library.

Images are uint8[h, w, 4]; planes come back apart: Y uint8[h, w], U and V uint8[ch, cw] with cw = (w + 1) // 2, ch = (h + 1) // 2.
resolve() fills in a smhv_yuv_layout as the header describes it and place() writes planes into a byte buffer by it, so a test can
build the whole destination buffer it expects, fill bytes included."""
import numpy as np

# (matrix, full_range) -> yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb
TABLE = {
    ("709", False): (11966, 40254, 4064, 16, -6596, -22188, 28784, 28784, -26145, -2639),
    ("709", True): (13933, 46871, 4732, 0, -7509, -25259, 32768, 32768, -29763, -3005),
    ("601", False): (16829, 33039, 6416, 16, -9714, -19070, 28784, 28784, -24103, -4681),
    ("601", True): (19595, 38470, 7471, 0, -11058, -21710, 32768, 32768, -27439, -5329),
}
ROWS = list(TABLE)
Y_SUM = {False: 56284, True: 65536}          # yr + yg + yb by range


def chroma_dims(w, h):
    return (w + 1) // 2, (h + 1) // 2


def tight_bytes(w, h):
    cw, ch = chroma_dims(w, h)
    return w * h + 2 * cw * ch


def _clip8(v):
    return np.minimum(np.maximum(v, 0), 255)


def _rgb(img, rgba):
    a = np.asarray(img).astype(np.int32)
    return (a[..., 0], a[..., 1], a[..., 2]) if rgba else (a[..., 2], a[..., 1], a[..., 0])


def luma(R, G, B, matrix="709", full_range=False):
    """Y of int arrays of one shape."""
    yr, yg, yb, yoff = TABLE[(matrix, bool(full_range))][:4]
    R = np.asarray(R, np.int32); G = np.asarray(G, np.int32); B = np.asarray(B, np.int32)
    return _clip8(((yr * R + yg * G + yb * B + 32768) >> 16) + yoff).astype(np.uint8)


def chroma(Rs, Gs, Bs, matrix="709", full_range=False):
    """(U, V) of the four-pixel sums."""
    _, _, _, _, ur, ug, ub, vr, vg, vb = TABLE[(matrix, bool(full_range))]
    Rs = np.asarray(Rs, np.int32); Gs = np.asarray(Gs, np.int32); Bs = np.asarray(Bs, np.int32)
    U = _clip8(((ur * Rs + ug * Gs + ub * Bs + 131072) >> 18) + 128)
    V = _clip8(((vr * Rs + vg * Gs + vb * Bs + 131072) >> 18) + 128)
    return U.astype(np.uint8), V.astype(np.uint8)


def grey(l, matrix="709", full_range=False):
    """Y of grey levels by the header's grey formula (U = V = 128 goes without saying)."""
    yoff = TABLE[(matrix, bool(full_range))][3]
    return _clip8(((Y_SUM[bool(full_range)] * np.asarray(l, np.int32) + 32768) >> 16) + yoff).astype(np.uint8)


def convert(img, matrix="709", full_range=False, rgba=False):
    """One image uint8[h, w, 4] -> (Y, U, V)."""
    R, G, B = _rgb(img, rgba)
    h, w = R.shape
    cw, ch = chroma_dims(w, h)
    Y = luma(R, G, B, matrix, full_range)
    ys = np.minimum(np.arange(2 * ch), h - 1)                      # min(2 cy + j, h - 1): an edge pixel counts twice
    xs = np.minimum(np.arange(2 * cw), w - 1)

    def box(p):
        return p[ys][:, xs].reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    U, V = chroma(box(R), box(G), box(B), matrix, full_range)
    return Y, U, V


def convert_pixel_by_pixel(img, matrix="709", full_range=False, rgba=False):
    """The same in plain Python integers, one sample at a time (Python's >> is the arithmetic shift): the check on the vectorised form."""
    yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb = TABLE[(matrix, bool(full_range))]
    h, w = img.shape[:2]
    cw, ch = chroma_dims(w, h)
    ri, bi = (0, 2) if rgba else (2, 0)
    clip8 = lambda v: 0 if v < 0 else 255 if v > 255 else v            # noqa: E731
    Y = np.zeros((h, w), np.uint8); U = np.zeros((ch, cw), np.uint8); V = np.zeros((ch, cw), np.uint8)
    for y in range(h):
        for x in range(w):
            r, g, b = int(img[y, x, ri]), int(img[y, x, 1]), int(img[y, x, bi])
            Y[y, x] = clip8(((yr * r + yg * g + yb * b + 32768) >> 16) + yoff)
    for cy in range(ch):
        for cx in range(cw):
            rs = gs = bs = 0
            for j in (0, 1):
                for i in (0, 1):
                    p = img[min(2 * cy + j, h - 1), min(2 * cx + i, w - 1)]
                    rs += int(p[ri]); gs += int(p[1]); bs += int(p[bi])
            U[cy, cx] = clip8(((ur * rs + ug * gs + ub * bs + 131072) >> 18) + 128)
            V[cy, cx] = clip8(((vr * rs + vg * gs + vb * bs + 131072) >> 18) + 128)
    return Y, U, V


def resolve(w, h, layout, n=1, y_pitch=0, uv_pitch=0, u_offset=0, v_offset=0, frame_stride=0):
    """smhv_yuv_layout with its zero members filled in as the header says -> dict (NV12: v_offset = u_offset + 1, where its V bytes lie)."""
    cw, ch = chroma_dims(w, h)
    row = 2 * cw if layout == "nv12" else cw
    yp, up = y_pitch or w, uv_pitch or row
    assert yp >= w and up >= row
    uo = u_offset or yp * h
    if layout == "nv12":
        assert v_offset in (0, uo + 1)
        vo = uo + 1
        end = max(yp * (h - 1) + w, uo + up * (ch - 1) + row)
    else:
        vo = v_offset or uo + up * ch
        end = max(yp * (h - 1) + w, uo + up * (ch - 1) + row, vo + up * (ch - 1) + row)
    fs = frame_stride or end
    assert n == 1 or fs >= end
    return dict(y_pitch=yp, uv_pitch=up, u_offset=uo, v_offset=vo, frame_stride=fs, frame_end=end, total=fs * (n - 1) + end)


def place(buf, base, Y, U, V, layout, lay):
    """Write one frame's planes into uint8 buf at byte offset base by the resolved layout `lay`; every other byte stays."""
    h, w = Y.shape
    ch, cw = U.shape
    for r in range(h):
        o = base + r * lay["y_pitch"]
        buf[o:o + w] = Y[r]
    for r in range(ch):
        ou, ov = base + lay["u_offset"] + r * lay["uv_pitch"], base + lay["v_offset"] + r * lay["uv_pitch"]
        if layout == "nv12":
            buf[ou:ou + 2 * cw:2] = U[r]
            buf[ov:ov + 2 * cw:2] = V[r]
        else:
            buf[ou:ou + cw] = U[r]
            buf[ov:ov + cw] = V[r]


def pack(frames, layout, base=0, tail=0, fill=0xA5, **members):
    """[(Y, U, V)] of one size -> (uint8 buffer of base + the frames by the layout + tail bytes, everything else `fill`; the resolved layout)."""
    h, w = frames[0][0].shape
    lay = resolve(w, h, layout, n=len(frames), **members)
    buf = np.full(base + lay["total"] + tail, fill, np.uint8)
    for f, (Y, U, V) in enumerate(frames):
        place(buf, base + f * lay["frame_stride"], Y, U, V, layout, lay)
    return buf, lay


def pack_tight(Y, U, V, layout):
    buf, _ = pack([(Y, U, V)], layout)
    assert buf.size == tight_bytes(Y.shape[1], Y.shape[0])
    return buf


def unpack_tight(buf, w, h, layout):
    """A tight frame's bytes -> (Y, U, V)."""
    cw, ch = chroma_dims(w, h)
    buf = np.asarray(buf, np.uint8).reshape(-1)
    Y = buf[:w * h].reshape(h, w)
    c = buf[w * h:w * h + 2 * cw * ch]
    if layout == "nv12":
        return Y, c[0::2].reshape(ch, cw), c[1::2].reshape(ch, cw)
    return Y, c[:cw * ch].reshape(ch, cw), c[cw * ch:].reshape(ch, cw)
