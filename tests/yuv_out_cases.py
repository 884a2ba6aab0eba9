"""Inputs of the video-out tests: images that decide every term of the outbound arithmetic, at the smallest shapes that reach every
branch of the kernel, and the destination layouts the library takes.  Pure numpy; yuv_out_ref restates the conversion."""
import functools

import numpy as np

import yuv_out_ref as yo

# w x h.  A lane takes 2 rows x 8 pixels: one pixel; one chroma sample; less than a row pair; one full block of one row; odd both
# ways; a full block, 7 more pixels and an odd height; two full blocks; two and one pixel; several blocks with both edges odd; a
# whole wave's quarter; 16 full blocks and two pixels; and three more so that w mod 8 takes every value 0 .. 7 (3, 4 and 6 are
# theirs), with h odd and even
SHAPES = [(1, 1), (2, 2), (1, 8), (8, 1), (5, 7), (15, 3), (16, 2), (17, 4), (33, 31), (64, 8), (130, 6), (11, 2), (12, 5), (22, 3)]
assert {w % 8 for w, _ in SHAPES} == set(range(8)) and {h % 2 for _, h in SHAPES} == {0, 1}
CASES = ["random", "blocks", "ramp", "corners", "blue", "alpha"]
N_FRAMES = 3
FILL = 0xCD


@functools.lru_cache(maxsize=None)
def image(case, w, h, frame=0):
    """uint8[h, w, 4] in BGRA byte order (the same bytes read as RGBA are another, equally good image).  frame varies the content."""
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    rng = np.random.default_rng(100000 * w + 100 * h + 7 * frame + CASES.index(case))
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 3] = 255
    if case == "random":
        img[..., :3] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif case == "blocks":
        # flat 2 x 2 blocks: every chroma sample is one colour's
        c = rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8)
        img[..., :3] = np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    elif case == "ramp":
        # grey ramps through all 256 levels: R = G = B
        img[..., :3] = ((x * 3 + y * 37 + 85 * frame) % 256).astype(np.uint8)[..., None]
    elif case == "corners":
        # the eight corners of the colour cube, pixel by pixel and in 2 x 2 blocks by turns
        k = np.where((y // 2) % 2 == 0, x + 3 * y, x // 2 + 5 * (y // 2)) + frame
        img[..., 0] = 255 * (k & 1); img[..., 1] = 255 * ((k >> 1) & 1); img[..., 2] = 255 * ((k >> 2) & 1)
    elif case == "blue":
        # columns of saturated blue (in either byte order: bytes 0 and 2 take turns by column pair) between black and white: U or V
        # reaches 256 in full range and clips
        pair = (x // 2 + frame) % 4
        img[..., 0] = np.where(pair == 0, 255, np.where(pair == 3, 255, 0))
        img[..., 2] = np.where(pair == 1, 255, np.where(pair == 3, 255, 0))
        img[..., 1] = np.where(pair == 3, 255, 0)
    else:
        assert case == "alpha"
        img[...] = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)          # alpha is ignored
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(case, w, h, frame, matrix, full_range, rgba):
    """The restated (Y, U, V) of image(case, w, h, frame): computed once, shared, read-only."""
    out = yo.convert(image(case, w, h, frame), matrix, full_range, rgba)
    for a in out:
        a.setflags(write=False)
    return out


def variants(w, h, layout):
    """Destination layouts and source placements: [dict(n, base, members of smhv_yuv_layout or None for a NULL layout, src_off,
    src_pitch, src_gap)].  base: bytes the destination lies off a 256-byte boundary; src_off: bytes the source lies off a 16-byte
    one (a multiple of 4); src_pitch: bytes beyond 4 w; src_gap: bytes between the images beyond src_pitch * h."""
    cw, ch = yo.chroma_dims(w, h)
    row = 2 * cw if layout == "nv12" else cw
    tight = yo.resolve(w, h, layout)
    p13 = yo.resolve(w, h, layout, y_pitch=w + 13, uv_pitch=row + 13)
    return [
        dict(n=1, base=0, members=None, src_off=0, src_pitch=0, src_gap=0),                                            # tight, everything aligned
        dict(n=1, base=1, members=dict(y_pitch=w + 1, uv_pitch=row + 1), src_off=4, src_pitch=4, src_gap=0),           # pitches of w + 1
        dict(n=1, base=2, members=dict(y_pitch=w + 13, uv_pitch=row + 13, u_offset=p13["u_offset"] + 3), src_off=8, src_pitch=20, src_gap=0),
        dict(n=1, base=3, members=None, src_off=12, src_pitch=0, src_gap=0),                                           # tight at an odd base
        # chroma rows pitched differently from Y / 2, and the V plane (I420) away from the end of U
        dict(n=1, base=0, members=dict(uv_pitch=row + 5, v_offset=0 if layout == "nv12" else w * h + (row + 5) * ch + 7), src_off=0, src_pitch=16, src_gap=0),
        dict(n=3, base=0, members=dict(frame_stride=tight["frame_end"] + 37), src_off=0, src_pitch=0, src_gap=0),      # three frames with a gap between them
        dict(n=3, base=1, members=dict(y_pitch=w + 1, uv_pitch=row + 1, frame_stride=yo.resolve(w, h, layout, y_pitch=w + 1, uv_pitch=row + 1)["frame_end"] + 2),
             src_off=4, src_pitch=8, src_gap=12),
    ]


N_VARIANTS = 7


def source(case, w, h, n, src_pitch, src_gap):
    """n images as the bytes the library reads: (uint8[...], pitch in bytes, stride in bytes); padding holds 0x5A."""
    pitch = 4 * w + src_pitch
    stride = pitch * h + src_gap
    buf = np.full(stride * n, 0x5A, np.uint8)
    for f in range(n):
        img = image(case, w, h, f)
        for r in range(h):
            o = f * stride + r * pitch
            buf[o:o + 4 * w] = img[r].reshape(-1)
    return buf, pitch, stride
