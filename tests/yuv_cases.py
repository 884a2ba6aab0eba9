"""Inputs of the 4:2:0 conversion tests: planes that decide every term of the arithmetic, at the smallest shapes that can go wrong,
in every source layout the library takes.  Pure numpy; yuv_ref restates the conversion."""
import functools

import numpy as np

import yuv_ref as yr

# w x h: one pixel; half a lane's block; odd both ways; odd with several row pairs; 16 blocks in one row pair; one pixel more
# and an odd height; 64 blocks and one pixel (a second wave), an odd height; more blocks than a workgroup has lanes, two bands,
# rows whose tight pitch is 2 mod 4 and a chroma row of 683 samples
SHAPES = [(1, 1), (2, 2), (3, 3), (5, 7), (64, 2), (65, 3), (257, 5), (1366, 8)]
CASES = ["clip", "chequer", "impulse", "edge", "random"]
PITCHES = ["tight", "+1", "+3", "256"]
SRC_OFFSETS = [0, 1, 2, 3]
OUT_OFFSETS = [4, 8, 12]                     # bytes off a 16-byte boundary
N_FRAMES = 3

# chroma pairs that push each channel over both ends (with the Y ramp), and the neutral pair
EXTREMES = [(0, 0), (255, 255), (0, 255), (255, 0), (0, 128), (255, 128), (128, 0), (128, 255), (128, 128)]


@functools.lru_cache(maxsize=None)
def planes(case, w, h, frame=0):
    """(Y, U, V) of one frame of the case at w x h.  frame varies the content (phase / seed)."""
    cw, ch = yr.chroma_dims(w, h)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    cx, cy = np.arange(cw)[None, :], np.arange(ch)[:, None]
    if case == "clip":
        # Y runs through 0..255 along a row; the chroma pair holds for 256 pixels and changes with the block, the row and the frame
        Y = (x % 256).astype(np.uint8)
        idx = ((2 * cx) // 256 + cy + 3 * frame) % len(EXTREMES)
        ext = np.array(EXTREMES, np.uint8)
        U, V = ext[idx, 0], ext[idx, 1]
    elif case == "chequer":
        # U: a chequer of single samples; V: of 2 x 2 blocks of samples.  Nearest and bilinear differ at every pixel of an edge.
        Y = (96 + 16 * ((x + y + frame) % 5)).astype(np.uint8)
        U = np.where((cx + cy + frame) & 1, 40, 220).astype(np.uint8)
        V = np.where(((cx >> 1) + (cy >> 1) + frame) & 1, 230, 30).astype(np.uint8)
    elif case == "impulse":
        # single samples 3 apart each way: each one's four neighbours see it from a different direction and nothing else
        Y = np.full((h, w), 128 + frame, np.uint8)
        U = np.full((ch, cw), 128, np.uint8)
        V = np.full((ch, cw), 128, np.uint8)
        U[(cy % 3 == frame % 3) & (cx % 3 == 1)] = 255
        V[(cy % 3 == (frame + 1) % 3) & (cx % 3 == 2)] = 0
    elif case == "edge":
        # impulses in the first and last chroma row and column: the clamps
        Y = np.full((h, w), 150 - frame, np.uint8)
        U = np.full((ch, cw), 128, np.uint8)
        V = np.full((ch, cw), 128, np.uint8)
        U[0, ::2] = 250; U[-1, 1::2] = 5; U[::2, 0] = 250; U[1::2, -1] = 5
        V[0, 1::2] = 10; V[-1, ::2] = 245; V[1::2, 0] = 10; V[::2, -1] = 245
        if frame:
            U, V = V.copy(), U.copy()
    else:
        assert case == "random"
        rng = np.random.default_rng(1000 * w + 10 * h + frame)
        Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        U = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        V = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    Y = np.ascontiguousarray(np.broadcast_to(Y, (h, w)), np.uint8)
    U = np.ascontiguousarray(np.broadcast_to(U, (ch, cw)), np.uint8)
    V = np.ascontiguousarray(np.broadcast_to(V, (ch, cw)), np.uint8)
    for a in (Y, U, V):
        a.setflags(write=False)
    return Y, U, V


@functools.lru_cache(maxsize=None)
def expected(case, w, h, frame, matrix, full_range, chroma):
    """The restated BGRA of planes(case, w, h, frame): computed once, shared, read-only."""
    out = yr.to_bgra(*planes(case, w, h, frame), matrix=matrix, full_range=full_range, chroma=chroma)
    out.setflags(write=False)
    return out


def pitches(kind, w, h, layout):
    """(y_pitch, uv_pitch) of a pitch kind."""
    cw, _ = yr.chroma_dims(w, h)
    row = 2 * cw if layout == "nv12" else cw
    if kind == "tight":
        return w, row
    if kind == "256":
        return (w + 255) // 256 * 256, (row + 255) // 256 * 256
    k = int(kind)
    return w + k, row + k


def source(case, w, h, layout, pitch_kind, n):
    """n frames of the case as one byte array with frames frame_stride apart -> (uint8[...], smhv_yuv_layout members).  n > 1: the
    stride is larger than a frame (and keeps a 256-byte pitch's alignment)."""
    yp, up = pitches(pitch_kind, w, h, layout)
    gap = 0 if pitch_kind == "tight" else (256 if pitch_kind == "256" else 5)
    bufs = []
    for f in range(n):
        b, lay = yr.pack(*planes(case, w, h, f), layout, y_pitch=yp, uv_pitch=up, gap=gap)
        bufs.append(b)
    size = bufs[0].size
    if n == 1:
        return bufs[0], dict(lay, frame_stride=0)
    stride = (size + 255) // 256 * 256 + 256 if pitch_kind == "256" else size + 37
    out = np.full(stride * (n - 1) + size, 0x5A, np.uint8)
    for f, b in enumerate(bufs):
        out[f * stride:f * stride + size] = b
    return out, dict(lay, frame_stride=stride)


# ---- the end-to-end frames: synthetic screenshots with marker lines, as a video decoder would hand them over -------------------
VIDEO_W, VIDEO_H = 1024, 768
VIDEO_SEEDS = (1, 4, 5)                      # chosen on the CPU: the oracle still finds lines after the forward conversion (test_yuv_host)


@functools.lru_cache(maxsize=None)
def video_frame(seed, matrix="709", full_range=False):
    """synth.make_frame(1024 x 768, seed) through the test-only forward converter -> (Y, U, V)."""
    from squad_mortar_helper_amd import synth
    f, _ = synth.make_frame(VIDEO_W, VIDEO_H, seed, n_lines=2)
    Y, U, V = yr.forward(f, matrix, full_range)
    for a in (Y, U, V):
        a.setflags(write=False)
    return Y, U, V


@functools.lru_cache(maxsize=None)
def video_bgra(seed, matrix="709", full_range=False, chroma="nearest"):
    """The restatement's BGRA of video_frame: what the pipeline must see."""
    out = yr.to_bgra(*video_frame(seed, matrix, full_range), matrix=matrix, full_range=full_range, chroma=chroma)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def video_oracle(seed, matrix="709", full_range=False, chroma="nearest"):
    """oracle.process_frame of video_bgra (markers + grey ui_map), computed once."""
    from oracle import oracle as o
    return o.process_frame(video_bgra(seed, matrix, full_range, chroma), grayscale=True, max_gap=15, stages=0x3, want_images=True)
