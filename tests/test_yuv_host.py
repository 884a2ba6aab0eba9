"""The 4:2:0 video layouts without a device: the restatement (tests/yuv_ref.py) against values derived by hand and against the
real matrices, the tight-layout sizes, the inputs of the end-to-end GPU test, and the library's refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import yuv_cases as yc
import yuv_ref as yr


def _px(y, u, v, matrix, full):
    return yr.convert(np.array([y]), np.array([u]), np.array([v]), matrix, full)[0].tolist()


def test_restatement_on_values_derived_by_hand():
    for matrix in ("709", "601"):
        # limited range: 16 is black, 235 is white: 298 * 219 + 128 = 65390 >> 8 = 255
        assert _px(16, 128, 128, matrix, False) == [0, 0, 0, 255]
        assert _px(235, 128, 128, matrix, False) == [255, 255, 255, 255]
        # below black and above white clip
        assert _px(0, 128, 128, matrix, False) == [0, 0, 0, 255] and _px(255, 128, 128, matrix, False) == [255, 255, 255, 255]
        # full range: grey k -> k for every k ((256 k + 128) >> 8 = k)
        k = np.arange(256)
        out = yr.convert(k, np.full(256, 128), np.full(256, 128), matrix, True)
        assert np.array_equal(out[:, :3], np.stack([k, k, k], axis=-1)) and (out[:, 3] == 255).all()
    # one coloured pixel by hand, 709 limited: Y 100, U 90, V 200: c = 298 * 84 = 25032, d = -38, e = 72
    #   R = (25032 + 459 * 72 + 128) >> 8 = 58208 >> 8 = 227;  G = (25032 + 55 * 38 - 136 * 72 + 128) >> 8 = 17458 >> 8 = 68
    #   B = (25032 - 541 * 38 + 128) >> 8 = 4602 >> 8 = 17
    assert _px(100, 90, 200, "709", False) == [17, 68, 227, 255]
    # a negative sum shifts arithmetically (floor), then clips: 601 full, Y 0, U 0: B = (-454 * 128 + 128) >> 8 = -227 -> 0
    assert _px(0, 0, 128, "601", True)[0] == 0
    # bytes are B, G, R, A: V alone raises R
    assert _px(128, 128, 255, "709", True)[2] == 255 and _px(128, 128, 255, "709", True)[0] == 128


def test_bilinear_weights_on_an_impulse():
    """One chroma sample of 128 + 16 among 128s, 8 x 8 pixels: the sample (1, 1) covers pixels (2..3, 2..3); its weight is 9/16 there,
    3/16 on the four edge neighbours that look at it and 1/16 on the diagonal ones, nothing elsewhere."""
    P = np.full((4, 4), 128, np.uint8)
    P[1, 1] = 144
    up = yr.upsample(P, 8, 8, "bilinear") - 128
    want = np.zeros((8, 8), np.int32)
    want[2:4, 2:4] = 9                       # (9 * 16 + 8) >> 4
    want[1, 2:4] = 3; want[4, 2:4] = 3; want[2:4, 1] = 3; want[2:4, 4] = 3      # (3 * 16 + 8) >> 4
    want[1, 1] = want[1, 4] = want[4, 1] = want[4, 4] = 1                       # (16 + 8) >> 4
    assert np.array_equal(up, want)
    assert np.array_equal(yr.upsample(P, 8, 8, "nearest") - 128, np.kron((P.astype(np.int32) - 128), np.ones((2, 2), np.int32)))
    # the clamps: a corner sample keeps its full weight in the corner pixel ((9 + 3 + 3 + 1) / 16)
    Q = np.full((2, 2), 128, np.uint8)
    Q[0, 0] = 144
    assert (yr.upsample(Q, 3, 3, "bilinear") - 128).tolist() == [[16, 12, 4], [12, 9, 3], [4, 3, 1]]


def test_vectorised_restatement_equals_the_pixel_by_pixel_one():
    for case in yc.CASES:
        for (w, h) in [s for s in yc.SHAPES if s[0] * s[1] <= 400]:
            Y, U, V = yc.planes(case, w, h, 1)
            for (matrix, full) in yr.ROWS:
                for chroma in ("nearest", "bilinear"):
                    assert np.array_equal(yr.to_bgra(Y, U, V, matrix, full, chroma), yr.to_bgra_pixel_by_pixel(Y, U, V, matrix, full, chroma)), (case, w, h)


def test_integer_table_is_within_one_level_of_the_real_matrices_over_the_whole_cube():
    """All 2^24 (Y, U, V) triples, all four rows: the integer result differs from the rounded float64 matrix by at most 1 level, and
    1 is reached."""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    for (matrix, full) in yr.ROWS:
        worst = 0
        for y0 in range(0, 256, 32):
            yy = np.repeat(np.arange(y0, y0 + 32), u.size)
            uu, vv = np.tile(u, 32), np.tile(v, 32)
            got = yr.convert(yy, uu, vv, matrix, full).astype(np.int32)
            r, g, b = yr.float_rgb(yy, uu, vv, matrix, full)
            worst = max(worst, int(np.abs(got[:, 2] - r).max()), int(np.abs(got[:, 1] - g).max()), int(np.abs(got[:, 0] - b).max()))
        assert worst == 1, (matrix, full, worst)


def test_the_clip_case_clips_every_channel_on_both_sides_in_all_four_rows():
    Y, U, V = [np.concatenate([yc.planes("clip", 1366, 8, f)[i].reshape(-1) for f in range(yc.N_FRAMES)]) for i in range(3)]
    assert set(np.unique(yc.planes("clip", 1366, 8, 0)[0])) == set(range(256))
    h, w = 8, 1366
    for (matrix, full) in yr.ROWS:
        cy, yoff, rv, gu, gv, bu = yr.TABLE[(matrix, full)]
        for f in range(yc.N_FRAMES):
            Yp, Up, Vp = yc.planes("clip", w, h, f)
            c = cy * (Yp.astype(np.int32) - yoff)
            d, e = yr.upsample(Up, w, h) - 128, yr.upsample(Vp, w, h) - 128
            raw = [(c + rv * e + 128) >> 8, (c - gu * d - gv * e + 128) >> 8, (c + bu * d + 128) >> 8]
            if f == 0:
                lo, hi = [r.min() for r in raw], [r.max() for r in raw]
            else:
                lo, hi = [min(a, r.min()) for a, r in zip(lo, raw)], [max(a, r.max()) for a, r in zip(hi, raw)]
        assert all(v < 0 for v in lo) and all(v > 255 for v in hi), (matrix, full, lo, hi)
    # nearest and bilinear differ on the chequer and the impulses, in every neighbour direction
    for case in ("chequer", "impulse", "edge"):
        Yc, Uc, Vc = yc.planes(case, 65, 3, 0)
        diff = (yr.upsample(Uc, 65, 3, "nearest") != yr.upsample(Uc, 65, 3, "bilinear")) | (yr.upsample(Vc, 65, 3, "nearest") != yr.upsample(Vc, 65, 3, "bilinear"))
        assert {(int(y) & 1, int(x) & 1) for y, x in zip(*np.nonzero(diff))} == {(0, 0), (0, 1), (1, 0), (1, 1)}, case


def test_tight_layout_sizes_and_staging_bytes(built):
    from squad_mortar_helper_amd import yuv
    for (w, h) in yc.SHAPES + [(1920, 1080), (1921, 1081)]:
        cw, ch = (w + 1) // 2, (h + 1) // 2
        want = w * h + 2 * cw * ch
        assert yr.tight_bytes(w, h) == want <= 4 * w * h
        for layout in ("nv12", "i420"):
            assert yuv.staging_bytes(w, h, layout) == want
            assert yr.pack_tight(*yc.planes("random", w, h), layout).size == want
        assert yuv.staging_bytes(w, h, "bgra") == 4 * w * h and yuv.staging_bytes(w, h, "rgb") == 3 * w * h and yuv.staging_bytes(w, h, "l") == w * h
    assert yuv.staging_bytes(1920, 1080, "nv12") == 3110400
    # NV12 and I420 hold the same samples: the I420 planes are the NV12 pairs de-interleaved
    Y, U, V = yc.planes("random", 5, 7)
    a, b = yr.pack_tight(Y, U, V, "nv12"), yr.pack_tight(Y, U, V, "i420")
    assert np.array_equal(a[:35], b[:35]) and np.array_equal(a[35::2], b[35:47]) and np.array_equal(a[36::2], b[47:])


def test_pixels_word(built):
    from squad_mortar_helper_amd import yuv
    assert yuv.pixels("nv12") == 5 and yuv.pixels("i420") == 6
    assert yuv.pixels("nv12", matrix="601") == 5 | 1 << 8 and yuv.pixels("i420", full_range=True) == 6 | 1 << 9
    assert yuv.pixels("nv12", chroma="bilinear") == 5 | 1 << 10 and yuv.pixels("i420", "601", True, "bilinear") == 6 | 7 << 8
    with pytest.raises(KeyError):
        yuv.pixels("nv21")
    with pytest.raises(KeyError):
        yuv.pixels("nv12", matrix="2020")


def test_refusals_that_need_no_device(built):
    from squad_mortar_helper_amd import _lib, yuv
    lib = _lib.load()
    for bad in (7, 5 | 1 << 11, 6 | 1 << 31, 0 | 1 << 8, 2 | 1 << 10):
        assert lib.smhv_ingest_staging_bytes(64, 64, bad) == 0
    assert lib.smhv_ingest_staging_bytes(0, 64, 5) == 0 and lib.smhv_ingest_staging_bytes(64, 0, 6) == 0
    with pytest.raises(_lib.VisionError) as ei:
        yuv.staging_bytes(0, 4, "nv12")
    assert ei.value.code == _lib.E_INVALID
    # null context / pointers: refused before anything touches a device
    one = C.c_void_p(16)
    assert lib.smhv_yuv_to_bgra_device(None, one, None, 1, 4, 4, 5, one, 0, 0, None) == _lib.E_INVALID
    assert lib.smhv_ingest_commit_pixels(None, 5) == _lib.E_INVALID and lib.smhv_ingest_push_pixels(None, one, 6) == _lib.E_INVALID


def test_end_to_end_inputs_keep_their_marker_lines_through_the_forward_conversion(built):
    """A condition on the inputs of the GPU tests: after synth.make_frame -> forward conversion -> restatement the oracle still finds
    the map open and at least one line, in every seed and colour description the GPU tests use."""
    for seed in yc.VIDEO_SEEDS:
        for (matrix, full, chroma) in (("709", False, "nearest"), ("601", True, "bilinear")):
            ref = yc.video_oracle(seed, matrix, full, chroma)
            assert ref["map_open"] == 1 and len(ref["lines"]) >= 1, (seed, matrix, full, chroma)
    # the forward converter and the restatement are inverses up to rounding and the chroma filter: flat areas come back within 2 levels
    flat = np.zeros((16, 16, 4), np.uint8)
    flat[...] = (40, 120, 200, 255)
    for (matrix, full) in yr.ROWS:
        back = yr.to_bgra(*yr.forward(flat, matrix, full), matrix=matrix, full_range=full)
        assert np.abs(back.astype(int) - flat).max() <= 2, (matrix, full)
