"""Video frames out without a device: the restatement of the outbound arithmetic (tests/yuv_out_ref.py) against its own
pixel-by-pixel form, against the float64 converter of the inbound tests (yuv_ref.forward) and through the inbound restatement
and back; the header's table; the tight sizes; and the library's refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_out_cases as oc
import yuv_out_ref as yo
import yuv_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |colour - round trip| per (R, G, B) over all 2^24 flat colours: yuv_out_ref -> yuv_ref.convert with the colour's own chroma
# (what nearest chroma gives a flat image).  Measured with the two restatements on the CPU; every value is reached.
ROUND_TRIP_MAX = {("709", False): (2, 1, 2), ("709", True): (1, 1, 1), ("601", False): (2, 1, 2), ("601", True): (1, 1, 2)}


def test_coefficient_sums_of_every_row():
    for (matrix, full), (yr_, yg, yb, yoff, ur, ug, ub, vr, vg, vb) in yo.TABLE.items():
        assert yr_ + yg + yb == (65536 if full else 56284) == yo.Y_SUM[full] and yoff == (0 if full else 16)
        assert ur + ug + ub == 0 and vr + vg + vb == 0
        assert ub == vr == (32768 if full else 28784)                # 0.5 * 65536 (* 224 / 255, rounded)
        # the real matrices times 65536 (times 219 / 255 or 224 / 255 in limited range), rounded; green takes up the remainder
        kr, kb = yr.K[matrix]
        sy, sc = (1.0, 1.0) if full else (219.0 / 255.0, 224.0 / 255.0)
        assert yr_ == round(kr * 65536 * sy) and yb == round(kb * 65536 * sy) and abs(yg - (1 - kr - kb) * 65536 * sy) <= 1
        assert ur == round(-kr / (2 * (1 - kb)) * 65536 * sc) and vb == round(-kb / (2 * (1 - kr)) * 65536 * sc)
        assert abs(ug - (-(1 - kr - kb) / (2 * (1 - kb)) * 65536 * sc)) <= 1 and abs(vg - (-(1 - kr - kb) / (2 * (1 - kr)) * 65536 * sc)) <= 1
        # int32 suffices: the largest magnitude a sum can reach
        assert max(abs(c) for c in (ur, ug, ub, vr, vg, vb)) * 1020 + 131072 < 2 ** 31


def test_grey_pixels_give_the_grey_formula_and_neutral_chroma():
    levels = np.arange(256)
    for (matrix, full) in yo.ROWS:
        yoff = yo.TABLE[(matrix, full)][3]
        for rgba in (False, True):
            img = np.stack([levels, levels, levels, 255 - levels], axis=-1).astype(np.uint8).reshape(2, 128, 4)
            Y, U, V = yo.convert(img, matrix, full, rgba)
            want = [min(max(((yo.Y_SUM[full] * int(l) + 32768) >> 16) + yoff, 0), 255) for l in levels]
            assert Y.reshape(-1).tolist() == want == yo.grey(levels, matrix, full).tolist()
            assert (U == 128).all() and (V == 128).all()
        assert yo.grey(0, matrix, full) == yoff and yo.grey(255, matrix, full) == (255 if full else 235)
    assert yo.grey(levels, "709", True).tolist() == levels.tolist()   # full range: the level itself


def test_values_derived_by_hand():
    px = lambda b, g, r: np.array([[[b, g, r, 9]]], np.uint8)        # noqa: E731
    # saturated blue, 709 full: Rs = Gs = 0, Bs = 1020: U = ((32768 * 1020 + 131072) >> 18) + 128 = 128 + 128 = 256 -> 255
    Y, U, V = yo.convert(px(255, 0, 0), "709", True)
    assert (32768 * 1020 + 131072) >> 18 == 128 and U[0, 0] == 255
    assert Y[0, 0] == (4732 * 255 + 32768) >> 16 == 18 and V[0, 0] == ((-3005 * 1020 + 131072) >> 18) + 128 == 116
    # the same bytes read as RGBA are saturated red: V clips instead
    Y, U, V = yo.convert(px(255, 0, 0), "709", True, rgba=True)
    assert V[0, 0] == 255 and Y[0, 0] == (13933 * 255 + 32768) >> 16 == 54
    # limited range: black 16, white 235, chroma 128
    for m in ("709", "601"):
        assert [int(a[0, 0]) for a in yo.convert(px(0, 0, 0), m, False)] == [16, 128, 128]
        assert [int(a[0, 0]) for a in yo.convert(px(255, 255, 255), m, False)] == [235, 128, 128]
    # a 3 x 1 image: chroma sample 0 sums pixels 0, 1 twice over (the missing row), sample 1 sums pixel 2 four times
    img = np.array([[[10, 20, 30, 0], [50, 60, 70, 0], [200, 100, 0, 0]]], np.uint8)
    Y, U, V = yo.convert(img, "601", False)
    rs, gs, bs = 2 * (30 + 70), 2 * (20 + 60), 2 * (10 + 50)
    assert U[0, 0] == ((-9714 * rs - 19070 * gs + 28784 * bs + 131072) >> 18) + 128
    assert V[0, 1] == ((28784 * 0 - 24103 * 400 - 4681 * 800 + 131072) >> 18) + 128
    # a negative sum shifts arithmetically (floor): -1 >> 18 = -1
    assert (-1) >> 18 == -1 and int(np.int32(-1) >> 18) == -1


def test_vectorised_restatement_equals_the_pixel_by_pixel_one():
    for case in oc.CASES:
        for (w, h) in [s for s in oc.SHAPES if s[0] * s[1] <= 1100]:
            for k, (matrix, full) in enumerate(yo.ROWS):
                rgba = bool((k + w) & 1)
                a, b = yo.convert(oc.image(case, w, h), matrix, full, rgba), yo.convert_pixel_by_pixel(oc.image(case, w, h), matrix, full, rgba)
                assert all(np.array_equal(p, q) for p, q in zip(a, b)), (case, w, h, matrix, full)


def test_luma_is_within_one_level_of_the_float_matrix_on_all_colours_and_the_round_trip_bound_holds():
    """All 2^24 colours, all four rows.  Y differs from yuv_ref.forward (float64, rounded) by at most 1 level.  A flat colour through
    the outbound restatement and back through the inbound one comes back within ROUND_TRIP_MAX, which is reached."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    g, b = g.reshape(-1), b.reshape(-1)
    for (matrix, full) in yo.ROWS:
        worst, y_worst, y_count = np.zeros(3, int), 0, 0
        for r in range(256):
            R = np.full(g.size, r)
            Y = yo.luma(R, g, b, matrix, full)
            U, V = yo.chroma(4 * R, 4 * g, 4 * b, matrix, full)     # a flat 2 x 2 block: four times the colour
            back = yr.convert(Y, U, V, matrix, full).astype(int)
            worst = np.maximum(worst, [np.abs(back[:, 2] - R).max(), np.abs(back[:, 1] - g).max(), np.abs(back[:, 0] - b).max()])
            img = np.stack([b, g, R, np.full(g.size, 255)], axis=-1).astype(np.uint8).reshape(256, 256, 4)
            d = np.abs(yr.forward(img, matrix, full)[0].astype(int).reshape(-1) - Y.astype(int))
            y_worst, y_count = max(y_worst, int(d.max())), y_count + int((d > 0).sum())
        assert y_worst == 1 and 5000 < y_count < 12000, (matrix, full, y_worst, y_count)
        assert tuple(worst.tolist()) == ROUND_TRIP_MAX[(matrix, full)], (matrix, full, worst)


def test_chroma_is_within_one_level_of_the_float_converter_on_the_case_images():
    for case in oc.CASES:
        for (w, h) in oc.SHAPES:
            for f in range(oc.N_FRAMES):
                for (matrix, full) in yo.ROWS:
                    Y, U, V = oc.expected(case, w, h, f, matrix, full, False)
                    Yf, Uf, Vf = yr.forward(oc.image(case, w, h, f), matrix, full)
                    for got, ref in ((Y, Yf), (U, Uf), (V, Vf)):
                        assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1, (case, w, h, f, matrix, full)
    # the blue columns reach the clip in full range and not in limited range
    assert oc.expected("blue", 64, 8, 0, "709", True, False)[1].max() == 255 and oc.expected("blue", 64, 8, 0, "709", True, True)[2].max() == 255
    assert oc.expected("blue", 64, 8, 0, "709", False, False)[1].max() == 240


def test_pack_and_layouts():
    Y, U, V = oc.expected("random", 5, 7, 0, "709", False, False)
    a, b = yo.pack_tight(Y, U, V, "nv12"), yo.pack_tight(Y, U, V, "i420")
    assert a.size == b.size == yo.tight_bytes(5, 7) == 35 + 2 * 3 * 4
    assert np.array_equal(a[:35], b[:35]) and np.array_equal(a[35::2], b[35:47]) and np.array_equal(a[36::2], b[47:])
    assert all(np.array_equal(p, q) for p, q in zip(yo.unpack_tight(a, 5, 7, "nv12"), (Y, U, V)))
    assert all(np.array_equal(p, q) for p, q in zip(yo.unpack_tight(b, 5, 7, "i420"), (Y, U, V)))
    # the outbound tight layout is the inbound one
    assert np.array_equal(a, yr.pack_tight(Y, U, V, "nv12")) and np.array_equal(b, yr.pack_tight(Y, U, V, "i420"))
    # every variant keeps its planes apart and inside the buffer; everything else is fill
    for layout in ("nv12", "i420"):
        for (w, h) in oc.SHAPES:
            vs = oc.variants(w, h, layout)
            assert len(vs) == oc.N_VARIANTS
            for v in vs:
                frames = [oc.expected("random", w, h, f, "709", False, False) for f in range(v["n"])]
                buf, lay = yo.pack(frames, layout, base=v["base"], tail=16, fill=oc.FILL, **(v["members"] or {}))
                marks = np.zeros(buf.size, np.int32)
                ones = tuple(np.ones_like(p) for p in frames[0])
                for f in range(v["n"]):
                    tmp = np.zeros(buf.size, np.uint8)
                    yo.place(tmp, v["base"] + f * lay["frame_stride"], *ones, layout, lay)
                    marks += tmp
                assert marks.max() == 1 and marks.sum() == v["n"] * yo.tight_bytes(w, h), (layout, w, h, v)
                assert (buf[marks == 0] == oc.FILL).all() and not marks[:v["base"]].any() and not marks[-16:].any()


def test_video_bytes_equals_staging_bytes(built):
    from squad_mortar_helper_amd import _lib, yuv
    lib = _lib.load()
    for (w, h) in oc.SHAPES + [(1920, 1080), (1921, 1081), (32768, 32768)]:
        for layout in ("nv12", "i420"):
            for matrix in ("709", "601"):
                for full in (False, True):
                    word = yuv.pixels(layout, matrix, full)
                    assert yuv.video_bytes(w, h, word) == yo.tight_bytes(w, h) == lib.smhv_ingest_staging_bytes(w, h, word) == yuv.staging_bytes(w, h, layout)
    assert yuv.video_bytes(1920, 1080, yuv.pixels("nv12")) == 3110400


def test_refusals_that_need_no_device(built):
    from squad_mortar_helper_amd import _lib, yuv
    lib = _lib.load()
    # not an output word: the chroma bit, unknown bits, the other layouts, word 7
    for bad in (5 | 1 << 10, 6 | 1 << 10, 5 | 1 << 11, 6 | 1 << 31, 7, 0, 1, 3, 0 | 1 << 8):
        assert lib.smhv_video_bytes(64, 64, bad) == 0, bad
    assert lib.smhv_video_bytes(0, 64, 5) == 0 and lib.smhv_video_bytes(64, 0, 6) == 0 and lib.smhv_video_bytes(32769, 8, 5) == 0
    with pytest.raises(_lib.VisionError) as ei:
        yuv.video_bytes(8, 8, yuv.pixels("nv12", chroma="bilinear"))
    assert ei.value.code == _lib.E_INVALID
    # the inbound validation stays as it is: the bilinear word is an inbound word, 7 is none
    assert lib.smhv_ingest_staging_bytes(64, 64, 5 | 1 << 10) == 64 * 64 * 3 // 2 and lib.smhv_ingest_staging_bytes(64, 64, 7) == 0
    # null context / batch / pointers: refused before anything touches a device
    one = C.c_void_p(16)
    assert lib.smhv_bgra_to_yuv_device(None, one, 0, 0, 1, 4, 4, 0, 5, one, None, None) == _lib.E_INVALID
    assert lib.smhv_batch_video(None, _lib.VIDEO_RENDER, 0, 1, 5, one, None, None) == _lib.E_INVALID
    assert "null" in lib.smhv_last_error().decode()


def test_header_section_parses_and_matches_the_restatement():
    txt = open(os.path.join(ROOT, "include", "smh_vision_hip.h")).read()
    sec = txt[txt.index("video frames OUT"):]
    rows = re.findall(r"\*\s+(709|601) (limited|full)\s+((?:-?\d+\s+){9}-?\d+)\s*\n", sec)
    assert len(rows) == 4
    for m, rng, nums in rows:
        assert tuple(int(v) for v in nums.split()) == yo.TABLE[(m, rng == "full")], (m, rng)
    for formula in ("Y[y][x]   = clip8(((yr * R + yg * G + yb * B + 32768) >> 16) + yoff)", "U[cy][cx] = clip8(((ur * Rs + ug * Gs + ub * Bs + 131072) >> 18) + 128)",
                    "V[cy][cx] = clip8(((vr * Rs + vg * Gs + vb * Bs + 131072) >> 18) + 128)", "min(2 cx + i, w - 1), min(2 cy + j, h - 1)"):
        assert formula in sec, formula
    consts = dict(re.findall(r"#define (SMHV_VIDEO_\w+) (\d+)u", sec))
    assert consts == {"SMHV_VIDEO_SRC_RGBA": "1", "SMHV_VIDEO_RENDER": "0", "SMHV_VIDEO_UI_MAP": "1"}
    from squad_mortar_helper_amd import _lib
    assert (_lib.VIDEO_SRC_RGBA, _lib.VIDEO_RENDER, _lib.VIDEO_UI_MAP) == (1, 0, 1)
    for name in ("smhv_bgra_to_yuv_device", "smhv_batch_video", "smhv_video_bytes"):
        assert re.search(r"SMHV_API\s+\w+\s+%s\(" % name, sec) and name in _lib.SIGNATURES
