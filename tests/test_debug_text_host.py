"""The debug text and the vision debugger without a GPU: the library's text font against the restatement's own copy and the label
font, the restatement's probe arithmetic (tests/debug_text_ref.py) against the oracle and values derived by hand, the strings and
the window's placement, the argument errors through the ABI, the public structs through a compiled C program, and the declared
minimum of every case (tests/debug_text_cases.py) on the restatement alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import debug_text_cases as DC
import debug_text_ref as R
import label_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RW, RH = 360, 585                                                # the map ROI of tests/minimap_scenes.py's frames (1024 x 768)
CONSTS = R.load_consts()


# ---- the font -------------------------------------------------------------------------------------------------------------------
def test_the_text_font_has_97_glyphs_the_label_fonts_27_among_them_and_refuses_every_other_byte(built):
    from squad_mortar_helper_amd import _lib as L
    lib = L.load()
    want = set(range(0x20, 0x7F)) | {0xB0, 0xB1}
    assert set(R.GLYPHS) == want and len(want) == 97
    rows, rows27 = (C.c_uint8 * 7)(), (C.c_uint8 * 7)()
    seen = {}
    for ch in range(256):
        rc = lib.smhv_text_font(ch, rows)
        if ch not in want:
            assert rc == L.E_INVALID, ch
            continue
        assert rc == 0 and list(rows) == R.GLYPHS[ch] and all(v < 32 for v in rows), (ch, list(rows), R.GLYPHS[ch])
        if ch in LR.GLYPHS:                                        # the 27 shared glyphs: the label font's rows, from the library and from its restatement
            assert lib.smhv_label_font(ch, rows27) == 0 and list(rows27) == list(rows) == LR.GLYPHS[ch], ch
        if ch != 0x20:
            assert bytes(rows) not in seen, (chr(ch), seen[bytes(rows)])
            seen[bytes(rows)] = chr(ch)
    assert set(LR.GLYPHS) <= want
    assert lib.smhv_text_font(ord("A"), None) == L.E_INVALID


def test_the_lightest_glyph_but_the_space_inks_5_font_pixels(built):
    """What the cases' minimum of 5 S^2 per character leans on."""
    ink = {ch: sum(bin(r).count("1") for r in rows) for ch, rows in R.GLYPHS.items()}
    assert ink[0x20] == 0
    assert min(v for ch, v in ink.items() if ch != 0x20) == 5
    assert {chr(ch) for ch, v in ink.items() if v == 5} == set("-/^_`~\\")


# ---- the probe's arithmetic -------------------------------------------------------------------------------------------------------
def _colours():
    rng = np.random.default_rng(77)
    cols = [tuple(int(v) for v in c) for c in rng.integers(0, 256, size=(4000, 3))]
    cols += [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    cols += [c for _, c, _ in DC.threshold_colours(CONSTS)]
    return cols


def test_hsv_is_the_oracles_and_the_nine_bits_tie_to_the_marker_predicate(built):
    from oracle import oracle as o
    for c in _colours():
        h, s, v = R.hsv(*c)
        assert (h, s, v) == o.hsv(*c), c
        bits = R.team_bits(h, s, v, CONSTS)
        some_team = any((bits >> (3 * t)) & 7 == 7 for t in range(3))
        assert some_team == o.is_any_map_marker_color(*c), (c, (h, s, v), bits)


def test_every_threshold_colour_flips_the_bit_it_is_made_for(built):
    th = {k: CONSTS["FIND_MARKER_HSV_%s_TOLERANCE" % k] for k in ("HUE", "SAT", "VIB")}
    seen = set()
    for what, c, (h, s, v) in DC.threshold_colours(CONSTS):
        if what == "black":
            assert R.hsv(*c) == (0, 0, 0) and R.team_bits(0, 0, 0, CONSTS) & 0b010010010 == 0     # mx == 0: s is NaN -> 0, below MIN_SAT
            continue
        team, kind = what.split(" ", 1)
        t = R.TEAMS.index(team)
        mh, ms, mv = CONSTS[team + "_MARKER_COLOR_HSV"]
        bits = (R.team_bits(h, s, v, CONSTS) >> (3 * t)) & 7
        d = int(kind.split()[-1][1:]) if kind[-1].isdigit() and kind.split()[-1][0] in "+-" else None
        if kind.startswith("hue"):
            assert bool(bits & 1) == (d <= th["HUE"]) and abs(mh - h) == d, (what, bits)
        elif kind.startswith("sat"):
            arc_ok = abs(s - (ms - CONSTS["FIND_MARKER_PLAYER_DIR_ARC_SAT"])) <= th["SAT"]
            assert bool(bits & 2) == ((d <= th["SAT"] or arc_ok) and s >= CONSTS["FIND_MARKER_HSV_MIN_SAT"]) and abs(ms - s) == d, (what, bits)
        elif kind.startswith("arc sat"):
            assert bool(bits & 2) == ((d <= th["SAT"] or abs(ms - s) <= th["SAT"]) and s >= CONSTS["FIND_MARKER_HSV_MIN_SAT"]), (what, bits, s)
        elif kind.startswith("value"):
            assert bool(bits & 4) == (d <= th["VIB"]) and abs(mv - v) == d, (what, bits)
        else:                                                      # min sat - 1 / min sat
            assert s in (34, 35) and (s == 35 or not bits & 2), (what, s, bits)
        seen.add((kind.split(" -")[0].split(" +")[0], bool(bits & (1 if "hue" in kind else 4 if "value" in kind else 2))))
    # every window is seen from both sides
    for kind in ("hue", "sat", "arc sat", "value"):
        assert (kind, True) in seen and (kind, False) in seen, kind


def test_mono_brightness_luma_and_the_186_rule_by_hand():
    ui = np.zeros((2, 3, 4), np.uint8)
    ui[0, 0, :3], ui[0, 1, :3], ui[0, 2, :3], ui[1, 0, :3], ui[1, 1, :3] = (10, 20, 40), (255, 255, 255), (0, 0, 0), (200, 100, 50), (90, 255, 60)
    view = ((1.0, 1.0), (0.0, 0.0))
    p = R.probe(ui, True, (0.5, 0.5), *view, CONSTS)
    # |10-20| + |10-40| + |20-40| = 60, counted for (a, b) and (b, a): 120; luma 0.2126*10 + 0.7152*20 + 0.0722*40 = 19.3
    assert (p["valid"], p["px"], p["py"], p["rgb"], p["mono"], p["brightness"], p["luma"]) == (1, 0, 0, (10, 20, 40), 120, 10, 19)
    # h = 60 * ((r - g) / d + 4) = 60 * (4 - 1/3) = 220; s = 100 * 30/40 = 75; v = 100 * 40/255 = 15.68
    assert (p["h"], p["s"], p["v"]) == (220, 75, 15)
    p = R.probe(ui, True, (1.99, 0.0), *view, CONSTS)
    assert (p["rgb"], p["mono"], p["brightness"], p["luma"], p["h"], p["s"], p["v"]) == ((255, 255, 255), 0, 255, 255, 0, 0, 100)
    p = R.probe(ui, True, (2.0, 0.99), *view, CONSTS)
    assert (p["valid"], p["px"], p["rgb"], p["mono"], p["luma"], p["h"], p["s"], p["v"], p["team_bits"]) == (1, 2, (0, 0, 0), 0, 0, 0, 0, 0, 0)
    p = R.probe(ui, True, (0.0, 1.5), *view, CONSTS)
    # (200 - 50) * 2 * 2 = 600: |200-100| + |200-50| + |100-50| = 300, twice
    assert (p["py"], p["mono"], p["brightness"]) == (1, 600, 50)
    # the frame's colour: 0.299 r + 0.587 g + 0.114 b > 186 -> black
    assert R.frame_color((255, 255, 255)) == R.BLACK and R.frame_color((0, 0, 0)) == R.WHITE
    assert R.frame_color((90, 255, 60)) == R.WHITE                 # 26.91 + 149.685 + 6.84 = 183.435
    assert R.frame_color((100, 255, 60)) == R.BLACK                # 29.9 + 149.685 + 6.84 = 186.425
    assert R.frame_color((0, 255, 255)) == R.WHITE and R.frame_color((255, 255, 0)) == R.BLACK    # 178.755; 225.93
    # validity: closed, off the map on each side, negative, NaN (passes: column 0), (FLT_MAX, FLT_MAX)
    zero = dict(R.ZERO_PROBE)
    assert R.probe(ui, False, (0.5, 0.5), *view, CONSTS) == zero
    for pt in ((3.0, 0.5), (0.5, 2.0), (-0.001, 0.5), (0.5, -1e-30), (DC.FLT_MAX, DC.FLT_MAX), (float("inf"), 0.5)):
        assert R.probe(ui, True, pt, *view, CONSTS) == zero, pt
    p = R.probe(ui, True, (float("nan"), 1.2), *view, CONSTS)
    assert (p["valid"], p["px"], p["py"], p["rgb"]) == (1, 0, 1, (200, 100, 50))
    assert R.probe(ui, True, (DC.FLT_MAX, 1.2), *view, CONSTS) == zero                      # px saturates: off the map
    # through a viewport: ix = (mx - tx) / sw
    p = R.probe(ui, True, (7.5 + 2 * 0.375 + 0.1, 3.25 + 1.5), (0.375, 1.5), (7.5, 3.25), CONSTS)
    assert (p["px"], p["py"]) == (2, 1)


# ---- strings and layout -----------------------------------------------------------------------------------------------------------
def _probe_struct(d):
    from squad_mortar_helper_amd import _lib as L
    p = L.Probe()
    p.valid, p.px, p.py, p.luma, p.h, p.s, p.v, p.mono, p.brightness, p.team_bits = (d["valid"], d["px"], d["py"], d["luma"], d["h"], d["s"], d["v"], d["mono"],
                                                                                      d["brightness"], d["team_bits"])
    for k in range(3):
        p.rgb[k] = d["rgb"][k]
    return p


def test_probe_text_against_strings_written_out_by_hand(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    cases = [
        (dict(valid=1, px=1, py=2, rgb=(255, 128, 0), luma=145, h=30, s=100, v=100, mono=1020, brightness=0, team_bits=0x1FF),
         "RGB [255, 128, 0]\nHSV [30, 100, 100]\nLuma8 145\nOCRPixelSimilarity 1020\nOCRBrightness 0\nAlphaMarker [true, true, true]\n"
         "BravoMarker [true, true, true]\nCharlieMarker [true, true, true]"),
        (dict(valid=1, px=0, py=0, rgb=(0, 0, 0), luma=0, h=0, s=0, v=0, mono=0, brightness=0, team_bits=0),
         "RGB [0, 0, 0]\nHSV [0, 0, 0]\nLuma8 0\nOCRPixelSimilarity 0\nOCRBrightness 0\nAlphaMarker [false, false, false]\n"
         "BravoMarker [false, false, false]\nCharlieMarker [false, false, false]"),
        (dict(valid=1, px=7, py=9, rgb=(90, 255, 60), luma=205, h=110, s=76, v=100, mono=780, brightness=60, team_bits=0b100100101),
         "RGB [90, 255, 60]\nHSV [110, 76, 100]\nLuma8 205\nOCRPixelSimilarity 780\nOCRBrightness 60\nAlphaMarker [true, false, true]\n"
         "BravoMarker [false, false, true]\nCharlieMarker [false, false, true]"),
    ]
    for d, want in cases:
        assert smh.probe_text(_probe_struct(d)) == want
        assert R.probe_text(d).decode("latin-1") == want
        assert len(want) + 1 <= 200 and all(c == 0x0A or c in R.GLYPHS for c in want.encode("latin-1"))
    # the longest string there can be fits the device's pool
    longest = dict(valid=1, px=0, py=0, rgb=(255, 255, 255), luma=255, h=65535, s=255, v=255, mono=1020, brightness=255, team_bits=0)
    assert len(R.probe_text(longest)) == 197 and 197 < 200
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = _probe_struct(cases[0][0])
    assert lib.smhv_probe_text(C.byref(p), buf, len(cases[0][1])) == L.E_INVALID       # no room for the NUL
    assert lib.smhv_probe_text(C.byref(p), buf, len(cases[0][1]) + 1) == 0 and buf.value.decode() == cases[0][1]
    assert lib.smhv_probe_text(None, buf, 256) == L.E_INVALID and lib.smhv_probe_text(C.byref(p), None, 256) == L.E_INVALID


def test_rust_debug_str_and_the_two_decimals():
    import squad_mortar_helper_amd as smh
    assert smh.rust_debug_str('say "hi"') == '"say \\"hi\\""'
    assert smh.rust_debug_str("a\\b") == '"a\\\\b"'
    assert smh.rust_debug_str("x\x01y") == '"x\\u{1}y"' and smh.rust_debug_str("\n\t\r\0") == '"\\n\\t\\r\\0"'
    assert smh.rust_debug_str("it's 5\xb0") == '"it\'s 5\xb0"'                       # {:?} of a str leaves the apostrophe alone
    assert smh.rust_debug_str("caf\xe9") is None and smh.rust_debug_str("€") is None
    # {:.2} of the f32: 99.995f is 99.99500274658203 -> 100.00; 0.005f is 0.004999999888241291 -> 0.00
    runs = smh.ocr_text_runs([(1, 2, 30, 40, 99.995, "100m"), (1, 2, 30, 50, 0.005, 'q"'), (0, 0, 1, 1, 50.0, "caf\xe9"), (0, 0, 1, 1, 50.0, "x" * 60)], 180, 292)
    assert [r[4] for r in runs] == [b'100.00%\n"100m"', b'0.00%\n"q\\""']
    assert runs[0][:4] == (181.0, 332.0, (0, 255, 0, 255), smh.TEXT_MAP_COORDS) and runs[1][2] == (255, 0, 0, 255)
    assert smh.scale_text_runs([(100, 5, 6, 50, True), (300, 7, 8, 90, False)], 180, 292) == [(185.0, 298.0, (255, 0, 255, 255), smh.TEXT_MAP_COORDS, b"100m")]
    assert all(R.valid_run(r) for r in runs)


def test_window_placement_on_both_sides_of_each_flip():
    S, Cw = 1, 33
    Wd, Hd = R.window_size(S, Cw)
    assert (Wd, Hd) == (6 * 33 + 16, 8 + 10 + 8 + 72 + 8) == (214, 106)
    assert R.window_size(3, 35) == (6 * 3 * 35 + 16, 34 + 216)
    W, H = 640, 360
    # wp.x + Wd > W flips; == W does not
    assert R.window_pos((W - Wd - 15.0, 10.0), S, Cw, W, H)[:2] == (W - Wd, 25.0)
    assert R.window_pos((W - Wd - 14.75, 10.0), S, Cw, W, H)[:2] == (W - Wd - 14.75 - Wd - 5.0, 10.0 - Hd - 5.0)
    assert R.window_pos((10.0, H - Hd - 15.0), S, Cw, W, H)[:2] == (25.0, H - Hd)
    assert R.window_pos((10.0, H - Hd - 14.5), S, Cw, W, H)[:2] == (10.0 - Wd - 5.0, H - Hd - 14.5 - Hd - 5.0)
    # a NaN never flips and never paints
    wx, wy, _, _ = R.window_pos((float("nan"), 10.0), S, Cw, W, H)
    assert wx != wx and wy == 25.0
    # the pixel frame: no snapping up to a scale of 1, ph in both coordinates of the second corner
    assert R.pixel_frame((10.75, 20.5), (0.75, 0.9)) == (10.75, 20.5, 10.75, 20.5)
    assert R.pixel_frame((10.75, 20.5), (1.5, 1.25)) == (9.75, 19.5, 11.75, 21.5)
    assert R.pixel_frame((10.75, 20.5), (2.5, 3.5)) == (8.0, 15.0, 13.0, 21.0)      # 10.75 - fmod(10.75, 2) = 10; 20.5 - fmod(20.5, 3) = 18
    assert R.pixel_frame((10.75, 20.5), (3.25, 2.0)) == (6.0, 18.0, 11.0, 22.0)     # 9 - 3, 20 - 2, 9 + 2, 20 + 2


def test_the_text_rule_pixel_by_pixel():
    """One character at S = 2: the cell's first row and last column stay empty, a font pixel is 2 x 2."""
    m = R.text_mask(40, 40, (f32(3.0), f32(5.0)), [b"T"], 2)
    want = np.zeros((40, 40), bool)
    for row, bits in enumerate(R.GLYPHS[ord("T")]):
        for col in range(5):
            if (bits >> (4 - col)) & 1:
                want[5 + 2 * (row + 1):5 + 2 * (row + 2), 3 + 2 * col:3 + 2 * col + 2] = True
    assert np.array_equal(m, want) and m.sum() == 4 * 11
    # a second line starts at the run's x, nine font rows down; an anchor at a pixel centre paints that pixel's column
    m = R.text_mask(40, 40, (f32(0.5), f32(0.5)), [b"", b"|"], 1)
    assert m.sum() == 7 and m[10:17, 2].all()
    # an anchor half a pixel further: centres at x + 0.5 < anchor are left of the run
    assert not R.text_mask(40, 40, (f32(0.75), f32(0.5)), [b"|"], 1)[:, 2].any() and R.text_mask(40, 40, (f32(0.75), f32(0.5)), [b"|"], 1)[1:8, 3].all()


# ---- the ABI without a device -----------------------------------------------------------------------------------------------------
def test_argument_errors_through_the_abi(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    good, keep = smh.DebugOptions([smh.text_run(1, 2, "ok\nfine")], probes=[(1, 2)], draw_probes=True, minimap_caption=True, scale=4).struct()
    opt = smh.render_options(smh.MapViewport.identity(RW, RH), 64, 32)
    out = np.zeros((32, 64, 4), np.uint8)

    def call(do):
        return lib.smhv_render_map_debug(None, None, C.byref(opt), None, None, 0, None, C.byref(do) if do is not None else None, out.ctypes.data, None, None)

    def options(runs=None, **kw):
        do, keep = smh.DebugOptions(runs if runs is not None else [smh.text_run(1, 2, "ok")], probes=[(1, 2)]).struct()
        for k, v in kw.items():
            setattr(do, k, v)
        return do, keep
    # the options are checked before the context: a good one gets as far as the null context
    assert call(good) == L.E_INVALID and b"null context" in lib.smhv_last_error()
    bad = [options(size=32), options(size=48), options(flags=4), options(flags=0x80000001), options(scale=5), options(n_runs=65), options(n_probes=17),
           options(runs=[smh.text_run(0, 0, "a", (1, 2, 3, 254))]), options(runs=[smh.text_run(0, 0, "a")] * 65),
           options(runs=[smh.text_run(0, 0, "1\n2\n3\n4\n5\n6\n7\n8\n9")]), options(runs=[smh.text_run(0, 0, "caf\xe9")]), options(runs=[smh.text_run(0, 0, "tab\t")]),
           options(runs=[smh.text_run(0, 0, "a"), (0.0, 0.0, (1, 2, 3, 255), 2, b"flag")])]
    do, keep1 = options()
    do.runs = None
    bad.append((do, keep1))
    do, keep2 = options()
    do.probes = None
    bad.append((do, keep2))
    do, keep3 = options()
    do.runs[0].n = 65
    bad.append((do, keep3))
    for i, (do, _) in enumerate(bad):
        assert call(do) == L.E_INVALID and b"null context" not in lib.smhv_last_error(), (i, lib.smhv_last_error())
    assert call(None) == L.E_INVALID
    assert not out.any()
    # eight lines, 64 bytes and 64 runs are fine
    ok = [options(runs=[smh.text_run(0, 0, "1\n2\n3\n4\n5\n6\n7\n8")]), options(runs=[smh.text_run(0, 0, "x" * 64)]), options(runs=[smh.text_run(0, 0, "a")] * 64),
          options(runs=[]), options(runs=[smh.text_run(0, 0, "\xb0\xb1~ ")])]
    for i, (do, _) in enumerate(ok):
        assert call(do) == L.E_INVALID and b"null context" in lib.smhv_last_error(), i
    # the batch calls without a batch
    pts = (L.ProbePoint * 1)()
    assert lib.smhv_batch_probe(None, 0, 1, C.byref(opt), pts, 1, None) == L.E_INVALID
    assert lib.smhv_batch_render_debug(None, 0, 1, C.byref(opt), C.byref(good), None) == L.E_INVALID
    assert lib.smhv_batch_read_probes(None, 0, 1, (L.Probe * 16)()) == L.E_INVALID
    assert lib.smhv_batch_probes_ptr(None, C.byref(C.c_void_p())) == L.E_INVALID


def test_the_headers_structs_have_the_documented_layout(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    src = tmp_path / "debug_text_abi.c"
    exe = tmp_path / "debug_text_abi"
    fields = ["sizeof(smhv_text_run)", "offsetof(smhv_text_run, rgba)", "offsetof(smhv_text_run, flags)", "offsetof(smhv_text_run, n)", "offsetof(smhv_text_run, text)",
              "sizeof(smhv_probe_point)", "sizeof(smhv_probe)", "offsetof(smhv_probe, rgb)", "offsetof(smhv_probe, luma)", "offsetof(smhv_probe, h)",
              "offsetof(smhv_probe, s)", "offsetof(smhv_probe, mono)", "offsetof(smhv_probe, brightness)", "offsetof(smhv_probe, team_bits)",
              "sizeof(smhv_debug_options)", "offsetof(smhv_debug_options, runs)", "offsetof(smhv_debug_options, n_probes)", "offsetof(smhv_debug_options, probes)",
              "SMHV_TEXT_MAX_RUNS", "SMHV_TEXT_MAX_BYTES", "SMHV_TEXT_MAX_LINES", "SMHV_MAX_PROBES", "SMHV_TEXT_MAP_COORDS", "SMHV_DEBUG_DRAW_PROBES",
              "SMHV_DEBUG_MINIMAP_CAPTION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\nint main(void) {\n'
                   + "".join('\tprintf("%%u\\n", (unsigned)(%s));\n' % f for f in fields) + "\treturn 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [84, 8, 12, 16, 20, 8, 32, 12, 15, 16, 18, 20, 22, 24, 40, 16, 24, 32, 64, 64, 8, 16, 1, 1, 2], got
    assert (got[0], got[5], got[6], got[14]) == (C.sizeof(L.TextRun), C.sizeof(L.ProbePoint), C.sizeof(L.Probe), C.sizeof(L.DebugOptionsStruct))
    assert (L.TEXT_MAX_RUNS, L.TEXT_MAX_BYTES, L.TEXT_MAX_LINES, L.MAX_PROBES, L.TEXT_MAP_COORDS, L.DEBUG_DRAW_PROBES, L.DEBUG_MINIMAP_CAPTION) == tuple(got[18:])
    assert (L.Probe.team_bits.offset, L.Probe.mono.offset, L.DebugOptionsStruct.probes.offset) == (24, 20, 32)
    assert (R.MAX_RUNS, R.MAX_BYTES, R.MAX_LINES, R.MAX_PROBES, R.MAP_COORDS, R.DRAW_PROBES, R.MINIMAP_CAPTION) == tuple(got[18:])


# ---- every case's minimum, on the restatement alone -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """A ui_map and images to draw over that hold none of the colours the provisos name: every channel in 40 .. 199."""
    rng = np.random.default_rng(3)
    ui = rng.integers(40, 200, size=(RH, RW, 4), dtype=np.uint8)
    ui[..., 3] = 255
    return ui, rng


@pytest.mark.parametrize("case", DC.all_cases(RW, RH), ids=lambda c: c.name)
def test_the_restatement_meets_every_declared_minimum(scene, case):
    ui, rng = scene
    ow, oh = case.window
    base = rng.integers(40, 200, size=(oh, ow, 4), dtype=np.uint8)
    base[..., 3] = 255
    assert all(R.valid_run(r) for r in case.runs) and len(case.runs) <= R.MAX_RUNS and len(case.points) <= R.MAX_PROBES
    S = case.S or 2
    item_list, probes = R.items(ui, True, True, case.runs, case.points, case.flags, S, ow, oh, case.view.scale, case.view.top_left, CONSTS)
    minimum = DC.minimum_of(case, base, item_list, probes)
    img = base.copy()
    n = R.draw(img, item_list, S)
    if minimum is None:
        assert n == 0 and np.array_equal(img, base)
    else:
        assert n >= minimum, (case, n, minimum)
    if case.name.startswith("64 runs"):                            # ... and without a rectangle the list is as long as it can be: 129 items
        full, probes = R.items(ui, True, False, case.runs, case.points, case.flags, S, ow, oh, case.view.scale, case.view.top_left, CONSTS)
        assert len(full) == 64 + 1 + 4 * 16 == 129 and all(p["valid"] for p in probes)
        img = base.copy()
        assert R.draw(img, full, S) >= DC.minimum_of(case, base, full, probes)
    # a closed frame gets nothing, whatever the case holds
    closed, zero = R.items(ui, False, False, case.runs, case.points, case.flags | R.MINIMAP_CAPTION, S, ow, oh, case.view.scale, case.view.top_left, CONSTS)
    assert closed == [] and all(p == R.ZERO_PROBE for p in zero)


def test_the_caption_and_the_stack_on_the_restatement(scene):
    ui, rng = scene
    base = rng.integers(40, 200, size=(360, 640, 4), dtype=np.uint8)
    base[..., 3] = 255
    for S in (1, 2, 4):
        img = base.copy()
        n, _ = R.debug_pass(img, ui, True, False, [], [], R.MINIMAP_CAPTION, S, (1.0, 1.0), (0.0, 0.0), CONSTS)
        changed = (img != base).any(axis=2)
        k = DC.ink_of(R.CAPTION)
        # 58 characters of 6 S: at S = 1 and 2 wholly inside (358, 706 > 640 at S = 2: cut) -- count what is inside
        inside = min(k, (640 - 10) // (6 * S) - R.CAPTION[:(640 - 10) // (6 * S)].count(b" "))
        assert n >= 5 * S * S * inside and (img[changed] == np.array((255, 0, 0, 255), np.uint8)).all()
        ys = np.nonzero(changed.any(axis=1))[0]
        assert ys.min() >= 360 - 10 - 9 * S and ys.max() < 360 - 10
        img2 = base.copy()
        assert R.debug_pass(img2, ui, True, True, [], [], R.MINIMAP_CAPTION, S, (1.0, 1.0), (0.0, 0.0), CONSTS)[0] == 0
    case = DC.stack_case(RW, RH)
    img = base[:128, :257].copy()
    R.debug_pass(img, ui, True, True, case.runs, [], 0, 1, case.view.scale, case.view.top_left, CONSTS)
    changed = (img != base[:128, :257]).any(axis=2)
    assert (img[changed] == np.array(case.runs[-1][2], np.uint8)).all()
