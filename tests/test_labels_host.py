"""The marker labels without a GPU: the library's font against the restatement's own copy, the restatement's strings and layouts
(tests/label_ref.py) against values derived by hand from the header's rules, the public structs through a compiled C program,
and the declared minimum of every case (tests/label_cases.py) on the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import label_cases as LC
import label_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN = float("nan")
ID = (1.0, 1.0, 0.0, 0.0)
RGBA = (9, 8, 7, 255)
RW, RH = 360, 585                                                # the map ROI of tests/minimap_scenes.py's frames (1024 x 768)
PM, DEG = b"\xb1", b"\xb0"


def _firing(meters=100.0, alt=0.0, mils=(1000.0, 1000.0), bearing=(90.0, 270.0), source=R.SCALES):
    return {"meters": meters, "alt_delta": alt, "mils": mils, "bearing": bearing, "source": source}


def _rows(slot):
    return [r[2] for r in slot["runs"]]


def test_the_librarys_font_is_the_restatements_and_has_no_other_glyph():
    from squad_mortar_helper_amd import _lib as L
    lib = L.load()
    assert len(R.GLYPHS) == 27
    assert set(R.GLYPHS) == set(b"0123456789milatRANGE!<-> ") | {0xB1, 0xB0}
    rows = (C.c_uint8 * 7)()
    for ch in range(256):
        rc = lib.smhv_label_font(ch, rows)
        if ch in R.GLYPHS:
            assert rc == 0 and list(rows) == R.GLYPHS[ch], (ch, list(rows), R.GLYPHS[ch])
            assert all(v < 32 for v in rows)
        else:
            assert rc == L.E_INVALID, ch
    assert lib.smhv_label_font(ord("0"), None) == L.E_INVALID
    assert sum(R.GLYPHS[ord(" ")]) == 0 and all(sum(g) > 0 for c, g in R.GLYPHS.items() if c != ord(" "))


def test_rounding_ties_go_to_even():
    line = (10.0, 20.0, 30.0, 20.0)
    for meters, want in ((12.5, b"12m"), (13.5, b"14m"), (0.5, b"0m"), (1.5, b"2m"), (2.4999, b"2m"), (999.5, b"1000m"), (0.0, b"0m")):
        assert _rows(R.format_label(line, _firing(meters=meters), ID, RGBA))[0] == want, meters
    for mils, want in ((1000.5, b"1000 mil"), (1001.5, b"1002 mil"), (800.49, b"800 mil"), (1579.5, b"1580 mil")):
        assert _rows(R.format_label(line, _firing(mils=(mils, 5.0)), ID, RGBA))[1] == want, mils


def test_range_on_each_side():
    right, left = (30.0, 20.0, 10.0, 20.0), (10.0, 20.0, 30.0, 20.0)      # d = P0 - P1: d.x > 0, d.x < 0
    assert _rows(R.format_label(right, _firing(mils=(NAN, 7.0)), ID, RGBA))[1] == b"RANGE!"
    assert _rows(R.format_label(right, _firing(mils=(7.0, NAN)), ID, RGBA))[1] == b"7 mil"       # SCALES prints mils[0] alone
    hm = dict(source=R.HEIGHTMAP, alt=3.0, bearing=(45.0, 225.0))
    # d.x > 0: a = 0 on the left, b = 1 on the right
    assert _rows(R.format_label(right, _firing(mils=(NAN, 812.0), **hm), ID, RGBA))[2:] == [b"<- RANGE!", b"45" + DEG, b"812 mil ->", b"225" + DEG]
    assert _rows(R.format_label(right, _firing(mils=(811.0, NAN), **hm), ID, RGBA))[2:] == [b"<- 811 mil", b"45" + DEG, b"RANGE! ->", b"225" + DEG]
    # d.x < 0: the sides swap
    assert _rows(R.format_label(left, _firing(mils=(NAN, 812.0), **hm), ID, RGBA))[2:] == [b"<- 812 mil", b"225" + DEG, b"RANGE! ->", b"45" + DEG]
    assert _rows(R.format_label(left, _firing(mils=(NAN, NAN), **hm), ID, RGBA))[2:] == [b"<- RANGE!", b"225" + DEG, b"RANGE! ->", b"45" + DEG]


def test_scales_layout_and_the_centring_quirk():
    right = (30.0, 20.0, 10.0, 20.0)
    # the bearing rows are the widest: "5m" 12, "RANGE!" 36 -> W2 = 36; "-> 270deg" and "<- 123deg" 42 -> W4 = 42
    s = R.format_label(right, _firing(meters=5.0, mils=(NAN, NAN), bearing=(123.0, 270.0)), ID, RGBA)
    assert s["runs"] == [(-6, 0, b"5m"), (-30, 18, b"RANGE!"), (-36, 36, b"-> 270" + DEG), (-36, 54, b"<- 123" + DEG)]
    # the mil row is the widest: W2 = W4 = 48, every row centred on it
    s = R.format_label(right, _firing(meters=250.0, mils=(1600.0, 1.0), bearing=(5.0, 185.0)), ID, RGBA)
    assert s["runs"] == [(-24, 0, b"250m"), (-48, 18, b"1600 mil"), (-42, 36, b"-> 185" + DEG), (-30, 54, b"<- 5" + DEG)]
    # the range row is the widest of the first two ("12345m" 36, "7 mil" 30: W2 = 36), a bearing row the widest of all (W4 = 42)
    s = R.format_label(right, _firing(meters=12345.0, mils=(7.0, 1.0), bearing=(100.0, 280.0)), ID, RGBA)
    assert s["runs"] == [(-30, 0, b"12345m"), (-24, 18, b"7 mil"), (-36, 36, b"-> 280" + DEG), (-36, 54, b"<- 100" + DEG)]


def test_heightmap_layout():
    right = (30.0, 20.0, 10.0, 20.0)
    s = R.format_label(right, _firing(meters=250.0, alt=-12.7, mils=(1234.0, 987.0), bearing=(90.0, 270.0), source=R.HEIGHTMAP), ID, RGBA)
    # left block "<- 1234 mil" 66 / "90deg" 18: Wf = 66; right block "987 mil ->" 60 / "270deg" 24: Wb = 60; -(66 + 60 + 5) = -131
    assert s["runs"] == [(-24, 0, b"250m"), (-48, 18, PM + b"12m alt"), (-131, 36, b"<- 1234 mil"), (-131 + 2 * 48, 54, b"90" + DEG),
                         (-131 + 2 * 71, 36, b"987 mil ->"), (-131 + 2 * 71, 54, b"270" + DEG)]
    assert max(len(r[2]) for r in s["runs"]) <= 16 and len(s["runs"]) == 6


def test_the_altitude_saturates_both_ways():
    right = (30.0, 20.0, 10.0, 20.0)
    for alt, want in ((3e9, b"2147483647"), (-3e9, b"2147483648"), (2147483646.9, b"2147483646"), (-2147483648.0, b"2147483648"), (-12.7, b"12"),
                      (12.999, b"12"), (-0.9, b"0"), (NAN, b"0"), (float("inf"), b"2147483647"), (float("-inf"), b"2147483648")):
        s = R.format_label(right, _firing(alt=alt, source=R.HEIGHTMAP), ID, RGBA)
        assert _rows(s)[1] == PM + want + b"m alt", alt
    assert len(PM + b"2147483648m alt") == 16


def test_every_sign_case_of_d():
    sc = dict(bearing=(10.0, 190.0), mils=(801.0, 802.0))
    hm = dict(source=R.HEIGHTMAP, alt=1.0, **sc)
    cases = {  # line -> (d.x >= 0 for SCALES, a for HEIGHTMAP)
        (30.0, 20.0, 10.0, 25.0): (True, 0),      # d = (20, -5)
        (10.0, 20.0, 30.0, 25.0): (False, 1),     # d = (-20, -5)
        (10.0, 10.0, 10.0, 30.0): (True, 0),      # d = (0, -20): vertical, P1 below
        (10.0, 30.0, 10.0, 10.0): (True, 1),      # d = (0, 20): vertical, P1 above
    }
    for line, (ge, a) in cases.items():
        rows = _rows(R.format_label(line, _firing(**sc), ID, RGBA))
        assert rows[2:] == ([b"-> 190" + DEG, b"<- 10" + DEG] if ge else [b"-> 10" + DEG, b"<- 190" + DEG]), line
        rows = _rows(R.format_label(line, _firing(**hm), ID, RGBA))
        b = 1 - a
        want = [b"<- %d mil" % (801 + a), b"%d" % (10 + 180 * a) + DEG, b"%d mil ->" % (801 + b), b"%d" % (10 + 180 * b) + DEG]
        assert rows[2:] == want, line
    # the placement: along the line, never upside down, s = -1 for a vertical line either way
    s = R.format_label((30.0, 20.0, 10.0, 20.0), _firing(), ID, RGBA)
    assert s["mid"] == (20.0, 20.0) and s["dir"] == (1.0, 0.0)
    s = R.format_label((10.0, 20.0, 30.0, 20.0), _firing(), ID, RGBA)
    assert s["mid"] == (20.0, 20.0) and s["dir"][0] == 1.0 and s["dir"][1] == 0.0
    s = R.format_label((10.0, 10.0, 10.0, 30.0), _firing(), ID, RGBA)           # d = (0, -20): e = (-0, 1)
    assert s["dir"][0] == 0.0 and s["dir"][1] == 1.0
    s = R.format_label((10.0, 30.0, 10.0, 10.0), _firing(), ID, RGBA)           # d = (0, 20): e = (-0, -1)
    assert s["dir"][0] == 0.0 and s["dir"][1] == -1.0
    s = R.format_label((3.0, 4.0, 0.0, 0.0), _firing(), (2.0, 2.0, 1.0, 1.0), RGBA)   # P0 = (7, 9), P1 = (1, 1): d = (6, 8), len 10
    assert s["mid"] == (4.0, 5.0) and s["dir"] == (f32(0.6), f32(0.8))


def test_no_label():
    line = (30.0, 20.0, 10.0, 20.0)
    assert R.format_label(line, _firing(meters=999999.5), ID, RGBA)["runs"] == []
    below = math.nextafter(999999.5, 0.0)
    assert _rows(R.format_label(line, _firing(meters=below), ID, RGBA))[0] == b"999999m"
    assert R.format_label(line, _firing(meters=NAN), ID, RGBA)["runs"] == []
    assert R.format_label(line, _firing(source=R.NONE), ID, RGBA)["runs"] == []
    assert R.format_label((5.0, 5.0, 5.0, 5.0), _firing(), ID, RGBA)["runs"] == []
    for bad in ((float("inf"), 1.0, 2.0, 3.0), (1.0, NAN, 2.0, 3.0), (1.0, 2.0, float("-inf"), 3.0), (1.0, 2.0, 3.0, NAN)):
        s = R.format_label(bad, _firing(), ID, RGBA)
        assert s["runs"] == [] and s["mid"] == (0.0, 0.0) and s["dir"] == (0.0, 0.0) and s["rgba"] == RGBA
    # finite in map coordinates, not finite through the viewport
    assert R.format_label((3e38, 1.0, 2.0, 3.0), _firing(), (4.0, 1.0, 0.0, 0.0), RGBA)["runs"] == []


def test_the_pixel_rule_on_a_label_derived_by_hand():
    # P0 = (30, 20), P1 = (10, 20): d = (20, 0), M = (20, 20), e = (1, 0); S = 1: u = cx - 20, v = cy - 20.  Rows "5m" 12, "RANGE!" 36
    # (W2 = 36), "-> 180deg" 42, "<- 0deg" 30 (W4 = 42): x2 = -36 + 30, -36 + 6, -36 + 0, -36 + 12.
    s = R.format_label((30.0, 20.0, 10.0, 20.0), _firing(meters=5.0, mils=(NAN, NAN), bearing=(0.0, 180.0)), ID, RGBA)
    assert s["runs"] == [(-6, 0, b"5m"), (-30, 18, b"RANGE!"), (-36, 36, b"-> 180" + DEG), (-24, 54, b"<- 0" + DEG)]
    img = np.zeros((64, 64, 4), np.uint8)
    n = R.draw(img, [s], 1)
    on = img[..., 3] == 255
    # "5m" starts at u = -3.  The '5': its top row (#####) is iv = 1, v in [1, 2): Y = 21; iu = 0 .. 4: u in [-3, 2): X = 17 .. 21
    assert on[21, 17:22].all() and not on[21, 22] and not on[21, 16] and not on[20].any()
    # its second row (#....): X = 17 only
    assert on[22, 17] and not on[22, 18:23].any()
    # 'm' starts at iu = 6, X = 23; its rows 0 and 1 are blank, row 2 (##.#.) is Y = 23: X = 23, 24, 26
    assert not on[21, 23:29].any() and not on[22, 23:29].any() and list(on[23, 23:29]) == [True, True, False, True, False, False]
    # "RANGE!" starts at u = -15 (X = 5) and hangs 9 rows lower: 'R' row 0 (####.) is Y = 30, X = 5 .. 8
    assert on[30, 5:9].all() and not on[30, 9:11].any() and not on[30, :5].any() and not on[29].any()
    assert np.all(img[on] == np.array(RGBA, np.uint8)) and n == on.sum()
    # draw() and the pixel-at-a-time rule agree
    for Y in range(18, 60):
        for X in range(0, 50):
            assert R.pixel_hit(s, X, Y, 1) == bool(on[Y, X]), (X, Y)
    # S = 3 about M = (60, 60): the same glyphs, three pixels per font unit: the '5's top row is X = 51 .. 65, Y = 63 .. 65
    img3 = np.zeros((192, 192, 4), np.uint8)
    s3 = R.format_label((90.0, 60.0, 30.0, 60.0), _firing(meters=5.0, mils=(NAN, NAN), bearing=(0.0, 180.0)), ID, RGBA)
    assert s3["runs"] == s["runs"]
    R.draw(img3, [s3], 3)
    on3 = img3[..., 3] == 255
    assert on3.sum() == 9 * on.sum() and on3[63:66, 51:66].all() and not on3[63:66, 66:69].any() and not on3[60:63].any()


def test_later_labels_paint_over_earlier_ones():
    c = LC.stack_case(RW, RH, 8)
    vp = (c.view.scale[0], c.view.scale[1], c.view.top_left[0], c.view.top_left[1])
    slots = [R.format_label(l, LC.synthetic_firing(l, c.view), vp, rgba) for l, rgba in c.lines]
    img = np.zeros((c.window[1], c.window[0], 4), np.uint8)
    n = R.draw(img, slots, c.S)
    assert n >= c.minimum
    assert np.all(img[img[..., 3] == 255] == np.array(c.lines[-1][1], np.uint8))


def test_the_python_builders():
    import squad_mortar_helper_amd as smh
    L = smh._lib
    custom = [((1.0, 2.0), (30.0, 40.0)), ((5.5, 6.25), (7.0, 8.0))]
    lines = smh.label_lines(custom, drag=((0.0, 0.0), (3.0, 5.0)), measure=((0.0, 0.0), (6.0, 0.0)))
    # the drag is sqrt(34) < 6 long: dropped; the measuring line is exactly 6: kept (>=), in red
    assert lines == [((1.0, 2.0, 30.0, 40.0), (255, 0, 255, 255)), ((5.5, 6.25, 7.0, 8.0), (255, 0, 255, 255)), ((0.0, 0.0, 6.0, 0.0), (255, 0, 0, 255))]
    assert [l[0] for l in lines[:2]] == [p[:4] for p in smh.ctl_marker_prims(custom)]
    lo, keep = smh.LabelOptions(lines, detected=True, scale=3, mpx=0.25).struct()
    assert (lo.size, lo.flags, lo.scale, lo.n_extra) == (C.sizeof(L.LabelOptionsStruct), L.LABEL_DETECTED, 3, 3)
    assert lo.extra[2].line.x1 == 6.0 and tuple(lo.extra[2].rgba) == (255, 0, 0, 255) and lo.mpx[0] == 0.25
    lo, keep = smh.LabelOptions(detected=False).struct()
    assert (lo.flags, lo.scale, lo.n_extra) == (0, 0, 0) and not lo.extra and not lo.mpx


def test_the_headers_structs_have_the_documented_layout(tmp_path):
    from squad_mortar_helper_amd import _lib as L
    src = tmp_path / "labels_abi.c"
    exe = tmp_path / "labels_abi"
    fields = ["sizeof(smhv_label_line)", "offsetof(smhv_label_line, rgba)", "sizeof(smhv_label_options)", "offsetof(smhv_label_options, extra)",
              "offsetof(smhv_label_options, mpx)", "sizeof(smhv_label_run)", "offsetof(smhv_label_run, n)", "offsetof(smhv_label_run, text)",
              "sizeof(smhv_label)", "offsetof(smhv_label, mid)", "offsetof(smhv_label, dir)", "offsetof(smhv_label, rgba)", "offsetof(smhv_label, n_runs)",
              "offsetof(smhv_label, run)", "sizeof(smhv_label_result)", "offsetof(smhv_label_result, label)", "SMHV_LABEL_DETECTED", "SMHV_LABEL_MAX_EXTRA"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\nint main(void) {\n' +
                   "".join('printf("%%zu\\n", (size_t)(%s));\n' % f for f in fields) + "return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [20, 16, 32, 16, 24, 24, 4, 8, 216, 48, 56, 64, 68, 72, 8 + 216 * 96, 8, 1, 64], got
    assert got[0] == C.sizeof(L.LabelLine) and got[2] == C.sizeof(L.LabelOptionsStruct) and got[5] == C.sizeof(L.LabelRun)
    assert got[8] == C.sizeof(L.Label) and got[14] == C.sizeof(L.LabelResult)
    assert (L.LabelLine.rgba.offset, L.LabelOptionsStruct.extra.offset, L.LabelOptionsStruct.mpx.offset) == (16, 16, 24)
    assert (L.LabelRun.n.offset, L.LabelRun.text.offset) == (4, 8)
    assert (L.Label.mid.offset, L.Label.dir.offset, L.Label.rgba.offset, L.Label.n_runs.offset, L.Label.run.offset) == (48, 56, 64, 68, 72)
    assert L.LabelResult.label.offset == 8 and L.LABEL_SLOTS == 96 and L.LABEL_MAX_EXTRA == 64 and L.LABEL_DETECTED == 1


@pytest.mark.parametrize("case", LC.all_cases(RW, RH), ids=lambda c: c.name)
def test_every_case_meets_its_declared_minimum_on_the_restatement(case):
    vp = (case.view.scale[0], case.view.scale[1], case.view.top_left[0], case.view.top_left[1])
    for source in (R.SCALES, R.HEIGHTMAP):
        slots = [R.format_label(l, LC.synthetic_firing(l, case.view, source), vp, rgba) for l, rgba in case.lines]
        img = np.zeros((case.window[1], case.window[0], 4), np.uint8)
        n = R.draw(img, slots, case.S)
        if case.minimum is None:
            assert n == 0, (case, n)
        else:
            assert n >= case.minimum, (case, source, n)
    assert len(case.lines) <= 64
