"""The reach map without a GPU: the thresholds, the structs' layout against the header, the library's defaults, and the restatement
(tests/reach_ref.py) against cases derived by hand and against the firing solutions' restatement (tests/firing_ref.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import firing_ref as FR
import reach_cases as RC
import reach_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS_CASES = ("every band", "out of range by altitude", "origin outside, m/px", "seam", "flat circle", "origin outside, no m/px")
CROSS_PER_CASE = 400                                              # 6 x 400 >= the issue's 2000 samples


def cross_samples():
    """[(case, its restatement, [(x, y)])] of the cross-check against the firing solutions, the same on the host and on the device."""
    out = []
    for i, c in enumerate(x for x in RC.all_cases() if x.name in CROSS_CASES):
        r = RC.checked(c)
        out.append((c, r, RC.samples(r, CROSS_PER_CASE, 100 + i)))
    assert len(out) == len(CROSS_CASES) and sum(len(s) for _, _, s in out) >= 2000
    return out


def cross_check(c, r, pts, solve):
    """solve([(x0, y0, x1, y1)]) -> [(mils0, source)]: the class byte of every sampled pixel against the firing solution of its line.
    -> (samples, samples left out because mils lies within 1e-6 of a multiple of 100, classes seen)."""
    lines = [R.sample_line(r, c.viewport, x, y) for x, y in pts]
    skipped, seen = 0, set()
    for (x, y), (mils, source) in zip(pts, solve(lines)):
        c7 = int(r["classes"][y, x]) & 0x7F
        seen.add(c7)
        assert (source == FR.NONE) == (c7 == 0), (c.name, x, y, source, c7)
        if source == FR.NONE:
            continue
        assert math.isnan(mils) == (c7 == R.OUT_OF_RANGE), (c.name, x, y, mils, c7)
        if math.isnan(mils):
            continue
        if abs(mils - 100.0 * round(mils / 100.0)) <= 1e-6:
            skipped += 1
            continue
        assert min(max(math.floor((mils - 800.0) / 100.0), 0), 7) == c7 - R.BAND0, (c.name, x, y, mils, c7)
    return len(pts), skipped, seen


def test_thresholds_are_tan_of_the_band_edges_within_one_ulp(built):
    import squad_mortar_helper_amd as smh
    got = smh.reach_thresholds()
    assert got == R.THRESHOLDS
    for mils, t in zip(R.MILS, got):
        want = math.tan(mils * math.pi / 3200.0)
        assert abs(t - want) <= math.ulp(want), (mils, t.hex(), want.hex())
    assert all(a < b for a, b in zip(got, got[1:])) and len(got) == 7
    assert smh._lib.load().smhv_reach_thresholds(None) == smh._lib.E_INVALID
    # the edges are where they belong: q = tan(elevation), 1600 mils = a quarter turn
    assert got[0] > 1.0 and math.isclose(math.atan(got[3]) * 3200.0 / math.pi, 1200.0, rel_tol=1e-12)


def test_struct_layouts_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   'int main(void) {\n'
                   '  printf("smhv_reach_options %zu\\nsmhv_reach_result %zu\\n", sizeof(smhv_reach_options), sizeof(smhv_reach_result));\n'
                   '  O(smhv_reach_options, size); O(smhv_reach_options, flags); O(smhv_reach_options, origin_mode); O(smhv_reach_options, line);\n'
                   '  O(smhv_reach_options, origin); O(smhv_reach_options, ring_m); O(smhv_reach_options, out_of_range); O(smhv_reach_options, band);\n'
                   '  O(smhv_reach_options, ring); O(smhv_reach_options, reserved);\n'
                   '  O(smhv_reach_result, valid); O(smhv_reach_result, source_mask); O(smhv_reach_result, origin); O(smhv_reach_result, count);\n'
                   '  O(smhv_reach_result, ring); O(smhv_reach_result, reserved);\n'
                   '  printf("flags %u %u %u %u %u %u %u %u\\n", SMHV_REACH_PAINT, SMHV_REACH_CLASSES, SMHV_REACH_ORIGIN_POINT, SMHV_REACH_ORIGIN_LINE_P0,\n'
                   '         SMHV_REACH_ORIGIN_LINE_P1, SMHV_REACH_OUT_OF_RANGE, SMHV_REACH_BAND0, SMHV_REACH_RING);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("flags") else ("flags", ln[6:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["smhv_reach_options"]) == 80 == C.sizeof(L.ReachOptionsStruct)
    assert int(got["smhv_reach_result"]) == 64 == C.sizeof(L.ReachResult)
    pinned = {"size": 0, "flags": 4, "origin_mode": 8, "line": 12, "origin": 16, "ring_m": 24, "out_of_range": 32, "band": 36, "ring": 68, "reserved": 72}
    for f, off in pinned.items():
        assert int(got["smhv_reach_options." + f]) == off == getattr(L.ReachOptionsStruct, f).offset, f
    pinned = {"valid": 0, "source_mask": 4, "origin": 8, "count": 16, "ring": 52, "reserved": 56}
    for f, off in pinned.items():
        assert int(got["smhv_reach_result." + f]) == off == getattr(L.ReachResult, f).offset, f
    assert [int(v) for v in got["flags"].split()] == [L.REACH_PAINT, L.REACH_CLASSES, L.REACH_ORIGIN_POINT, L.REACH_ORIGIN_LINE_P0, L.REACH_ORIGIN_LINE_P1,
                                                      L.REACH_OUT_OF_RANGE, L.REACH_BAND0, L.REACH_RING] == [1, 2, 0, 1, 2, 1, 2, 0x80]


def test_defaults(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    o = L.ReachOptionsStruct()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    assert lib.smhv_reach_defaults(C.byref(o)) == 0
    assert (o.size, o.flags, o.origin_mode, o.line, tuple(o.origin), o.ring_m, tuple(o.reserved)) == (80, L.REACH_PAINT, L.REACH_ORIGIN_POINT, 0, (0.0, 0.0), 0.0, (0, 0))
    p = R.DEFAULT_PALETTE
    assert tuple(o.out_of_range) == p["out_of_range"] and tuple(o.ring) == p["ring"] and [tuple(b) for b in o.band] == p["band"]
    assert lib.smhv_reach_defaults(None) == L.E_INVALID
    # the Python options are the defaults with their own fields on top
    s = smh.ReachOptions(origin=("p1", 3), ring_m=250.0, paint=False, classes=True).struct()
    assert (s.size, s.flags, s.origin_mode, s.line, s.ring_m) == (80, L.REACH_CLASSES, L.REACH_ORIGIN_LINE_P1, 3, 250.0) and tuple(s.ring) == p["ring"]
    pal = dict(out_of_range=(1, 2, 3, 4), ring=(5, 6, 7, 8), band=[(k, k + 1, k + 2, 255) for k in range(8)])
    s = smh.ReachOptions(origin=(1.5, -2.0), palette=pal).struct()
    assert tuple(s.origin) == (1.5, -2.0) and tuple(s.out_of_range) == (1, 2, 3, 4) and tuple(s.band[7]) == (7, 8, 9, 255) and s.flags == L.REACH_PAINT


@pytest.mark.parametrize("case", RC.all_cases(), ids=lambda c: c.name)
def test_every_case_holds_what_it_is_for(case):
    r = RC.checked(case)
    s = R.summary(r)
    assert sum(s["count"]) == int(((r["classes"] & 0x7F) != 0).sum()) and s["valid"] == r["valid"]
    # the rings change nothing but the ring bit, and without a spacing there is none
    bare = RC.restate(case, ring_m=0.0)
    assert np.array_equal(bare["classes"], r["classes"] & 0x7F) and not (bare["classes"] & R.RING).any()


def test_hand_derived_pixels():
    """Numbers worked out on paper, not by the restatement's own formulas."""
    # flat ground, scales branch, 10 m per pixel, origin at the centre of pixel (0, 0): pixel (X, 0) is 10 X metres away
    r = R.reach((0.5, 0.5), (130, 1), None, None, 10.0, None, True, 250.0)
    c = r["classes"][0]
    assert np.array_equal(r["meters"][0], 10.0 * np.arange(130))
    # V^2 / g = 1232.25 m: 123 pixels (1230 m) are in range, 124 (1240 m) are not
    assert (c[:124] & 0x7F >= R.BAND0).all() and (c[124:] & 0x7F == R.OUT_OF_RANGE).all()
    assert c[0] & 0x7F == R.BAND0 + 7                              # m == 0: q = +inf, straight up
    # the high-angle solution at m metres is 1600 - (3200 / pi) * asin(g m / V^2) / 2 mils: 1000 m -> 1122.2 mils (band 3), 500 m ->
    # 1387.1 (band 5), 100 m -> 1558.6 (band 7), 1200 m -> 931.9 (band 1), 1230 m -> 846.6 (band 0)
    for px, band in ((100, 3), (50, 5), (10, 7), (120, 1), (123, 0)):
        mils = 1600.0 - (3200.0 / math.pi) * math.asin(FR.G * 10.0 * px / FR.V2) / 2.0
        assert min(max(math.floor((mils - 800.0) / 100.0), 0), 7) == band and c[px] & 0x7F == R.BAND0 + band, (px, mils, c[px])
    # rings every 250 m: floor(10 X / 250) steps between X = 24 and 25, 49 and 50, ...; the pixel LEFT of the step carries the bit
    want = np.zeros(130, bool)
    want[[24, 49, 74, 99, 124]] = True
    assert np.array_equal((c & R.RING) != 0, want)
    # paint: 200 -> (200 * (255 - 72) + 40 * 72 + 127) / 255 = 155 for band 0's red channel; alpha stays
    img = np.full((1, 130, 4), 200, np.uint8)
    img[..., 3] = 17
    R.paint(img, r["classes"])
    assert tuple(img[0, 123]) == ((200 * 183 + 40 * 72 + 127) // 255, (200 * 183 + 90 * 72 + 127) // 255, (200 * 183 + 255 * 72 + 127) // 255, 17)
    assert tuple(img[0, 123]) == (155, 169, 216, 17)
    ringed = (200 * 183 + 255 * 72 + 127) // 255                   # band 6 at X = 24 (1493 mils), red 255; then white at a = 160
    assert img[0, 24, 0] == (ringed * 95 + 255 * 160 + 127) // 255 and (img[..., 3] == 17).all()
    s = R.summary(r)
    assert s["count"][0] == 6 and sum(s["count"]) == 130 and s["ring"] == 5 and s["source_mask"] == 1 << R.SCALES and s["valid"] == 1


def test_the_restatement_agrees_with_the_firing_restatement_and_meets_the_cap():
    """The pass tied to what is already pinned: the class byte against milliradians::calc of the same line, on the host (libm's atan);
    samples within 1e-6 of a band edge are left out, and they are at most 1 % of the samples."""
    total = skipped = 0
    seen = {}
    for c, r, pts in cross_samples():
        def solve(lines, c=c):
            out = []
            for ln in lines:
                met = FR.record_meters(ln, c.mpx) if c.mpx is not None else None
                f = FR.firing_line(tuple(float(v) for v in ln), c.minimap, met, c.hm, c.fit, c.viewport)
                out.append((f["mils"][0], f["source"]))
            return out
        n, k, classes = cross_check(c, r, pts, solve)
        total, skipped = total + n, skipped + k
        seen[c.name] = classes
        assert classes == set(int(v) for v in np.unique(r["classes"] & 0x7F)), c.name       # every class present is sampled
    assert total >= 2000 and skipped <= total // 100, (total, skipped)
    assert set().union(*seen.values()) == set(range(10))
