"""Terrain clearance without a GPU: the structs' layout and the constants against a C program compiled from the header, the
library's defaults and the Python options, the restatement (tests/clearance_ref.py) against values worked by hand, and every case's
own assertions (tests/clearance_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clearance_cases as CC
import clearance_ref as R
import firing_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_and_constants_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    opts = ["size", "flags", "samples", "origin_mode", "line", "reserved0", "origin", "margin_m", "out_of_range", "clear", "blocked", "los", "reserved"]
    dirs = ["status", "first_blocked", "n_blocked", "los_blocked", "min_margin", "min_at", "reserved"]
    maps = ["valid", "reserved", "origin", "count", "los_blocked"]
    body = "".join('  O(smhv_clearance_options, %s);\n' % f for f in opts) + "".join('  O(smhv_clearance_dir, %s);\n' % f for f in dirs)
    body += "".join('  O(smhv_clearance_map_result, %s);\n' % f for f in maps)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   '#define Z(t) printf(#t " %zu\\n", sizeof(t))\n'
                   'int main(void) {\n'
                   '  Z(smhv_clearance_options); Z(smhv_clearance_dir); Z(smhv_clearance); Z(smhv_clearance_result); Z(smhv_clearance_map_result);\n'
                   '  O(smhv_clearance, dir); O(smhv_clearance_result, n_lines); O(smhv_clearance_result, reserved); O(smhv_clearance_result, line);\n'
                   + body +
                   '  printf("consts %u %u %u %u %u %u %u %u %u\\n", SMHV_CLEAR_MAX_SAMPLES, SMHV_CLEAR_PAINT, SMHV_CLEAR_BYTES, SMHV_CLEAR_NONE,\n'
                   '         SMHV_CLEAR_OUT_OF_RANGE, SMHV_CLEAR_CLEAR, SMHV_CLEAR_BLOCKED, SMHV_CLEAR_LOS_BLOCKED, (unsigned)SMHV_MAX_LINES);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("consts") else ("consts", ln[7:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["smhv_clearance_options"]) == 64 == C.sizeof(L.ClearanceOptionsStruct)
    assert int(got["smhv_clearance_dir"]) == 32 == C.sizeof(L.ClearanceDir)
    assert int(got["smhv_clearance"]) == 64 == C.sizeof(L.Clearance)
    assert int(got["smhv_clearance_result"]) == 8 + 64 * 32 == C.sizeof(L.ClearanceResult)
    assert int(got["smhv_clearance_map_result"]) == 32 == C.sizeof(L.ClearanceMapResult)
    assert int(got["smhv_clearance_result.line"]) == 8 == L.ClearanceResult.line.offset and int(got["smhv_clearance.dir"]) == 0
    # laid out as smhv_firing_result is: the count, a reserved word, then SMHV_MAX_LINES entries
    assert (L.ClearanceResult.n_lines.offset, L.ClearanceResult.reserved.offset) == (L.FiringResult.n_lines.offset, L.FiringResult.reserved.offset) == (0, 4)
    pinned = dict(size=0, flags=4, samples=8, origin_mode=12, line=16, reserved0=20, origin=24, margin_m=32, out_of_range=40, clear=44, blocked=48, los=52,
                  reserved=56)
    assert sorted(pinned) == sorted(opts)
    for f, off in pinned.items():
        assert int(got["smhv_clearance_options." + f]) == off == getattr(L.ClearanceOptionsStruct, f).offset, f
    pinned = dict(status=0, first_blocked=4, n_blocked=8, los_blocked=12, min_margin=16, min_at=24, reserved=28)
    for f, off in pinned.items():
        assert int(got["smhv_clearance_dir." + f]) == off == getattr(L.ClearanceDir, f).offset, f
    pinned = dict(valid=0, reserved=4, origin=8, count=16, los_blocked=28)
    for f, off in pinned.items():
        assert int(got["smhv_clearance_map_result." + f]) == off == getattr(L.ClearanceMapResult, f).offset, f
    assert [int(v) for v in got["consts"].split()] == [L.CLEAR_MAX_SAMPLES, L.CLEAR_PAINT, L.CLEAR_BYTES, L.CLEAR_NONE, L.CLEAR_OUT_OF_RANGE, L.CLEAR_CLEAR,
                                                       L.CLEAR_BLOCKED, L.CLEAR_LOS_BLOCKED, L.MAX_LINES] == [256, 1, 2, 0, 1, 2, 3, 0x80, 32]
    assert (R.MAX_SAMPLES, R.PROFILE, L.CLEAR_PROFILE) == (256, 257, 257)
    assert (R.NONE, R.OUT_OF_RANGE, R.CLEAR, R.BLOCKED, R.LOS_BLOCKED) == (L.CLEAR_NONE, L.CLEAR_OUT_OF_RANGE, L.CLEAR_CLEAR, L.CLEAR_BLOCKED, L.CLEAR_LOS_BLOCKED)


def test_defaults_and_the_python_options_round_trip(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    o = L.ClearanceOptionsStruct()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    assert lib.smhv_clearance_defaults(C.byref(o)) == 0
    assert (o.size, o.flags, o.samples, o.origin_mode, o.line, o.reserved0, tuple(o.origin), o.margin_m, tuple(o.reserved)) == \
        (64, L.CLEAR_PAINT, 64, L.REACH_ORIGIN_POINT, 0, 0, (0.0, 0.0), 0.0, (0, 0))
    p = R.DEFAULT_PALETTE
    assert (tuple(o.out_of_range), tuple(o.clear), tuple(o.blocked), tuple(o.los)) == (p["out_of_range"], p["clear"], p["blocked"], p["los"])
    assert p["blocked"] == (230, 40, 40, 110) and p["los"] == (0, 0, 0, 70) and p["clear"] == p["out_of_range"] == (0, 0, 0, 0)
    assert lib.smhv_clearance_defaults(None) == L.E_INVALID
    s = smh.ClearanceOptions(samples=200, margin_m=12.5, origin=("p1", 3), paint=False, bytes=True).struct()
    assert (s.size, s.flags, s.samples, s.margin_m, s.origin_mode, s.line) == (64, L.CLEAR_BYTES, 200, 12.5, L.REACH_ORIGIN_LINE_P1, 3) and tuple(s.blocked) == p["blocked"]
    s = smh.ClearanceOptions(origin=("p0", 31)).struct()
    assert (s.flags, s.samples, s.margin_m, s.origin_mode, s.line) == (L.CLEAR_PAINT, 64, 0.0, L.REACH_ORIGIN_LINE_P0, 31)
    pal = dict(out_of_range=(1, 2, 3, 4), clear=(5, 6, 7, 8), blocked=(9, 10, 11, 12), los=(13, 14, 15, 255))
    s = smh.ClearanceOptions(origin=(1.5, -2.0), paint=True, bytes=True, palette=pal).struct()
    assert tuple(s.origin) == (1.5, -2.0) and s.flags == L.CLEAR_PAINT | L.CLEAR_BYTES and s.origin_mode == L.REACH_ORIGIN_POINT
    assert (tuple(s.out_of_range), tuple(s.clear), tuple(s.blocked), tuple(s.los)) == (pal["out_of_range"], pal["clear"], pal["blocked"], pal["los"])


def test_the_800_m_line_by_hand():
    """Level ground, 800 m: sin(2 theta) = g d / V^2 = 0.6492, the high angle is theta = 69.76 degrees, q = tan(theta) = 2.71.  780 m out the
    arc is 780 q - g 780^2 (1 + q^2) / (2 V^2) = 2115.3 - 2062.4 = 52.9 m up: a wall of 60 m there blocks, one of 40 m does not."""
    disc, q = R.high_angle(800.0, 0.0)
    assert disc > 0.0 and abs(float(q) - 2.71) < 0.005
    theta = (np.pi - np.arcsin(FR.G * 800.0 / FR.V2)) / 2.0
    assert abs(np.degrees(theta) - 69.76) < 0.01 and abs(np.tan(theta) - float(q)) < 1e-9
    a = float(R.arc_height(800.0, q, 780.0))
    assert abs(a - 53.0) < 1.0 and abs(a - (780.0 * 2.7119 - 9.8 * 780.0 ** 2 * (1.0 + 2.7119 ** 2) / (2.0 * 109.890938 ** 2))) < 0.1
    line = [(10.0, 30.0, 810.0, 30.0)]                             # S = 40: a sample every 20 m, k = 39 at 780 m, on column 790
    for wall, status in ((60.0, R.BLOCKED), (40.0, R.CLEAR)):
        hm = CC.hill_with_wall(wall)
        (fwd, bck), = R.lines(line, 40, 0.0, CC.whole(hm), hm)[0]
        assert fwd["status"] == status, (wall, fwd)
        assert fwd["min_at"] == 39 and abs(fwd["min_margin"] - (a - wall)) < 1e-9
        assert fwd["n_blocked"] == (1 if status == R.BLOCKED else 0) and fwd["first_blocked"] == (39 if status == R.BLOCKED else 40)
        # the sight line: the hill's two samples (k = 19 and 20, columns 390 and 410) and the wall's; level ground itself does not
        # block (l = 0 < z = 0 is false)
        assert fwd["los_blocked"] == 3 == bck["los_blocked"]
        # from the other end the wall is 20 m from the tube, where the arc is as high as it is 20 m before the target: the same verdict
        assert bck["status"] == status and bck["min_at"] == 1 and abs(bck["min_margin"] - fwd["min_margin"]) < 1e-6
    # a margin of 15 m turns the 40 m wall (12.9 m under the arc) into a block
    hm = CC.hill_with_wall(40.0)
    (fwd, _), = R.lines(line, 40, 15.0, CC.whole(hm), hm)[0]
    assert fwd["status"] == R.BLOCKED and fwd["first_blocked"] == 39


def test_the_division_by_65535_in_three_operations(tmp_path):
    """The device forms (double)v / 65535.0 as v * r, one fused remainder and one fused correction (csrc/smh_firing.h, clear_height):
    the same operations in C, with the header's own constant, against the division for every 16-bit v."""
    import re
    hdr = open(os.path.join(ROOT, "squad-mortar-helper_amd", "csrc", "smh_firing.h")).read()
    rcp = re.search(r"#define SMH_RCP_65535 (\S+)", hdr).group(1)
    assert float.fromhex(rcp) == 1.0 / 65535.0 and "fma(fma(-q0, 65535.0, n), SMH_RCP_65535, q0)" in hdr
    src = tmp_path / "div.c"
    src.write_text('#include <math.h>\n#include <stdio.h>\n#include <string.h>\n'
                   'int main(void) {\n  const double r = %s;\n  int bad = 0, plain = 0;\n'
                   '  for (unsigned v = 0; v <= 65535u; ++v) {\n'
                   '    const double n = (double)v, q0 = n * r, q = fma(fma(-q0, 65535.0, n), r, q0), want = n / 65535.0;\n'
                   '    bad += memcmp(&q, &want, 8) != 0; plain += memcmp(&q0, &want, 8) != 0;\n  }\n'
                   '  printf("%%d %%d\\n", bad, plain);\n  return 0;\n}\n' % rcp)
    exe = tmp_path / "div"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-ffp-contract=off", "-Wall", "-Werror", str(src), "-o", str(exe), "-lm"])
    bad, plain = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert bad == 0 and plain > 0                                   # exact with the corrections, and not without them: they are no decoration


def test_the_arc_lands_on_the_target():
    """a at x = d is alt, within 1e-6 m, on 1,000 random in-range lines: q solves the trajectory through (d, alt)."""
    rng = np.random.default_rng(3)
    d, alt = rng.uniform(1.0, 1200.0, 4000), rng.uniform(-150.0, 150.0, 4000)
    disc, q = R.high_angle(d, alt)
    keep = np.nonzero(disc >= 0.0)[0][:1000]
    assert len(keep) == 1000
    a = R.arc_height(d[keep], q[keep], d[keep])
    assert np.abs(a - alt[keep]).max() < 1e-6, np.abs(a - alt[keep]).max()
    # and the high angle it is: steeper than 45 degrees
    assert (q[keep] >= 1.0).all()


def test_min_margin_ties_nans_and_single_samples():
    """The least m is replaced only by a smaller one: on level ground the arc is symmetric, and of the two equal least margins (k = 1
    and k = S - 1 are NOT equal in floating point, so the tie is made by hand) the lower k stays."""
    flat = CC.flat_map()
    # S = 1: no interior sample: CLEAR, S, 0 counts, min_margin reported as 0
    (a, b), = R.lines([(10.0, 30.0, 810.0, 30.0)], 1, 0.0, CC.whole(flat), flat)[0]
    assert a == b == dict(status=R.CLEAR, first_blocked=1, n_blocked=0, los_blocked=0, min_margin=0.0, min_at=0)
    # S = 2: the one sample is the midpoint, the apex: 800 q / 4 = d q / 4 up on level ground
    (a, _), = R.lines([(10.0, 30.0, 810.0, 30.0)], 2, 0.0, CC.whole(flat), flat)[0]
    q = float(R.high_angle(800.0, 0.0)[1])
    assert a["min_at"] == 1 and abs(a["min_margin"] - 800.0 * q / 4.0) < 1e-6
    # an exact tie: a heightmap whose every sample gives the same m is not to be had, so the rule itself is driven with equal margins
    data = np.zeros((1, 8), np.uint16)
    r = R.sample_rule(np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), data, 1.0, 8, 0.0)
    assert int(r["status"][0]) == R.CLEAR and int(r["min_at"][0]) == 0 and float(r["min_margin"][0]) == 0.0 and int(r["first_blocked"][0]) == 8   # d == 0
    # NaN margins never win: a range of NaN is out of range, with zero arc counts
    r = R.sample_rule(np.array([np.nan]), np.array([0.0]), np.array([3.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([np.nan]), data, 1.0, 8, 0.0)
    assert int(r["status"][0]) == R.OUT_OF_RANGE and int(r["n_blocked"][0]) == 0 and float(r["min_margin"][0]) == 0.0


@pytest.mark.parametrize("case", CC.line_cases(), ids=lambda c: c.name)
def test_every_line_case_holds_what_it_is_for(case):
    recs, prof = CC.checked_lines(case)
    assert len(recs) == len(case.lines) and prof.shape == (len(case.lines), R.PROFILE) and prof.dtype == np.float32
    for (a, b), row in zip(recs, prof):
        if a["status"] == R.NONE:
            assert b["status"] == R.NONE and not row.any()
        else:
            assert b["status"] != R.NONE and not row[case.samples + 1:].any()
        for d in (a, b):
            if d["status"] in (R.CLEAR, R.OUT_OF_RANGE):
                assert d["n_blocked"] == 0 and d["first_blocked"] == case.samples
            if d["status"] == R.BLOCKED:
                assert 1 <= d["first_blocked"] < case.samples and 1 <= d["n_blocked"] < case.samples and d["min_margin"] < case.margin


@pytest.mark.parametrize("case", CC.map_cases(), ids=lambda c: c.name)
def test_every_map_case_holds_what_it_is_for(case):
    r = CC.checked_map(case)
    s = R.summary(r)
    assert sum(s["count"]) == int(((r["bytes"] & 0x7F) != 0).sum()) and s["valid"] == r["valid"]
    assert set(int(v) for v in np.unique(r["bytes"])) <= {0, 1, 2, 3, 0x81, 0x82, 0x83}


def test_the_dense_form_is_the_line_form_pixel_by_pixel():
    """One rule, two callers: the byte of a window pixel is the status and the LOS count of the line (origin, the pixel's target),
    direction 0, as lines() judges it."""
    c = next(x for x in CC.map_cases() if x.name == "window 65 x 17")
    r = CC.checked_map(c)
    sw, sh, tx, ty = (np.float32(v) for v in c.viewport)
    rng = np.random.default_rng(9)
    pts = [(int(x), int(y)) for x, y in zip(rng.integers(0, 65, 300), rng.integers(0, 17, 300))]
    lns = [(c.origin[0], c.origin[1], (np.float32(x) + np.float32(0.5) - tx) / sw, (np.float32(y) + np.float32(0.5) - ty) / sh) for x, y in pts]
    recs, _ = R.lines(lns, c.samples, c.margin, c.minimap, c.hm, c.fit, c.viewport)
    seen = set()
    for (x, y), (fwd, _) in zip(pts, recs):
        want = fwd["status"] | (R.LOS_BLOCKED if fwd["los_blocked"] else 0)
        assert int(r["bytes"][y, x]) == want, (x, y, fwd)
        seen.add(want & 0x7F)
    assert seen == {0, 1, 2, 3}


def test_a_wrong_sample_count_shows():
    wall = next(c for c in CC.line_cases() if c.name == "wall, S = 64")
    a, pa = CC.restate_lines(wall)
    b, pb = CC.restate_lines(wall, samples=65)
    assert a != b and not np.array_equal(pa, pb)
    land = next(c for c in CC.map_cases() if c.name == "130 x 33 panned, S = 64")
    assert not np.array_equal(CC.checked_map(land)["bytes"], CC.restate_map(land, samples=65)["bytes"])
