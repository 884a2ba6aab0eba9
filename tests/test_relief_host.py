"""The terrain relief without a GPU: the structs' layout against the header, the exported symbols, the library's defaults, the
Python options, what the entry points refuse before they ask for a device, and the restatement (tests/relief_ref.py) against cases
derived by hand and against itself with one rule changed at a time."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import relief_cases as RC
import relief_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smhv_relief_defaults", "smhv_batch_relief", "smhv_batch_read_relief", "smhv_batch_relief_ptr", "smhv_relief_map")
# the rule changed -> the family whose cases must notice, and the outputs they may notice it in
MUTANTS = {"nearest": "bilinear", "round_l": "level", "trunc": "below base", "left": "witness", "clamp": "witness", "den": "den", "no_half": "shade"}


def test_struct_layouts_and_constants_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   'int main(void) {\n'
                   '  printf("smhv_relief_options %zu\\nsmhv_relief_result %zu\\nsmhv_relief_planes %zu\\n", sizeof(smhv_relief_options),\n'
                   '         sizeof(smhv_relief_result), sizeof(smhv_relief_planes));\n'
                   '  O(smhv_relief_options, size); O(smhv_relief_options, flags); O(smhv_relief_options, major_every); O(smhv_relief_options, reserved0);\n'
                   '  O(smhv_relief_options, interval_m); O(smhv_relief_options, base_m); O(smhv_relief_options, exaggeration); O(smhv_relief_options, light);\n'
                   '  O(smhv_relief_options, contour); O(smhv_relief_options, major); O(smhv_relief_options, shade_weight); O(smhv_relief_options, reserved);\n'
                   '  O(smhv_relief_result, valid); O(smhv_relief_result, n_height); O(smhv_relief_result, n_contour); O(smhv_relief_result, n_major);\n'
                   '  O(smhv_relief_result, z_min); O(smhv_relief_result, z_max); O(smhv_relief_result, reserved);\n'
                   '  O(smhv_relief_planes, bytes); O(smhv_relief_planes, shades); O(smhv_relief_planes, heights);\n'
                   '  printf("flags %u %u %u %u %u %u %u %u\\n", SMHV_RELIEF_PAINT, SMHV_RELIEF_BYTES, SMHV_RELIEF_SHADES, SMHV_RELIEF_HEIGHTS,\n'
                   '         SMHV_RELIEF_NEAREST, SMHV_RELIEF_HAS_HEIGHT, SMHV_RELIEF_CONTOUR, SMHV_RELIEF_MAJOR);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("flags") else ("flags", ln[6:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["smhv_relief_options"]) == 80 == C.sizeof(L.ReliefOptionsStruct)
    assert int(got["smhv_relief_result"]) == 48 == C.sizeof(L.ReliefResult)
    assert int(got["smhv_relief_planes"]) == 24 == C.sizeof(L.ReliefPlanes)
    pinned = {"size": 0, "flags": 4, "major_every": 8, "reserved0": 12, "interval_m": 16, "base_m": 24, "exaggeration": 32, "light": 40, "contour": 64,
              "major": 68, "shade_weight": 72, "reserved": 76}
    for f, off in pinned.items():
        assert int(got["smhv_relief_options." + f]) == off == getattr(L.ReliefOptionsStruct, f).offset, f
    pinned = {"valid": 0, "n_height": 4, "n_contour": 8, "n_major": 12, "z_min": 16, "z_max": 24, "reserved": 32}
    for f, off in pinned.items():
        assert int(got["smhv_relief_result." + f]) == off == getattr(L.ReliefResult, f).offset, f
    for f, off in {"bytes": 0, "shades": 8, "heights": 16}.items():
        assert int(got["smhv_relief_planes." + f]) == off == getattr(L.ReliefPlanes, f).offset, f
    assert [int(v) for v in got["flags"].split()] == [L.RELIEF_PAINT, L.RELIEF_BYTES, L.RELIEF_SHADES, L.RELIEF_HEIGHTS, L.RELIEF_NEAREST, L.RELIEF_HAS_HEIGHT,
                                                      L.RELIEF_CONTOUR, L.RELIEF_MAJOR] == [1, 2, 4, 8, 16, 1, 2, 4]
    assert (R.PAINT, R.BYTES, R.SHADES, R.HEIGHTS, R.NEAREST, R.HAS_HEIGHT, R.CONTOUR, R.MAJOR) == (1, 2, 4, 8, 16, 1, 2, 4)


def test_exported_symbols_and_the_defaults_bytes(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib._name], text=True)
    assert sorted(ln.split()[-1] for ln in out.splitlines() if "relief" in ln and ln.split()[-1].startswith("smhv_")) == sorted(SYMBOLS)
    o = L.ReliefOptionsStruct()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    assert lib.smhv_relief_defaults(C.byref(o)) == 0
    d = R.DEFAULTS
    import struct
    want = struct.pack("<IIII", 80, L.RELIEF_PAINT, d["major_every"], 0) + struct.pack("<ddd", d["interval_m"], d["base_m"], d["exaggeration"]) + \
        struct.pack("<ddd", *d["light"]) + bytes(d["contour"]) + bytes(d["major"]) + struct.pack("<II", d["shade_weight"], 0)
    assert bytes(o) == want and len(want) == 80
    assert tuple(o.light) == (-0.5, -0.5, math.sqrt(0.5)) and (o.interval_m, o.base_m, o.major_every, o.exaggeration, o.shade_weight) == (10.0, 0.0, 5, 1.0, 96)
    assert tuple(o.contour) == (60, 40, 20, 110) and tuple(o.major) == (60, 40, 20, 200)


def test_what_is_refused_before_a_device_is_asked(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    assert lib.smhv_relief_defaults(None) == L.E_INVALID
    o = smh.ReliefOptions().struct()
    ropt = L.RenderOptions()
    planes = L.ReliefPlanes()
    res = (L.ReliefResult * 1)()
    d = C.c_void_p()
    assert lib.smhv_batch_relief(None, 0, 1, None, C.byref(ropt), C.byref(o), C.byref(planes), None) == L.E_INVALID
    assert lib.smhv_batch_read_relief(None, 0, 1, res) == L.E_INVALID
    assert lib.smhv_batch_relief_ptr(None, C.byref(d)) == L.E_INVALID
    assert lib.smhv_relief_map(None, None, C.byref(ropt), C.byref(o), None, None, None, None, None, res) == L.E_INVALID


def test_the_python_options_round_trip(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    s = smh.ReliefOptions().struct()
    assert (s.size, s.flags, s.interval_m, s.major_every, s.shade_weight) == (80, L.RELIEF_PAINT, 10.0, 5, 96)
    s = smh.ReliefOptions(interval_m=2.5, base_m=-3.0, major_every=4, exaggeration=2.0, light=(0.0, 1.0, 0.25), nearest=True, paint=False, bytes=True,
                          shades=True, heights=True, contour=(1, 2, 3, 4), major=(5, 6, 7, 8), shade_weight=255).struct()
    assert s.flags == L.RELIEF_BYTES | L.RELIEF_SHADES | L.RELIEF_HEIGHTS | L.RELIEF_NEAREST and s.size == 80 and (s.reserved0, s.reserved) == (0, 0)
    assert (s.interval_m, s.base_m, s.major_every, s.exaggeration, tuple(s.light), s.shade_weight) == (2.5, -3.0, 4, 2.0, (0.0, 1.0, 0.25), 255)
    assert tuple(s.contour) == (1, 2, 3, 4) and tuple(s.major) == (5, 6, 7, 8)
    s = smh.ReliefOptions(interval_m=0.0, major_every=0, shade_weight=0).struct()
    assert (s.interval_m, s.major_every, s.shade_weight) == (0.0, 0, 0) and tuple(s.light) == R.DEFAULTS["light"]
    # the light: north-west at 45 degrees is the library's default to an ulp or two; the axes are the heightmap's (y down)
    lx, ly, lz = smh.relief_light(315.0, 45.0)
    assert math.isclose(lx, -0.5, abs_tol=1e-15) and math.isclose(ly, -0.5, abs_tol=1e-15) and math.isclose(lz, math.sqrt(0.5), abs_tol=1e-15)
    assert smh.relief_light() == (lx, ly, lz)
    for az, alt, want in ((0.0, 0.0, (0.0, -1.0, 0.0)), (90.0, 0.0, (1.0, 0.0, 0.0)), (180.0, 0.0, (0.0, 1.0, 0.0)), (123.0, 90.0, (0.0, 0.0, 1.0))):
        assert np.allclose(smh.relief_light(az, alt), want, atol=1e-15), (az, alt)


@pytest.mark.parametrize("case", RC.all_cases(), ids=lambda c: c.name)
def test_every_case_holds_what_it_is_for(case):
    r = RC.checked(case)
    s = R.summary(r)
    has = (r["bytes"] & R.HAS_HEIGHT) != 0
    assert s["n_height"] == int(has.sum()) and s["valid"] == r["valid"]
    assert np.array_equal(np.isnan(r["z"]), ~has) and (r["bytes"] <= 7).all()
    if s["n_height"]:
        assert s["z_min"] <= s["z_max"] and np.float32(s["z_min"]) == r["heights"][has].min() and np.float32(s["z_max"]) == r["heights"][has].max()
    else:
        assert (s["z_min"], s["z_max"]) == (0.0, 0.0)
    # without an interval nothing changes but the contour bits
    bare = RC.restate(case, interval_m=0.0)
    assert np.array_equal(bare["bytes"], r["bytes"] & R.HAS_HEIGHT) and np.array_equal(bare["shades"], r["shades"]) and np.array_equal(bare["heights"], r["heights"])


def test_every_family_and_every_issue_case_is_there():
    cases = RC.all_cases()
    assert set(MUTANTS.values()) <= set(c.family for c in cases)
    assert set(c.window for c in cases) >= {(1, 1), (63, 15), (64, 16), (65, 17), (130, 33)}
    assert set(c.hm[0].shape for c in cases if c.hm) >= {(1, 1), (2, 2), (5, 3), (64, 64)}
    assert set(c.opt["major_every"] for c in cases) >= {0, 1, 5} and set(c.opt["interval_m"] for c in cases) >= {0.0, 5e-324, 1e300}
    assert any(not c.fit for c in cases) and any(c.hm[2][2] < 0 for c in cases) and any(c.opt["light"][2] == 0.0 for c in cases)
    # the contour cases hold contours and index contours, the shade cases at least three shades (their own checks say how many)
    assert sum(int(((RC.checked(c)["bytes"] & R.MAJOR) != 0).sum()) for c in RC.by_family("level")) >= 50


def test_the_ramp_and_the_paint_by_hand():
    """Numbers worked out on paper, not by the restatement's own formulas."""
    c = next(x for x in RC.all_cases() if x.name == "integer coordinates, the ramp by hand")
    r = RC.checked(c)                                              # (the levels and the contour columns: relief_cases._check_ramp)
    # the shade by hand at X = 1: z = 1000, 2000 to the right, the same below: p = 1000, q = 0; light (-0.5, -0.5, sqrt(1/2)):
    # t = sqrt(1/2) + 500, den = sqrt(1 + 10^6), s = 0.50070..., shade = floor(s * 255 + 0.5) = 128
    s = (math.sqrt(0.5) + 500.0) / math.sqrt(1.0 + 1e6)
    assert math.floor(s * 255.0 + 0.5) == 128 and r["shades"][0, 1] == 128
    # the last row has no pixel below it and the last column none to its right: q = 0 there, p = 0 here -> s = sqrt(1/2) -> 180
    assert r["shades"][3, 15] == 180 and r["shades"][0, 15] == 180
    # paint: grey 200 under shade 128 at weight 96 -> (200 * 159 + 128 * 96 + 127) / 255 = 173; X = 2 is a contour pixel: then
    # (173 * 145 + 60 * 110 + 127) / 255 = 124 for red; X = 5 an index contour: weight 200
    img = np.full((4, 16, 4), 200, np.uint8)
    img[..., 3] = 17
    R.paint(img, r, c.opt)
    assert (200 * 159 + 128 * 96 + 127) // 255 == 173 and tuple(img[0, 1]) == (173, 173, 173, 17)
    assert tuple(img[0, 2]) == ((173 * 145 + 60 * 110 + 127) // 255, (173 * 145 + 40 * 110 + 127) // 255, (173 * 145 + 20 * 110 + 127) // 255, 17)
    assert tuple(img[0, 5]) == ((173 * 55 + 60 * 200 + 127) // 255, (173 * 55 + 40 * 200 + 127) // 255, (173 * 55 + 20 * 200 + 127) // 255, 17)
    assert (img[..., 3] == 17).all()
    summ = R.summary(r)
    assert (summ["n_height"], summ["n_contour"], summ["n_major"]) == (64, 24, 12) and summ["z_min"] == 0.0 and abs(summ["z_max"] - 15000.0) < 1e-8
    # all weights 0: the image stays as it is
    c0 = next(x for x in RC.all_cases() if x.name == "all weights 0")
    base = np.random.default_rng(1).integers(0, 256, size=(33, 65, 4)).astype(np.uint8)
    assert np.array_equal(R.paint(base.copy(), RC.checked(c0), c0.opt), base)


@pytest.mark.parametrize("mutant", sorted(MUTANTS), ids=str)
def test_one_rule_changed_changes_a_case_of_its_family(mutant):
    family = RC.by_family(MUTANTS[mutant])
    assert family
    changed = []
    for c in family:
        r, m = RC.checked(c), RC.restate(c, mutant=mutant)
        if any(not np.array_equal(r[k], m[k]) for k in ("bytes", "shades", "heights")):
            changed.append(c.name)
    assert changed, (mutant, [c.name for c in family])
