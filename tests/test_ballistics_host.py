"""Ballistics without a GPU: the structs' layout against the header, the exported symbols, the library's defaults and what
smhv_weapon_check refuses, the default weapon's V^2 and V^4 against the firing solutions' constants, the cases' own assertions on the
restatement (tests/ballistics_ref.py), the restatement against itself with one rule changed at a time, smhv_ballistic_solve against the
restatement, and csrc/smh_ballistics.h compiled into a stand-alone program (tests/ballistics_rule_check.cpp, with
-fsanitize=address,undefined where the host compiler links it): everything bit-equal but the elevations, which get 4 ulps."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ballistics_cases as BC
import ballistics_ref as B
import firing_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "squad-mortar-helper_amd", "csrc")
SYMBOLS = ("smhv_weapon_defaults", "smhv_weapon_check", "smhv_weapon_thresholds", "smhv_ballistic_defaults", "smhv_ballistic_solve", "smhv_batch_ballistics",
           "smhv_batch_read_ballistics", "smhv_batch_ballistics_ptr", "smhv_ballistic_lines", "smhv_batch_ballistic_map", "smhv_batch_read_ballistic_map",
           "smhv_batch_ballistic_map_ptr", "smhv_ballistic_map")
EXACT = ("tof", "apex", "fall", "along", "status", "band")
ULPS = 4                                                          # what test_firing_edges_gpu.py gives mortar_mils against glibc's atan


def _weapon_struct(w):
    import squad_mortar_helper_amd as smh
    return smh.Weapon(velocity=w.velocity, gravity=w.gravity, arc=("high", "low")[w.arc], unit=("mils6400", "mils6000", "degrees")[w.unit],
                      elev_min=w.elev_min, elev_max=w.elev_max, range_min=w.range_min, dispersion=w.dispersion).struct()


def same_bits(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or struct.pack("<d", a) == struct.pack("<d", b)


def hold_solution(got, want, ctx, source=0):
    """A smhv_ballistic_solution (ctypes) against solve()'s dict: bit-equal but for the elevations."""
    assert same_bits(got.meters, want["meters"]) and same_bits(got.alt_delta, want["alt_delta"]) and same_bits(got.cross, want["cross"]), ctx
    assert (got.source, got.reserved) == (source, 0), ctx
    for i in (B.HIGH, B.LOW):
        a, w = got.arc[i], want["arc"][i]
        for f in ("tof", "apex", "fall", "along"):
            assert same_bits(getattr(a, f), w[f]), (ctx, i, f, getattr(a, f), float(w[f]))
        assert (a.status, a.band) == (int(w["status"]), int(w["band"])), (ctx, i, a.status, a.band, int(w["status"]), int(w["band"]))
        assert B.ulps(a.elevation, w["elevation"]) <= ULPS, (ctx, i, a.elevation, float(w["elevation"]))


def test_struct_layouts_and_constants_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    fields = {"smhv_weapon": (L.WeaponStruct, 80), "smhv_weapon_rule": (L.WeaponRule, 136), "smhv_ballistic_arc": (L.BallisticArc, 48),
              "smhv_ballistic_solution": (L.BallisticSolution, 128), "smhv_ballistic": (L.Ballistic, 256), "smhv_ballistic_result": (L.BallisticResult, 16 + 256 * L.MAX_LINES),
              "smhv_ballistic_options": (L.BallisticOptionsStruct, 96), "smhv_ballistic_map_result": (L.BallisticMapResult, 96),
              "smhv_ballistic_planes": (L.BallisticPlanes, 16)}
    body = "".join('  Z(%s);\n' % t + "".join('  O(%s, %s);\n' % (t, f) for f, _ in cls._fields_) for t, (cls, _) in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   '#define Z(t) printf(#t " %zu\\n", sizeof(t))\n'
                   'int main(void) {\n' + body +
                   '  printf("consts %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\\n", SMHV_ARC_HIGH, SMHV_ARC_LOW, SMHV_ANGLE_MILS6400, SMHV_ANGLE_MILS6000,\n'
                   '         SMHV_ANGLE_DEGREES, SMHV_BAL_OUT_OF_RANGE, SMHV_BAL_BELOW_MIN_RANGE, SMHV_BAL_ELEV_LOW, SMHV_BAL_ELEV_HIGH, SMHV_BMAP_PAINT, SMHV_BMAP_CLASSES,\n'
                   '         SMHV_BMAP_TOF, SMHV_BMAP_OUT_OF_RANGE, SMHV_BMAP_BELOW_MIN_RANGE, SMHV_BMAP_ELEV_LOW, SMHV_BMAP_ELEV_HIGH, SMHV_BMAP_BAND0, SMHV_BMAP_ISO);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("consts") else ("consts", ln[7:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for t, (cls, size) in fields.items():
        assert int(got[t]) == C.sizeof(cls) == size, t               # the sizes the header states
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (t, f)]) == getattr(cls, f).offset, (t, f)
    # the offsets the header states for the record
    assert (L.BallisticArc.status.offset, L.BallisticSolution.arc.offset, L.BallisticSolution.source.offset, L.BallisticResult.line.offset) == (40, 32, 24, 16)
    assert (L.BallisticMapResult.iso.offset, L.BallisticMapResult.tof_min.offset, L.BallisticOptionsStruct.pal.offset, L.WeaponRule.band.offset) == (64, 72, 32, 48)
    assert [int(v) for v in got["consts"].split()] == [L.ARC_HIGH, L.ARC_LOW, L.ANGLE_MILS6400, L.ANGLE_MILS6000, L.ANGLE_DEGREES, L.BAL_OUT_OF_RANGE,
                                                        L.BAL_BELOW_MIN_RANGE, L.BAL_ELEV_LOW, L.BAL_ELEV_HIGH, L.BMAP_PAINT, L.BMAP_CLASSES, L.BMAP_TOF,
                                                        L.BMAP_OUT_OF_RANGE, L.BMAP_BELOW_MIN_RANGE, L.BMAP_ELEV_LOW, L.BMAP_ELEV_HIGH, L.BMAP_BAND0, L.BMAP_ISO]
    assert (B.HIGH, B.LOW, B.MILS6400, B.MILS6000, B.DEGREES, B.OUT_OF_RANGE, B.BELOW_MIN_RANGE, B.ELEV_LOW, B.ELEV_HIGH, B.C_OUT_OF_RANGE, B.C_BELOW_MIN_RANGE,
            B.C_ELEV_LOW, B.C_ELEV_HIGH, B.C_BAND0, B.C_ISO) == (0, 1, 0, 1, 2, 1, 2, 4, 8, 1, 2, 3, 4, 5, 0x80)


def test_symbols_defaults_and_the_python_options(built):
    """Host-only entry points load and answer without a device."""
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name
    w = L.WeaponStruct()
    C.memset(C.byref(w), 0xA5, C.sizeof(w))
    assert lib.smhv_weapon_defaults(C.byref(w)) == 0 and lib.smhv_weapon_defaults(None) == L.E_INVALID
    d = B.Weapon()
    assert (w.size, w.arc, w.unit, w.reserved0, tuple(w.reserved)) == (80, B.HIGH, B.MILS6400, 0, (0, 0, 0, 0))
    assert (w.velocity, w.gravity, w.elev_min, w.elev_max, w.range_min, w.dispersion) == (FR.V, FR.G, d.elev_min, d.elev_max, 0.0, 0.0) == (d.velocity, d.gravity, 0.0, 1600.0, 0.0, 0.0)
    assert bytes(smh.Weapon().struct()) == bytes(w) and lib.smhv_weapon_check(C.byref(w)) == 0
    o = L.BallisticOptionsStruct()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    assert lib.smhv_ballistic_defaults(C.byref(o)) == 0 and lib.smhv_ballistic_defaults(None) == L.E_INVALID
    assert (o.size, o.flags, o.origin_mode, o.line, tuple(o.origin), o.iso_s, tuple(o.reserved)) == (96, L.BMAP_PAINT, 0, 0, (0.0, 0.0), 0.0, (0, 0, 0))
    assert [tuple(p) for p in o.pal] == B.DEFAULT_PALETTE["pal"] and tuple(o.iso) == B.DEFAULT_PALETTE["iso"]
    assert bytes(smh.BallisticOptions().struct()) == bytes(o)
    p = smh.BallisticOptions(origin=("p1", 3), iso_s=2.5, paint=False, classes=True, tof=True, palette=dict(pal=[(k, 2, 3, 4) for k in range(12)], iso=(9, 8, 7, 6))).struct()
    assert (p.flags, p.origin_mode, p.line, p.iso_s, tuple(p.pal[11]), tuple(p.iso)) == (L.BMAP_CLASSES | L.BMAP_TOF, L.REACH_ORIGIN_LINE_P1, 3, 2.5, (11, 2, 3, 4), (9, 8, 7, 6))


def test_the_default_weapon_reproduces_the_firing_constants(built):
    """V^2 and V^4 derived from the velocity are SMH_MORTAR_V2 / SMH_MORTAR_V4 as tests/firing_ref.py reads them, bit for bit; and the
    restatement's, and csrc/smh_firing.h's literals."""
    import squad_mortar_helper_amd as smh
    k = smh.Weapon().thresholds()
    r = B.rule(B.Weapon())
    assert same_bits(k.v2, FR.V2) and same_bits(k.v4, FR.V4) and same_bits(r["v2"], FR.V2) and same_bits(r["v4"], FR.V4)
    text = open(os.path.join(CSRC, "smh_firing.h")).read()
    assert "#define SMH_MORTAR_V2 %s\n" % FR.V2.hex() in text and "#define SMH_MORTAR_V4 %s\n" % FR.V4.hex() in text
    assert (k.v, k.g, k.t_min, k.t_max, k.t_disp, k.range_min, k.unit_deg, k.arc, k.unit) == (FR.V, FR.G, 0.0, math.inf, 0.0, 0.0, 360.0 / 6400.0, 0, 0)


@pytest.mark.parametrize("w", [BC.MORTAR, BC.ROCKET, BC.TUBE, BC.BINARY], ids=["mortar", "rocket", "tube", "binary"])
def test_thresholds_equal_the_restatement(built, w):
    from squad_mortar_helper_amd import _lib as L
    ws, k, r = _weapon_struct(w), L.WeaponRule(), B.rule(w)
    assert L.load().smhv_weapon_thresholds(C.byref(ws), C.byref(k)) == 0
    for f in ("v", "g", "v2", "v4", "t_min", "t_max", "t_disp", "range_min", "unit_deg"):
        assert same_bits(getattr(k, f), r[f]), f
    assert all(same_bits(a, b) for a, b in zip(k.band, r["band"])) and (k.arc, k.unit) == (w.arc, w.unit)
    assert list(k.band) == sorted(k.band) and k.t_min <= k.band[0] and k.band[6] <= k.t_max


def test_weapon_check_refuses_exactly_the_list(built):
    from squad_mortar_helper_amd import _lib as L
    lib = L.load()
    nan, inf = math.nan, math.inf

    def weapon(**kw):
        w = _weapon_struct(BC.ROCKET)
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    bad = [weapon(size=76), weapon(size=84), weapon(size=0), weapon(arc=2), weapon(arc=0xFFFFFFFF), weapon(unit=3), weapon(velocity=0.0), weapon(velocity=-1.0),
           weapon(velocity=nan), weapon(velocity=inf), weapon(gravity=0.0), weapon(gravity=-9.8), weapon(gravity=nan), weapon(gravity=inf), weapon(elev_min=nan),
           weapon(elev_max=nan), weapon(elev_min=-inf), weapon(elev_max=inf), weapon(elev_min=41.0), weapon(elev_max=4.0), weapon(range_min=-1.0),
           weapon(range_min=nan), weapon(range_min=inf), weapon(dispersion=-0.001), weapon(dispersion=nan), weapon(dispersion=inf)]
    rule, sol = L.WeaponRule(), L.BallisticSolution()
    C.memset(C.byref(rule), 0x5A, C.sizeof(rule))
    C.memset(C.byref(sol), 0x5A, C.sizeof(sol))
    for i, w in enumerate(bad):
        assert lib.smhv_weapon_check(C.byref(w)) == L.E_INVALID, i
        assert lib.smhv_weapon_thresholds(C.byref(w), C.byref(rule)) == L.E_INVALID and lib.smhv_ballistic_solve(C.byref(w), 500.0, 0.0, C.byref(sol)) == L.E_INVALID, i
    assert bytes(rule) == b"\x5a" * 136 and bytes(sol) == b"\x5a" * 128
    good = [weapon(), weapon(elev_min=40.0), weapon(elev_min=-3000.0, elev_max=3000.0), weapon(range_min=0.0, dispersion=0.0), weapon(arc=0, unit=0),
            weapon(velocity=5e-324), weapon(gravity=1e300), weapon(reserved0=7)]
    for i, w in enumerate(good):
        assert lib.smhv_weapon_check(C.byref(w)) == 0, i
    assert lib.smhv_weapon_check(None) == L.E_INVALID and lib.smhv_weapon_thresholds(C.byref(good[0]), None) == L.E_INVALID
    assert lib.smhv_ballistic_solve(C.byref(good[0]), 500.0, 0.0, None) == L.E_INVALID
    import squad_mortar_helper_amd as smh
    with pytest.raises(smh.VisionError) as ei:
        smh.Weapon(elev_min=2.0, elev_max=1.0).check()
    assert ei.value.code == L.E_INVALID
    smh.Weapon().check()


@pytest.mark.parametrize("p", BC.points(), ids=lambda p: p.name)
def test_every_point_holds_its_purpose_and_the_host_solves_it(built, p):
    """The point's own check on the restatement (and that no elevation lies within 4 ulps of a limit of the mount), then
    smhv_ballistic_solve against the restatement."""
    from squad_mortar_helper_amd import _lib as L
    want = BC.checked_point(p)
    ws, got = _weapon_struct(p.weapon), L.BallisticSolution()
    assert L.load().smhv_ballistic_solve(C.byref(ws), p.m, p.alt, C.byref(got)) == 0
    hold_solution(got, want, p.name)


@pytest.mark.parametrize("c", BC.maps(), ids=lambda c: c.name)
def test_every_map_holds_its_purpose(c):
    r = BC.checked_map(c)
    s = B.summary(r)
    assert sum(s["count"]) + int(((r["classes"] & 0x7F) == 0).sum()) == r["classes"].size and s["n_tof"] <= sum(s["count"][4:])
    if s["n_tof"]:
        assert 0.0 < s["tof_min"] <= s["tof_max"] < math.inf


def test_the_cases_cover_what_the_issue_names():
    pts, maps = BC.points(), BC.maps()
    hits = BC.threshold_hits()
    assert len(hits) == 18 and {h[3] for h in hits} == {-2, -1, 0, 1, 2, 3, 4, 5, 6}                  # both limits and seven band thresholds, of two weapons
    assert sum(1 for h in hits if h[4] == 0.0) >= 4                                                    # ... some on flat ground: those run on the device too
    assert {p.weapon.unit for p in pts} == {B.MILS6400, B.MILS6000, B.DEGREES} and {p.weapon.arc for p in pts} == {B.HIGH, B.LOW}
    assert {(c.weapon.arc, c.weapon.unit) for c in maps} >= {(B.LOW, B.DEGREES), (B.HIGH, B.MILS6000), (B.HIGH, B.MILS6400)}
    assert {c.window for c in maps} >= {(1, 1), (63, 15), (64, 16), (65, 17), (130, 33)}
    assert any(p.m == 0.0 for p in pts) and any(p.m != p.m for p in pts) and any(p.alt != p.alt for p in pts) and any(math.isinf(p.m) for p in pts)
    assert any(p.alt == math.inf for p in pts) and any(p.alt == -math.inf for p in pts)


def _answer_point(p, mut):
    s = B.solve(p.weapon, p.m, p.alt, mut)
    return [repr(float(s["cross"]))] + [repr(float(a[f])) for a in s["arc"] for f in ("elevation",) + EXACT]


def _answer_map(c, mut):
    r = BC.restate_map(c, mut)
    return (r["classes"].tobytes(), r["tof"].tobytes(), repr(B.summary(r)))


@pytest.mark.parametrize("mut", B.MUTANTS)
def test_every_changed_rule_is_told_apart_by_its_family(mut):
    fam = BC.FAMILY_OF[mut]
    pts = [p for p in BC.points() if fam in p.families]
    maps = [c for c in BC.maps() if fam in c.families]
    assert pts or maps, fam
    told = [p.name for p in pts if _answer_point(p, (mut,)) != _answer_point(p, ())] + [c.name for c in maps if _answer_map(c, (mut,)) != _answer_map(c, ())]
    assert told, (mut, fam, "no case of the family notices")
    # ... and both kinds notice where both can: the isochrone is the map's alone, the apex the solution's alone, and a T exactly on a
    # limit is a point found by search -- no pixel of a window lands on one
    if mut != "iso_left":
        assert any(n in told for n in (p.name for p in pts)), (mut, "no point notices")
    if mut not in ("apex_no_clamp", "limit_gt"):
        assert any(n in told for n in (c.name for c in maps)), (mut, "no map notices")


def test_the_header_as_a_stand_alone_program(built, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ballistics_rule_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "ballistics_rule_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    pts = BC.points()
    refused = _weapon_struct(BC.ROCKET)
    refused.elev_min = 41.0
    blob = b"".join(bytes(_weapon_struct(p.weapon)) + struct.pack("<dd", p.m, p.alt) for p in pts) + bytes(refused) + struct.pack("<dd", 1.0, 0.0)
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(pts) + 1) + blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok: %d jobs" % (len(pts) + 1)), (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    from squad_mortar_helper_amd import _lib as L
    got = (tmp_path / "out.bin").read_bytes()
    assert len(got) == 272 * (len(pts) + 1)
    for i, p in enumerate(pts):
        rec = got[272 * i:272 * (i + 1)]
        assert struct.unpack_from("<II", rec) == (1, 0), p.name
        k, want = L.WeaponRule.from_buffer_copy(rec, 8), B.rule(p.weapon)
        for f in ("v", "g", "v2", "v4", "t_min", "t_max", "t_disp", "range_min", "unit_deg"):
            assert same_bits(getattr(k, f), want[f]), (p.name, f)
        assert all(same_bits(a, b) for a, b in zip(k.band, want["band"])), p.name
        hold_solution(L.BallisticSolution.from_buffer_copy(rec, 144), BC.restate_point(p), p.name)
    assert got[272 * len(pts):] == bytes(272)                    # the refused weapon: nothing computed
