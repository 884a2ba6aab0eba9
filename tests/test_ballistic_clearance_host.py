"""Ballistic clearance without a GPU: the structs' layout against the header (a compiled C99 program), the exported symbols, the
library's defaults and every refusal of the options check, the cases' own assertions on the restatement
(tests/ballistic_clearance_ref.py), the restatement against itself with one rule changed at a time, and the rule's steps of
csrc/smh_ballistics.h compiled into a stand-alone program (tests/ballistic_clearance_rule_check.cpp, with -fsanitize=address,undefined
where the host compiler links it) against the restatement, bit for bit."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ballistic_clearance_cases as K
import ballistic_clearance_ref as R
import ballistics_ref as B
from test_ballistics_host import _weapon_struct, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "squad-mortar-helper_amd", "csrc")
SYMBOLS = ("smhv_ballistic_clearance_defaults", "smhv_ballistic_clearance_check", "smhv_batch_ballistic_clearance", "smhv_batch_read_ballistic_clearance",
           "smhv_batch_ballistic_clearance_ptr", "smhv_ballistic_clearance_lines", "smhv_batch_ballistic_clearance_map", "smhv_batch_read_ballistic_clearance_map",
           "smhv_batch_ballistic_clearance_map_ptr", "smhv_ballistic_clearance_map")
ARC_FIELDS = ("status", "first_blocked", "n_blocked", "bal", "min_at")


def hold_dir(got, want, ctx):
    """A smhv_ballistic_clearance_dir (ctypes) against the restatement's record of a direction (None: no verdict, all zeros)."""
    if want is None:
        assert bytes(got) == bytes(96), (ctx, "no verdict leaves a record of zeros")
        return
    for a in (B.HIGH, B.LOW):
        g, w = got.arc[a], want["arc"][a]
        assert tuple(getattr(g, f) for f in ARC_FIELDS) == tuple(w[f] for f in ARC_FIELDS) and g.reserved == 0, (ctx, a, [getattr(g, f) for f in ARC_FIELDS], w)
        assert same_bits(g.min_margin, w["min_margin"]), (ctx, a, g.min_margin, w["min_margin"])
    assert same_bits(got.meters, want["meters"]) and same_bits(got.alt_delta, want["alt_delta"]), (ctx, got.meters, got.alt_delta, want)
    assert (got.los_blocked, got.valid, got.choice, got.reserved) == (want["los_blocked"], 1, want["choice"], 0), (ctx, got.los_blocked, got.valid, got.choice, want)


def test_struct_layouts_and_constants_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    fields = {"smhv_ballistic_clearance_options": (L.BallisticClearanceOptionsStruct, 80), "smhv_arc_clearance": (L.ArcClearance, 32),
              "smhv_ballistic_clearance_dir": (L.BallisticClearanceDir, 96), "smhv_ballistic_clearance": (L.BallisticClearance, 192),
              "smhv_ballistic_clearance_result": (L.BallisticClearanceResult, 16 + 192 * L.MAX_LINES),
              "smhv_ballistic_clearance_map_result": (L.BallisticClearanceMapResult, 64), "smhv_ballistic_clearance_planes": (L.BallisticClearancePlanes, 16)}
    body = "".join('  Z(%s);\n' % t + "".join('  O(%s, %s);\n' % (t, f) for f, _ in cls._fields_) for t, (cls, _) in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   '#define Z(t) printf(#t " %zu\\n", sizeof(t))\n'
                   'int main(void) {\n' + body +
                   '  printf("consts %u %u %u %u %u %u %u %u %u\\n", SMHV_BCLR_PAINT, SMHV_BCLR_BYTES, SMHV_BCLR_MARGIN, SMHV_BCLR_NONE, SMHV_BCLR_OUT_OF_RANGE,\n'
                   '         SMHV_BCLR_UNUSABLE, SMHV_BCLR_CLEAR, SMHV_BCLR_BLOCKED, SMHV_BCLR_LOS);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("consts") else ("consts", ln[7:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for t, (cls, size) in fields.items():
        assert int(got[t]) == C.sizeof(cls) == size, t               # the sizes the header states
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (t, f)]) == getattr(cls, f).offset, (t, f)
    # the offsets the header states
    D, O, M = L.BallisticClearanceDir, L.BallisticClearanceOptionsStruct, L.BallisticClearanceMapResult
    assert (L.ArcClearance.bal.offset, L.ArcClearance.min_margin.offset, D.meters.offset, D.los_blocked.offset, D.valid.offset, D.choice.offset) == (12, 16, 64, 80, 84, 88)
    assert (O.origin.offset, O.margin_m.offset, O.pal.offset, O.switch_arc.offset, O.los.offset, O.reserved.offset) == (24, 32, 40, 56, 60, 64)
    assert (M.own.offset, M.other.offset, M.los_blocked.offset, M.switch_arc.offset, L.BallisticClearanceResult.line.offset) == (16, 32, 48, 52, 16)
    assert [int(v) for v in got["consts"].split()] == [L.BCLR_PAINT, L.BCLR_BYTES, L.BCLR_MARGIN, L.BCLR_NONE, L.BCLR_OUT_OF_RANGE, L.BCLR_UNUSABLE, L.BCLR_CLEAR,
                                                        L.BCLR_BLOCKED, L.BCLR_LOS]
    assert (R.C_NONE, R.C_OUT_OF_RANGE, R.C_UNUSABLE, R.C_CLEAR, R.C_BLOCKED, R.C_LOS) == (0, 1, 2, 3, 4, 0x80)
    assert (R.S_OUT_OF_RANGE, R.S_CLEAR, R.S_BLOCKED) == (L.CLEAR_OUT_OF_RANGE, L.CLEAR_CLEAR, L.CLEAR_BLOCKED) and R.MAX_SAMPLES == L.CLEAR_MAX_SAMPLES


def test_symbols_defaults_and_the_python_options(built):
    """Host-only entry points load and answer without a device."""
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in L.SIGNATURES, name
    o = L.BallisticClearanceOptionsStruct()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    assert lib.smhv_ballistic_clearance_defaults(C.byref(o)) == 0 and lib.smhv_ballistic_clearance_defaults(None) == L.E_INVALID
    assert (o.size, o.flags, o.samples, o.origin_mode, o.line, o.reserved0, tuple(o.origin), o.margin_m, tuple(o.reserved)) == (80, L.BCLR_PAINT, 64, 0, 0, 0, (0.0, 0.0), 0.0,
                                                                                                                                 (0, 0, 0, 0))
    assert [tuple(p) for p in o.pal] == R.DEFAULT_PALETTE["pal"] and tuple(o.switch_arc) == R.DEFAULT_PALETTE["switch_arc"] and tuple(o.los) == R.DEFAULT_PALETTE["los"]
    assert R.DEFAULT_PALETTE == dict(pal=[(0, 0, 0, 0)] * 3 + [(230, 40, 40, 110)], switch_arc=(240, 190, 40, 110), los=(0, 0, 0, 70))
    assert bytes(smh.BallisticClearanceOptions().struct()) == bytes(o) and lib.smhv_ballistic_clearance_check(C.byref(o)) == 0
    p = smh.BallisticClearanceOptions(samples=33, margin_m=2.5, origin=("p1", 3), paint=False, bytes=True, margin=True,
                                      palette=dict(pal=[(k, 2, 3, 4) for k in range(4)], switch_arc=(9, 8, 7, 6), los=(1, 2, 3, 4))).struct()
    assert (p.flags, p.samples, p.margin_m, p.origin_mode, p.line) == (L.BCLR_BYTES | L.BCLR_MARGIN, 33, 2.5, L.REACH_ORIGIN_LINE_P1, 3)
    assert (tuple(p.pal[3]), tuple(p.switch_arc), tuple(p.los)) == ((3, 2, 3, 4), (9, 8, 7, 6), (1, 2, 3, 4)) and lib.smhv_ballistic_clearance_check(C.byref(p)) == 0


def bad_options(good):
    """Every smhv_ballistic_clearance_options the check refuses, made from a good one (a callable that returns a fresh struct)."""
    from squad_mortar_helper_amd import _lib as L
    nan, inf = math.nan, math.inf

    def options(**kw):
        o = good()
        for k, v in kw.items():
            if k.startswith("reserved_"):
                o.reserved[int(k[9:])] = v
            else:
                setattr(o, k, v)
        return o
    return [options(size=76), options(size=84), options(size=0), options(flags=8), options(flags=0x80000007), options(samples=0), options(samples=257),
            options(samples=0xFFFFFFFF), options(margin_m=-1.0), options(margin_m=-5e-324), options(margin_m=nan), options(margin_m=inf), options(margin_m=-inf),
            options(origin_mode=3), options(origin_mode=0xFFFFFFFF), options(origin_mode=L.REACH_ORIGIN_LINE_P0, line=32),
            options(origin_mode=L.REACH_ORIGIN_LINE_P1, line=0xFFFFFFFF), options(reserved0=1), options(reserved_0=1), options(reserved_1=7), options(reserved_2=1),
            options(reserved_3=0x80000000)]


def test_the_options_check_refuses_exactly_the_list(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    good = smh.BallisticClearanceOptions(samples=64, margin_m=1.0, bytes=True, margin=True).struct
    for i, o in enumerate(bad_options(good)):
        assert lib.smhv_ballistic_clearance_check(C.byref(o)) == L.E_INVALID, i
    assert lib.smhv_ballistic_clearance_check(None) == L.E_INVALID

    def ok(**kw):
        o = good()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    fine = [ok(), ok(samples=1), ok(samples=256), ok(margin_m=0.0), ok(margin_m=-0.0), ok(margin_m=1e300), ok(flags=0), ok(flags=7), ok(origin_mode=L.REACH_ORIGIN_POINT, line=999),
            ok(origin_mode=L.REACH_ORIGIN_LINE_P1, line=31)]
    for i, o in enumerate(fine):
        assert lib.smhv_ballistic_clearance_check(C.byref(o)) == 0, i
    fine[0].origin[0] = math.nan                                  # (an origin that is not finite is "no origin", not an error)
    assert lib.smhv_ballistic_clearance_check(C.byref(fine[0])) == 0


@pytest.mark.parametrize("c", K.line_cases(), ids=lambda c: c.name)
def test_every_line_case_holds_its_purpose(c):
    recs = K.checked_lines(c)
    assert len(recs) == len(c.lines)
    for pair in recs:
        for d in pair:
            if d is not None:                                      # the high arc lies above the low arc: it is blocked no more often
                assert d["arc"][B.HIGH]["n_blocked"] <= d["arc"][B.LOW]["n_blocked"] or d["arc"][B.HIGH]["status"] == R.S_OUT_OF_RANGE, (c.name, d)


@pytest.mark.parametrize("c", K.map_cases(), ids=lambda c: c.name)
def test_every_map_case_holds_its_purpose(c):
    r = K.checked_map(c)
    s = R.summary(r)
    own = r["bytes"] & 7
    assert sum(s["own"]) == sum(s["other"]) == int((own != 0).sum()) and s["own"][0] == s["other"][0] and s["switch_arc"] <= s["other"][2]


def test_the_cases_cover_what_the_issue_names():
    lines, maps = K.line_cases(), K.map_cases()
    names = " | ".join(c.name for c in lines)
    for what in ("low blocked, high clear, laid low", "low blocked, high clear, laid high", "low blocked, high unusable", "high unusable, low clear", "disc == 0.0",
                 "target far below", "no arc", "d == 0", "S == 1", "an end outside", "the scales branch", "a margin of", "m == margin_m", "ties of m"):
        assert what in names, what
    assert {c.samples for c in lines if c.name.startswith("32 lines")} == set(K.SAMPLES) == {c.samples for c in maps if "panned" in c.name}
    assert set(K.SAMPLES) == {1, 2, K.KC, K.KC + 1, K.KC + 2, 64, 65, 66, 256}
    dense = [c for c in maps if c.show == K.ALL]
    assert {c.window for c in dense} == {(130, 33), (65, 17)} and {id(c.hm[0]) for c in dense} >= {id(K.CC.country_map()[0]), id(K.CC.random_map()[0])}
    assert any(c.viewport is None for c in dense) and any(c.viewport is not None and c.viewport[0] != c.viewport[1] for c in dense)
    assert any(c.name == "origin outside its rectangle" for c in maps) and {c.weapon.arc for c in dense} == {B.HIGH, B.LOW}
    # every dense case that shows everything has every class of both arcs, the LOS bit and a switch pixel, each on both sides of a tile edge
    # (in two tiles that share an edge); of the sample counts only S = 1, which has no sample to block anything, shows less
    for c in dense:
        f = K.features(K.checked_map(c))
        assert all(f[w][0] >= 1 and f[w][2] for w in K.ALL), (c.name, f)
    assert [c.samples for c in maps if "panned" in c.name and c.show != K.ALL] == [1] and len(dense) >= 14
    assert set(R.MUTANTS) == {m for c in lines + maps for m in c.families}


def _answer_lines(c, mut):
    return repr(K.restate_lines(c, mut))


def _answer_map(c, mut):
    r = K.restate_map(c, mut)
    return (r["bytes"].tobytes(), r["margin"].tobytes(), repr(R.summary(r)))


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_changed_rule_is_told_apart_by_every_case_named_for_it(mut):
    lines = [c for c in K.line_cases() if mut in c.families]
    maps = [c for c in K.map_cases() if mut in c.families]
    assert lines or maps, mut
    for c in lines:
        assert _answer_lines(c, (mut,)) != _answer_lines(c, ()), (mut, c.name, "names the switch and does not notice it")
    for c in maps:
        assert _answer_map(c, (mut,)) != _answer_map(c, ()), (mut, c.name, "names the switch and does not notice it")
    if mut in ("class_precedence", "los_not_oor"):                # the map's alone
        assert not lines and len(maps) >= 10
    if mut == "margin_le":                                        # the lines' alone: no pixel's m equals a margin exactly
        assert not maps
    if mut == "choice_no_bal":                                    # ... and the named answer itself: the rocket under the hill would be told to fire high
        c = next(c for c in lines if c.name == "low blocked, high unusable")
        assert K.restate_lines(c, (mut,))[0][0]["choice"] == 1 + B.HIGH and K.restate_lines(c)[0][0]["choice"] == 0


def _jobs():
    """Directions for the stand-alone program: (weapon, d, alt, S, margin, z [S - 1]).  Random terrain around the arcs, the exact ties, and
    what a heightmap cannot give: a terrain of NaN (no m: never the minimum) and of infinities."""
    rng = np.random.default_rng(23)
    jobs = []
    for w in (K.MORTAR, K.MORTAR_LOW, K.ROCKET, K.ROCKET_HIGH, K.THROWER, K.THROWER_LOW, K.EXACT, K.LOB_LOW):
        reach = w.velocity * w.velocity / w.gravity
        for S in K.SAMPLES:
            for frac, alt in ((0.5, 0.0), (0.9, 12.5), (0.3, -40.0), (1.2, 0.0), (0.0, 0.0)):
                d = reach * frac
                z = rng.uniform(-30.0, 0.2 * max(d, 1.0), size=S - 1)
                jobs.append((w, d, alt, S, float(rng.choice([0.0, 0.0, 3.0])), z))
    for S in (2, 64, 256):
        jobs.append((K.EXACT, 128.0, 0.0, S, 0.0, np.zeros(S - 1)))  # disc == 0, ties of m between k and S - k
    z = np.zeros(63)
    z[[0, 5, 62]] = np.nan
    jobs.append((K.EXACT, 128.0, 0.0, 64, 0.0, z.copy()))            # NaN at the tying ends: the minimum moves inward, to the lowest k of the next tie
    jobs.append((K.MORTAR, 500.0, 0.0, 64, 0.0, np.full(63, np.nan)))  # nothing ever replaces best
    z[:] = 1.0
    z[[7, 9]] = np.inf
    jobs.append((K.MORTAR_LOW, 500.0, 0.0, 64, 0.0, z.copy()))       # m = -inf twice: the first wins
    z[[7, 9]] = -np.inf
    jobs.append((K.MORTAR_LOW, 500.0, 0.0, 64, 0.0, z.copy()))       # m = +inf never replaces the starting +inf
    return jobs


def test_the_rule_header_as_a_stand_alone_program(built, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ballistic_clearance_rule_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "ballistic_clearance_rule_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    jobs = _jobs()
    refused = _weapon_struct(K.ROCKET)
    refused.elev_min = 41.0
    blob = b"".join(bytes(_weapon_struct(w)) + struct.pack("<dddII", d, alt, margin, S, 0) + np.asarray(z, np.float64).tobytes() for w, d, alt, S, margin, z in jobs)
    blob += bytes(refused) + struct.pack("<dddII", 100.0, 0.0, 0.0, 2, 0) + struct.pack("<d", 0.0)
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(jobs) + 1) + blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok: %d jobs" % (len(jobs) + 1)), (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    from squad_mortar_helper_amd import _lib as L
    got = (tmp_path / "out.bin").read_bytes()
    assert len(got) == 96 * (len(jobs) + 1)
    seen = set()
    for i, (w, d, alt, S, margin, z) in enumerate(jobs):
        want = R.march(w, d, alt, S, margin, z)
        hold_dir(L.BallisticClearanceDir.from_buffer_copy(got, 96 * i), want, (i, w, d, alt, S, margin))
        seen |= {(a["status"], bool(a["bal"])) for a in want["arc"]}
    assert seen == {(s, b) for s in (R.S_OUT_OF_RANGE, R.S_CLEAR, R.S_BLOCKED) for b in (False, True)} - {(R.S_OUT_OF_RANGE, False)}
    assert got[96 * len(jobs):] == bytes(96)                     # the refused weapon: nothing computed
    tie = R.march(K.EXACT, 128.0, 0.0, 64, 0.0, np.zeros(63))
    assert tie["arc"][0] == tie["arc"][1] and tie["arc"][0]["min_at"] == 1
    nan_ends = R.march(*jobs[-4][:5], jobs[-4][5])
    assert nan_ends["arc"][0]["min_at"] == 2 and R.march(*jobs[-3][:5], jobs[-3][5])["arc"][0] == dict(status=R.S_CLEAR, first_blocked=64, n_blocked=0, bal=0, min_margin=0.0, min_at=0)
    assert R.march(*jobs[-2][:5], jobs[-2][5])["arc"][B.LOW]["min_at"] == 8 and R.march(*jobs[-1][:5], jobs[-1][5])["arc"][B.LOW]["min_at"] not in (8, 10)
