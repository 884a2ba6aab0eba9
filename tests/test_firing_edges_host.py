"""The crafted firing and label cases (tests/firing_edge_cases.py) on the CPU: every case holds its own boundary on the restatement,
every literal label row is what label_ref prints for the restated numbers -- and the cases have teeth: the restatements with one
rule changed at a time give another answer on at least one case of the family named for the rule."""
import inspect
import math

import numpy as np
import pytest

import firing_edge_cases as E
import firing_ref as R
import label_ref as LR

f32 = np.float32


@pytest.mark.parametrize("case", E.cases(), ids=lambda c: "%s: %s" % (c.family, c.name))
def test_every_case_holds_its_boundary_and_prints_its_literal_rows(case):
    wants = E.restate(case)
    case.check(case, wants)
    if case.rows is not None:
        for i, (got, rows) in enumerate(zip(E.label_rows(case, wants), case.rows)):
            assert (got == rows) if rows is not None else (len(got) in (4, 6)), (case, i, got, rows)      # None: prints, rows not typed
            assert all(len(r) <= 16 for r in got)


def test_the_families_and_what_they_hold():
    cases = E.cases()
    count = {f: sum(c.family == f for c in cases) for f in E.FAMILIES}
    lines = {f: sum(len(c.lines) for c in cases if c.family == f) for f in E.FAMILIES}
    print("cases per family:", count, "lines per family:", lines)
    assert all(count[f] >= 4 for f in E.FAMILIES), count
    # the injected meters arrive exactly (the unit lines have length 1 in f64)
    for m in (0.0, 0.5, 2.5, 9.5, 1232.25, math.nextafter(999999.5, 0.0), 999999.5, 5e-324):
        for line in (E.EAST, E.WEST, E.SOUTH, E.NORTH):
            assert R.record_meters(line, m) == m
    # the range limit is where the discriminant changes sign, and the next f64 is V^2 / g
    lo, hi = E.range_limit()
    assert math.nextafter(lo, math.inf) == hi and hi == R.V2 / R.G and 800.0 < R.calc(lo, 0.0) < 800.00001 and math.isnan(R.calc(hi, 0.0))
    assert R.calc(0.0, 0.0) == R.calc(5e-324, 0.0) == R.calc(100.0, -1.95e37) == 1600.0 and math.isnan(R.calc(math.inf, 0.0))
    # the label calls the device test makes: one per distinct (mpx, heightmap, fit, viewport) among the cases that print
    groups = {c.group for c in cases if c.rows is not None}
    assert 15 <= len(groups) <= 32, len(groups)
    # the texel ties reach the per-call label path in every geometry it has: fitted, a viewport that scales, "fit to minimap" off
    ties = [(c.fit, c.viewport is not None) for c in cases if c.family == "ties" and c.rows is not None]
    assert sorted(ties) == [(False, False), (True, False), (True, True)], ties
    assert any(c.rows is not None and c.hm and c.viewport and c.viewport[0] == 0 for c in cases)
    # every kind of row is among the literals: both 16-byte rows, RANGE! on either side, three and four digits of mils, no label
    rows = [r for c in cases if c.rows is not None for rr in c.rows if rr is not None for r in rr]
    for r in (E.PM + b"2147483647m alt", E.PM + b"2147483648m alt", b"<- RANGE!", b"RANGE! ->", b"RANGE!", b"800 mil", b"1600 mil", b"0m", b"999999m",
              b"-> 0" + E.DEG, b"<- 0" + E.DEG, b"0" + E.DEG, b"-> 5" + E.DEG, b"-> 40" + E.DEG, b"<- 271" + E.DEG):
        assert r in rows, r
    assert sum(rr == [] for c in cases if c.rows is not None for rr in c.rows) >= 6


def test_a_case_that_has_left_its_boundary_fails():
    """One ulp on one end point of a tie, and a range one f64 further: the case's own check says so."""
    ties = [c for c in E.cases() if c.name == "every tie, identity geometry"][0]
    moved = E.Case(ties.name, "ties", [tuple(np.nextafter(f32(v), f32(1e9)) for v in ties.lines[0])] + ties.lines[1:], ties.check, mpx=ties.mpx,
                   minimap=ties.minimap, hm=ties.hm)
    with pytest.raises(AssertionError):
        moved.check(moved, E.restate(moved))
    last = [c for c in E.cases() if c.name == "the last range with mils"][0]
    moved = E.Case(last.name, "range", last.lines, last.check, mpx=math.nextafter(last.mpx, 0.0))
    with pytest.raises(AssertionError):
        moved.check(moved, E.restate(moved))
    half = [c for c in E.cases() if c.name == "270.5 exactly: half away from zero is 271"][0]
    moved = E.Case(half.name, "bearings", [E._ray(0.5001)], half.check, mpx=half.mpx)
    with pytest.raises(AssertionError):
        moved.check(moved, E.restate(moved))


# ---- teeth: the restatements with one rule changed at a time (the modules themselves stay as they are) -----------------------------
def _finite_or(f):
    return lambda x: x if not math.isfinite(x) else f(x)


def _wrap_i32(v):
    v = float(v)
    return 0 if v != v or math.isinf(v) else (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _cast_with(rounding):
    def cast(v):
        v = float(v)
        if v != v:
            return 0
        return 2147483647 if v >= 2147483647.0 else -2147483648 if v <= -2147483648.0 else int(rounding(v))
    return cast


def _rewritten(module, name, old, new):
    """A copy of module.name with the text `old` of its source replaced by `new`, living in a copy of the module's globals.
    The copy looks its helpers up in that COPY of the globals, so what is patched into the module afterwards does not reach it:
    a rewritten firing_line goes past E.restate()'s probe of round_f64 and restate() hands back None for the coordinates.
    E.expected() does not read them; a mutant whose verdict needs them has to patch the helper in `ns`, not in the module."""
    src = inspect.getsource(getattr(module, name))
    assert src.count(old) == 1, (name, old)
    ns = dict(vars(module))
    exec(compile(src.replace(old, new), "<%s, mutated>" % name, "exec"), ns)
    return ns[name]


_INSIDE = "0 <= i0 < W and 0 <= j0 < H and 0 <= i1 < W and 0 <= j1 < H"
MUTANTS = {  # name: (module, attribute, the replacement, the family whose edge it moves)
    "round_f64: half to even": (R, "round_f64", lambda: _finite_or(lambda x: float(np.rint(x))), "ties"),
    "round_f64: floor(x + 0.5)": (R, "round_f64", lambda: _finite_or(lambda x: float(math.floor(x + 0.5))), "ties"),
    "inside: < n becomes <= n": (R, "firing_line", lambda: _rewritten(R, "firing_line", _INSIDE, _INSIDE.replace(" < ", " <= ")), "ties"),
    "inside: > -1 on the unrounded coordinate": (R, "firing_line", lambda: _rewritten(
        R, "firing_line", _INSIDE, "ax0 > -1 and i0 < W and ay0 > -1 and j0 < H and ax1 > -1 and i1 < W and ay1 > -1 and j1 < H"), "ties"),
    "as_i32: NaN becomes -1": (R, "as_i32", lambda: (lambda x, orig=R.as_i32: -1 if x != x else orig(x)), "degenerate"),
    "fmt0: half away from zero": (LR, "fmt0", lambda: (lambda v: str(int(math.floor(float(v) + 0.5))).encode("latin-1")), "print"),
    "cast_i32: rounds": (LR, "cast_i32", lambda: _cast_with(lambda v: math.floor(abs(v) + 0.5) * math.copysign(1, v)), "print"),
    "cast_i32: floor": (LR, "cast_i32", lambda: _cast_with(math.floor), "print"),
    "cast_i32: wraps, no saturation": (LR, "cast_i32", lambda: _wrap_i32, "print"),
    "cut-off: <= 999999.5": (LR, "format_label", lambda: _rewritten(LR, "format_label", '< 999999.5:', '<= 999999.5:'), "print"),
    "cut-off: < 1e6": (LR, "format_label", lambda: _rewritten(LR, "format_label", '< 999999.5:', '< 1e6:'), "print"),
    "roundf: half to even": (R, "roundf", lambda: (lambda x: f32(x) if not np.isfinite(f32(x)) else f32(np.rint(f32(x)))), "bearings"),
    "back bearing without its fmod": (R, "bearings_from_degrees", lambda: _rewritten(
        R, "bearings_from_degrees", "bck = F32(np.fmod(roundf(F32(fwd + F32(180.0))), F32(360.0)))", "bck = roundf(F32(fwd + F32(180.0)))"), "bearings"),
    "d < 0: the + 360 dropped": (R, "bearings_from_degrees", lambda: _rewritten(
        R, "bearings_from_degrees", "        if d < F32(0.0):\n            d = F32(d + F32(360.0))\n", ""), "bearings"),
    "forward wrap: fwd without its fmod": (R, "bearings_from_degrees", lambda: _rewritten(
        R, "bearings_from_degrees", "fwd = F32(np.fmod(roundf(d), F32(360.0)))", "fwd = roundf(d)"), "bearings"),
    "arrows: d.x >= 0 becomes d.x > 0": (LR, "format_label", lambda: _rewritten(LR, "format_label", "        if dx >= 0:", "        if dx > 0:"), "print"),
    "block order: d.y < 0 becomes d.y > 0": (LR, "format_label", lambda: _rewritten(LR, "format_label", "(dx == 0 and dy < 0)", "(dx == 0 and dy > 0)"), "print"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_told_apart(mutant, monkeypatch):
    """The family named for the mutant holds a case whose expected output (numbers and rows) the mutant changes."""
    module, attr, make, family = MUTANTS[mutant]
    cases = [c for c in E.cases() if c.family == family]
    before = [E.expected(c) for c in cases]
    monkeypatch.setattr(module, attr, make())
    after = [E.expected(c) for c in cases]
    monkeypatch.undo()
    assert [E.expected(c) for c in cases] == before              # (the restatements are themselves again)
    killers = [c.name for c, a, b in zip(cases, before, after) if a != b]
    print("%s: told apart by %s" % (mutant, killers))
    assert killers, (mutant, family)
