"""The crafted find_longest_line cases (tests/longest_line_cases.py) on the CPU: every case's check holds on the oracle at every size
it is placed at, the restated residency rule gives every case's declared mode and every mode is hit from inside and outside the
kept box, the oracle agrees bit for bit with the numpy restatement (tests/independent_lsd.py) and with the cases' own walker on
every call -- and the cases have teeth: the walker with one rule changed at a time differs from the oracle on at least one call of
the family named for that rule."""
import numpy as np
import pytest

import independent_lsd as ind
import longest_line_cases as L
import lsd_cases as C
from oracle import oracle as o

f32 = np.float32
SIZE_IDS = {C.SMALL: "768p", C.HD: "1080p", C.QHD: "1440p", C.WIDE: "ultrawide"}


def test_the_case_list():
    names = [c.name for c in L.cases()]
    assert len(set(names)) == len(names) and set(c.family for c in L.cases()) == set(L.FAMILIES)
    for size in (C.SMALL, C.HD):
        assert set(c.family for c in L.cases_at(size)) == set(L.FAMILIES), size           # every family at both small sizes
    assert all(c.family == "residency" for c in L.cases_at(C.WIDE)) and len(L.cases_at(C.WIDE)) >= 3
    assert sum(c.family == "residency" for c in L.cases_at(C.QHD)) >= 5
    for size in C.SIZES:
        for family in L.FAMILIES:
            n = sum(len(L.calls_of(c, size)) for c in L.cases_at(size, family))
            assert n <= L.MAX_CALLS, (size, family, n)
        assert all(1 <= len(L.calls_of(c, size)) <= 16 for c in L.cases_at(size))
    # the short family holds a winner for every K it names (K = 1 has none: see the module's docstring)
    ks = set(k for kind in L.BAR_LEN for k in L.BAR_LEN[kind]) | {2, 3}
    assert ks == set(L.SHORT_KS), sorted(ks)
    assert L.kernel_constant("LSD_QCAP") == 1024 and L.kernel_constant("LSD_A_BATCHES") * 32 == 64       # what "handover" and "overflow" are built around
    assert L.GAP_NEXT_60000 > 60000.0 and f32(L.GAP_NEXT_60000) == np.nextafter(f32(60000), f32(np.inf))


@pytest.mark.parametrize("size", C.SIZES, ids=SIZE_IDS.get)
def test_checks_hold_on_the_oracle(size):
    bad = []
    for P in L.reference(size):
        assert np.array_equal(P.mask, L.synthetic_mask(P.case.seeds, size, P.case.anchor)), P.case.name     # the mask the seeds were designed for
        if P.case.check is not None:
            try:
                P.case.check(P)
            except AssertionError as e:
                bad.append((P.case.name, str(e)[:300]))
    assert not bad, bad


def test_residency_rule_and_its_coverage():
    hit = set()
    for size in C.SIZES:
        for P in L.reference(size):
            mode = L.mode_for(P.mask, size)
            assert mode == P.case.modes.get(size, L.ROWS), (P.case.name, size, mode)           # (a case that declares nothing is a ROWS case)
            for (px, py, gap) in P.calls:
                if np.isfinite(px) and np.isfinite(py):
                    hit.add((mode, L.in_box(P, px, py)))
    assert hit == {(m, b) for m in (L.ROWS, L.XWIN, L.GLOBAL) for b in (True, False)}, sorted(hit)
    # up to 1080p every non-empty mask is a ROWS frame; above, the three modes part by the box
    for size in (C.SMALL, C.HD):
        assert all(L.mode_for(P.mask, size) == (L.ROWS if P.mask.any() else L.GLOBAL) for P in L.reference(size))
    # the starts one row / pixel outside the kept rows and word columns, with white on the box's own edge within max_gap of them
    for P in L.reference(C.QHD):
        if P.case.name in ("res_rows", "res_xwin"):
            y0, y1, w0, w1 = L.box(P.mask, C.QHD)
            _, xoff = L.geometry(C.QHD)
            x0, x1 = w0 * 32 - xoff, (w1 + 1) * 32 - xoff - 1
            starts = [(px, py) for px, py, _ in P.calls]
            for edge, want in (("above", lambda px, py: py == y0 - 1), ("below", lambda px, py: py == y1 + 1),
                               ("left", lambda px, py: px == x0 - 1 and y0 <= py <= y1), ("right", lambda px, py: px == x1 + 1 and y0 <= py <= y1)):
                near = [(px, py) for px, py in starts if want(px, py)]
                assert near, (P.case.name, edge)
                for px, py in near:
                    assert o.find_longest_line(P.mask, px, py, 15.0)[1] > 4, (P.case.name, edge, px, py)     # its rays reach the white on the edge
    # GLOBAL: two consecutive calls further apart than the row cache, which does not hold the whole ROI
    P = [P for P in L.reference(C.QHD) if P.case.name == "res_global"][0]
    assert L.cache_rows(C.QHD) < C.ROI[C.QHD][3] and abs(P.calls[1][1] - P.calls[0][1]) > L.cache_rows(C.QHD)


@pytest.mark.parametrize("family", L.FAMILIES)
def test_oracle_equals_the_restatements(family):
    n = 0
    for size in C.SIZES:
        for P in L.reference(size):
            if P.case.family != family:
                continue
            for (px, py, gap) in P.calls:
                a = o.find_longest_line(P.mask, px, py, gap)
                b = ind.find_longest_line(P.mask, px, py, gap)
                c = L.longest(P.mask, px, py, gap)
                assert L.same(a, b) and L.same(a, c), (P.case.name, size, px, py, gap, a, b, c)
                n += 1
    assert n >= 5


def test_the_walker_is_the_restatement_ray_by_ray():
    for P in L.reference(C.SMALL):
        if P.case.name in ("short_h_K49", "hand_white_again_at_64", "over_disc_80", "out_top_left", "gaps_handover_K64", "nonfinite_starts"):
            for (px, py, gap) in P.calls:
                xe, ye, l2 = ind.ray_lengths(P.mask, px, py, f32(gap))
                R = L.rays(P.mask, px, py, gap)
                assert np.array_equal(xe, R.xe, equal_nan=True) and np.array_equal(ye, R.ye, equal_nan=True) and np.array_equal(l2, R.len2, equal_nan=True), (P.case.name, px, py, gap)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

MUTANTS = {  # name: (knobs of the walker, the family whose edge the rule moves)
    "ties go to the lowest index": (dict(first_max=True), "ties"),
    "the end point is x, not x - dx": (dict(end_at_x=True), "short"),
    "abort at gap > max_gap": (dict(abort_gt=True), "handover"),
    "the position restored is the last sample": (dict(no_restore=True), "handover"),
    "wrapping cast behind a ray that left the image": (dict(wrap_cast=True), "outside"),
    "T = floor(max_gap) + 1": (dict(floor_T=True), "gaps"),
    "short rays end at start + (K - 1) d": (dict(short_mul=True), "short"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_told_apart(mutant):
    """The family named for the mutant holds a call on which it differs from the oracle, and on that call the walker without any change
    agrees with the oracle."""
    knobs, family = MUTANTS[mutant]
    killers = []
    for P in L.reference(C.SMALL):
        if P.case.family != family or killers:
            continue
        for (px, py, gap) in P.calls:
            a = o.find_longest_line(P.mask, px, py, gap)
            if not L.same(a, L.longest(P.mask, px, py, gap, **knobs)):
                assert L.same(a, L.longest(P.mask, px, py, gap)), (P.case.name, px, py, gap)
                killers.append((P.case.name, px, py, gap))
                break
    print("%s: told apart by %s" % (mutant, killers))
    assert killers, (mutant, family)


def test_short_rays_need_the_replayed_sum():
    """The rule that tells an inexact short ray from an exact one, counted: start + (K - 1) d is not the sum of K - 1 additions on most
    calls of the short family whose winner has K <= 49."""
    n = differ = 0
    for P in L.reference(C.SMALL):
        if P.case.family != "short":
            continue
        for (px, py, gap) in P.calls:
            R = L.rays(P.mask, px, py, gap)
            if R.K[L.winner(R)] <= 49:
                n += 1
                differ += not L.same(L.longest(P.mask, px, py, gap), L.longest(P.mask, px, py, gap, short_mul=True))
    print("short winners with K <= 49: %d calls, %d differ under the mutant" % (n, differ))
    assert n >= 20 and differ >= 5, (n, differ)


def test_pruned_rays_end_K_minus_1_steps_from_the_start():
    """What pass 1 and pass 2 of the ray engine rest on (csrc/smh_lsd.hip, above ray_engine): a ray that aborts within the first 64 samples with
    its gap starting at step K ends K - 1 unit steps from the start to within 0.25, so a unit whose largest K is more than 2 below the
    candidate's cannot hold the winner."""
    worst = 0.0
    for size in C.SIZES:
        for P in L.reference(size):
            for (px, py, gap) in P.calls:
                if not (np.isfinite(px) and np.isfinite(py) and 0 < gap <= 60000):
                    continue
                R = L.rays(P.mask, px, py, gap)
                s = R.aborted & (R.stop < 64) & (R.K >= 1)
                if s.any():
                    worst = max(worst, float(np.abs(np.sqrt(R.len2[s].astype(np.float64)) - (R.K[s] - 1)).max()))
    print("largest |length - (K - 1)| of a ray that aborts within 64 samples: %.6f" % worst)
    assert 0 < worst < 0.25, worst
