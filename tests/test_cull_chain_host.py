"""The chained sector cull (csrc/smh_cull_rule.h; behind -DSMH_CULL_CHAIN: the library's own build applies the outer annulus alone, and
these tests keep the rule that is not in use proven), on the CPU:

  * the header compiled into a stand-alone program (tests/cull_rule_check.cpp; with -fsanitize=address,undefined where the host compiler
    links it): its own checks of the windows, the entries and the AND, and its dense table equal to the numpy restatement of
    tests/cull_chain_cases.py;
  * the table covers what rays sample: every ray of the committed direction table, every step of each annulus' window, the reference's
    repeated f32 additions, start points on a grid of fractions (the multiples of 0.5 get_centre produces among them): the sampled pixel's
    offset from floor(start) carries the ray's unit in that annulus' table.  This is the conservativeness the proof rests on;
  * soundness by the second restatement: on the crafted masks and on two sample screenshots, every ray with len^2 > 2500
    (tests/independent_lsd.ray_lengths) of every visited candidate lies in a unit the chained rule keeps;
  * the mutants -- a middle annulus one step too narrow at either end, an angular half-width without its margin (the start point's place in
    its pixel), an AND taken across neighbouring units instead of the same unit -- are each caught by one of the two.

(The half-width asin(rho / r0) + 0.2 degrees has two margins.  The 0.2 degrees alone is not needed by any ray of the committed table at
these radii -- dropping it goes unnoticed, which the first test of the mutants states -- so the mutant drops rho's share for the start
point, 0.7072 px, as well.)"""
import numpy as np
import pytest

import cull_chain_cases as CC
import fixtures

T = CC.MAX_GAP
SCREENSHOTS = ("point_png", "points_intersect_png")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return CC.checker(tmp_path_factory.mktemp("cull_rule"))


@pytest.fixture(scope="module")
def table(exe):
    return CC.header_table(exe, T)


@pytest.fixture(scope="module")
def scans():
    """[(name, mask, candidates)] of the crafted cases at the smallest size and of two screenshots: the scan once for all tests."""
    from oracle import oracle as o
    out = []
    refs = CC.reference(CC.SIZES[0])
    for c in CC.cases():
        out.append((c.name, refs[c.name].mask, CC.candidates(refs[c.name].mask)))
        assert len(out[-1][2]) == refs[c.name].rounds, (c.name, len(out[-1][2]), refs[c.name].rounds)
    for stem in SCREENSHOTS:
        f, _, _ = fixtures.load_fixture(stem)
        r = o.process_frame(f, stages=0x1, max_gap=T, want_images=True)
        out.append((stem, r["lsd"], CC.candidates(r["lsd"])))
        assert len(out[-1][2]) == r["rounds"], (stem, len(out[-1][2]), r["rounds"])
    return out


def _unsound(scans, w, tab, **kw):
    """Rays with len^2 > 2500 that lie in a unit the rule does not keep: [(name, candidate, ray)]."""
    bad = []
    for name, mask, cands in scans:
        for i, (xs, ys, length, _) in enumerate(cands):
            rays = np.nonzero(length > np.float32(2500))[0]
            if len(rays):
                _, live = CC.live_units(mask, xs, ys, w, tab, **kw)
                bad += [(name, i, int(r_)) for r_ in rays if not (live >> (int(r_) // 64)) & 1]
    return bad


def test_the_header_checks_itself(exe, tmp_path):
    import subprocess
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    # the library's own build (no -DSMH_CULL_CHAIN): the outer annulus alone, the same outer table
    plain = CC.checker(tmp_path, defines=())
    r = subprocess.run([plain, "check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    (w0, t0), (w1, t1) = CC.header_table(plain, T), CC.header_table(exe, T)
    assert w0 == dict(outer=(35, 50), middle=None) and not (t0 & CC.IN_MIDDLE).any()
    sel = (t1 & CC.IN_OUTER) != 0
    assert np.array_equal(sel, t0 != 0) and np.array_equal(t0[sel], t1[sel] & ~CC.IN_MIDDLE)


def test_the_model_speaks_of_the_same_rule(exe, table):
    assert CC.header_constants() == dict(R=CC.R, units=CC.UNITS, step=50)
    for t in (T, 7, 24, 25, 49):
        w, tab = CC.header_table(exe, t) if t != T else table
        mw, mtab = CC.model_table(t)
        assert w == mw and np.array_equal(tab, mtab), (t, w, mw, int((tab != mtab).sum()))
    assert table[0] == dict(outer=(35, 50), middle=(19, 34))
    assert CC.header_table(exe, 25)[0]["middle"] is None and CC.header_table(exe, 24)[0]["middle"] == (1, 25)


@pytest.mark.parametrize("t", (T, 7, 24, 30))
def test_table_covers_what_rays_sample(exe, table, t):
    w, tab = table if t == T else CC.header_table(exe, t)
    assert CC.covers(w, tab) == 0


@pytest.mark.parametrize("size", CC.SIZES, ids=["768p", "1440p"])
def test_the_cases_are_what_they_claim(size):
    """On the oracle, along the axis (where a seed is a sample; the rounded seeds of an oblique bar make its gaps a sample longer or shorter
    for one ray or another, and the oracle says which): the bars with gaps of T are found whole, across both gaps; with a gap of T + 1 in the
    same place they are not.  The blobs are rejected."""
    for n, R in CC.reference(size).items():
        if R.case.lines is not None:
            assert len(R.lines) == R.case.lines, (n, R.lines)
        if n.startswith("gap_t_at_") and n.endswith("_000_0"):
            assert len(R.lines) >= 1 and max(np.hypot(ln[2] - ln[0], ln[3] - ln[1]) for ln in R.lines) > 80, (n, R.lines)
        if n.startswith("gap_t1_at_") and n.endswith("_000_0"):
            assert all(np.hypot(ln[2] - ln[0], ln[3] - ln[1]) < 80 for ln in R.lines), (n, R.lines)


def test_the_rule_is_sound_on_masks(scans, table):
    w, tab = table
    assert sum(len(c) for _, _, c in scans) > 300 and sum(ok for _, _, c in scans for _, _, _, ok in c) >= 20
    assert _unsound(scans, w, tab) == []
    # and it rejects what the outer annulus alone would cast: the blob whose only white neighbours are 40 px away
    name, mask, cands = next(s_ for s_ in scans if s_[0] == "arc_outer_only")
    outer, live = CC.live_units(mask, cands[0][0], cands[0][1], w, tab)
    assert outer != 0 and live == 0, (outer, live)
    outer, live = CC.live_units(*next((m, c[0][0], c[0][1]) for n, m, c in scans if n == "arc_both"), w, tab)
    assert outer != 0 and live == outer, (outer, live)


def test_dropping_the_small_angular_margin_alone_goes_unnoticed():
    w, tab = CC.model_table(T, margin=0.0)
    assert CC.covers(w, tab) == 0


MUTANTS = {
    "middle_lower_end_narrow": dict(table=dict(mid_lo=1)),
    "middle_upper_end_narrow": dict(table=dict(mid_hi=-1)),
    "delta_without_margin": dict(table=dict(rho_units=0.7072, margin=0.0)),
    "and_with_the_next_unit": dict(live=dict(neighbour=1)),
    "and_with_the_previous_unit": dict(live=dict(neighbour=-1)),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_is_caught(scans, table, mutant):
    m = MUTANTS[mutant]
    if "table" in m:
        # the windows the samples are taken from are the rule's own: a narrowed annulus has to answer for the whole window
        missed = CC.covers(table[0], CC.model_table(T, **m["table"])[1])
        print(mutant, "samples not covered:", missed)
        assert missed > 0
    else:
        bad = _unsound(scans, table[0], table[1], **m["live"])
        print(mutant, "acceptable rays in units the mutant drops:", len(bad), bad[:4])
        assert bad
