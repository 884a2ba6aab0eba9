"""The search service's window reuse, on the CPU:

  * the placement rule of csrc/smh_window_place.h, compiled into a stand-alone program (tests/window_place_check.cpp; with
    -fsanitize=address,undefined where the host compiler links it) and held against a pixel-wise statement of what it means, for
    every candidate of a corner region and the border strips of the 1080p and 1440p ROIs, E in {0, 8, 24}; the four mutants (the
    predicate asked about a window one row or one word off the stored one) must fail;
  * the crafted cases of tests/window_reuse_cases.py on the oracle: lines, the pixel the line was accepted at, the scan of
    tests/independent_lsd.py agreeing with the oracle's rounds, and what the Python model of the rule says about the probe's
    candidate for E = 0 and for the E the sources are built with."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lsd_cases as C
import window_reuse_cases as WR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "squad-mortar-helper_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("window_place") / "window_place_check")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "window_place_check.cpp"), "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                                  # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    return out


def test_the_rule_means_containment(checker):
    r = subprocess.run([checker, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])


@pytest.mark.parametrize("mutant,what", [(1, "row_above"), (2, "row_below"), (3, "word_left"), (4, "word_right")])
def test_a_rule_that_is_one_off_fails(checker, mutant, what):
    r = subprocess.run([checker, str(mutant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAILED" in r.stdout, (what, r.returncode, r.stdout[-400:], r.stderr[-2000:])


def test_the_python_model_speaks_of_the_same_window():
    assert WR.header_constants() == {"SMH_WIN_R": WR.R, "SMH_WIN_WORDS": WR.WORDS}
    assert WR.built_extra() in WR.E_CHOICES
    # the model against the rule's own statement, on a grid that crosses words, rows and the negative placements
    for px in range(0, 300, 7):
        for py in (0, 3, 66, 67, 68, 200):
            x0w, y0 = WR.fresh(px, py)
            assert x0w * 32 <= px - WR.R < x0w * 32 + 32 and y0 == py - WR.R
            for extra in WR.E_CHOICES:
                rows = WR.BASE_ROWS + extra
                assert WR.holds(x0w, y0, rows, px, py)
                assert WR.holds(x0w, y0, rows, px, py + extra) and not WR.holds(x0w, y0, rows, px, py + extra + 1) and not WR.holds(x0w, y0, rows, px, py - 1)
                last = x0w * 32 + 32 * WR.WORDS - 1 - WR.R
                assert WR.holds(x0w, y0, rows, last, py) and not WR.holds(x0w, y0, rows, last + 1, py) and not WR.holds(x0w, y0, rows, x0w * 32 + WR.R - 1, py)


@pytest.mark.parametrize("size", WR.SIZES, ids=["768p", "1440p"])
def test_cases_on_the_oracle(size):
    refs = WR.reference(size)
    _, _, rw, rh = C.ROI[size]
    eb = WR.built_extra()
    for c in WR.cases():
        R = refs[c.name]
        assert len(R.lines) == c.lines, (c.name, R.lines)
        if size != WR.SIZES[0] and c.family not in ("a", "b", "c"):
            continue                                                         # (the scan below once per case: the mask is the same up to the anchor's shift)
        seq = WR.visited(R.mask)
        assert len(seq) == R.rounds and sum(ok for _, _, ok in seq) == c.lines, (c.name, len(seq), R.rounds)
        if c.family in ("e", "f"):
            assert R.rounds >= (300 if c.name == "f_heavy" else 1), (c.name, R.rounds)
            continue
        # the probe: the only accepted candidate, where the case put it, with rejected candidates of the dots before it
        k = [i for i, (_, _, ok) in enumerate(seq) if ok]
        assert len(k) == 1 and k[0] >= 1, (c.name, k)
        ax, ay = C.ANCHORS[c.anchor](rw, rh)
        if c.probe is not None:
            assert seq[k[0]][:2] == (c.probe[0] + ax, c.probe[1] + ay), (c.name, seq[k[0]], c.probe)
        px = [(x, y) for x, y, _ in seq]
        for extra, want in ((0, c.fill_e0), (eb, c.fill_built)):
            if want is not None:
                assert WR.model(px, extra)[k[0]] == want, (c.name, extra, want, px[:k[0] + 1])


def test_a_frames_last_window_holds_the_next_frames_first_candidate():
    """e_first_*: whichever mask a wave had last, the window it is left with (the rule at the E the sources are built with, no help and any
    help: the owner never fills again after the blob's first pixel) holds the first candidate of the other mask, (150, 99), and covers
    columns in which the masks differ along that candidate's ray: an owner that kept its tag across frames would change a record."""
    refs = WR.reference(WR.SIZES[0])
    eb = WR.built_extra()
    a, b = WR.visited(refs["e_first_alone"].mask), WR.visited(refs["e_first_continued"].mask)
    assert a[0][:2] == b[0][:2] == (150, 99) and b[0][2] and not any(ok for _, _, ok in a)
    for seq in (a, b):
        px = [(x, y) for x, y, _ in seq]
        fills = WR.model(px, eb)
        assert fills == [True] + [False] * (len(px) - 1), fills                # one fill, at the first candidate: what every later one leaves behind
        x0w, y0 = WR.fresh(*px[0])
        assert WR.holds(x0w, y0, WR.BASE_ROWS + eb, 150, 99)
        lo, hi = x0w * 32, x0w * 32 + 32 * WR.WORDS
        ma, mb = refs["e_first_alone"].mask, refs["e_first_continued"].mask
        assert lo <= 150 and hi > 150 + 64 and not np.array_equal(ma[99:102, 150:150 + 64], mb[99:102, 150:150 + 64])


def test_stale_masks_differ_only_beyond_the_blob():
    """e: the two masks agree on every candidate's pixel up to the blob's first, and that candidate is accepted in one and rejected in
    the other: a window carried from one to the other changes a record."""
    refs = WR.reference(WR.SIZES[0])
    a, b = WR.visited(refs["e_blob_alone"].mask), WR.visited(refs["e_blob_continued"].mask)
    k = [i for i, (_, _, ok) in enumerate(b) if ok]
    assert len(k) == 1 and k[0] >= 8 and b[k[0]][:2] == (150, 99), (k, b[k[0]] if k else None)
    assert [p[:2] for p in a[:k[0] + 1]] == [p[:2] for p in b[:k[0] + 1]] and not a[k[0]][2]
    assert np.array_equal(refs["e_blob_alone"].mask[:, :181], refs["e_blob_continued"].mask[:, :181])
