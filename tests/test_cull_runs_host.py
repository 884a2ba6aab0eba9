"""The run rule of the sector cull (csrc/smh_cull_rule.h: smh_cull_run_units, smh_cull_by_runs, the starts / ends of a word's runs) on the
CPU.  The header is compiled into a stand-alone program, tests/cull_runs_check.cpp, with -fsanitize=address,undefined where the host
compiler links it; the program walks every threshold T = 1 .. 49, every annulus the rule applies to, every row, every cell and every
sub-run inside the cell, with the byte codes the host condenses the table into (smh_cull_unit_code):

  (a) the run's units contain the OR of its pixels' dense units;
  (b) where no code of the run is 0xFF they equal the OR of the pixels' coded units -- all of T = 15;
  (c) the predicate refuses exactly the annuli with a lower step < 3, and T = 24, 48 and 49 each hold a counter-example there;
  (d) starts, ends and their pairing over a whole word give the union over the word's runs (single runs, pairs, alternating, full, random).

Each mutant -- the first pixel's code alone, the larger of the two cyclic intervals, 0xFF read as a range, the rule applied from a lower
step of 1 on, runs taken before the annulus mask -- fails some check."""
import os
import shutil
import subprocess

import pytest

import cull_chain_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
MUTANTS = ("first_code_alone", "larger_interval", "ff_as_a_range", "runs_at_lower_step_1", "runs_before_the_mask")


def checker(directory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = os.path.join(str(directory), "cull_runs_check")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CC.CSRC, os.path.join(HERE, "cull_runs_check.cpp"), "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                                # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return checker(tmp_path_factory.mktemp("cull_runs"))


def test_the_run_rule_holds(exe):
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.splitlines()[-1].startswith("ok:"), (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    # the three refused annuli each showed their counter-example, and T = 15 was walked in both annuli
    for t, a in ((24, 1), (48, 0), (49, 0)):
        assert any(ln.startswith("T = %d, annulus %d" % (t, a)) and "(refused)" in ln for ln in r.stdout.splitlines()), r.stdout
    assert sum(ln.startswith("T = 15, annulus") for ln in r.stdout.splitlines()) == 2


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_mutant_is_caught(exe, mutant):
    r = subprocess.run([exe, "check", mutant], capture_output=True, text=True, timeout=120)
    print(r.stdout[-600:])
    assert r.returncode == 1 and "FAILED" in r.stdout and r.stderr == "", (r.returncode, r.stdout[-600:], r.stderr[-2000:])


def test_the_codes_are_the_tables(exe, tmp_path):
    """The program's condensed table speaks of the same annuli as the header's dense one (tests/cull_rule_check.cpp)."""
    import numpy as np
    w, tab = CC.header_table(CC.checker(tmp_path), 15)
    rows = subprocess.run([exe, "codes", "15"], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert rows[0].split() == ["windows", "35", "50", "19", "34", "1", "1", "1"]
    ent = [ln.split() for ln in rows[1:]]
    assert np.array_equal(np.array([[e[0] == "1" for e in ln] for ln in ent]), (tab & CC.IN_OUTER) != 0)
    assert np.array_equal(np.array([[e[1] == "1" for e in ln] for ln in ent]), (tab & CC.IN_MIDDLE) != 0)
    assert all(e[2:] != "ff" for ln in ent for e in ln if e[:2] != "00")   # every annulus pixel of T = 15 has a plain range
