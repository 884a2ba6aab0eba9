"""How many 64-ray units the sector cull leaves per candidate, under the outer annulus alone and under the chained rule (CPU only).

  python tools/cull_chain_count.py [frames=16] [W=1920 H=1080] [n_lines=2]

The frames are bench.py's scene, synth.make_frame(W, H, i, n_lines), and after them the 2560 x 1440 open-map fixtures of tests/golden; the mask
is the oracle's; the candidates are those of the sequential scan (tests/independent_lsd.py, through tests/cull_chain_cases.candidates); the
table is the one the device tabulates -- csrc/smh_cull_rule.h compiled into tests/cull_rule_check.cpp -- condensed as the host condenses it
(smh_runtime.cpp: a pixel's units as the smallest cyclic run of at most four units, else every unit).  Prints rounds and live units per
candidate and per frame under both rules, and one JSON line.  `units_per_frame` is what the -DSMH_LSD_WDEBUG build counts as `n_units` per
frame (tools/svc_rate.py) when the frame's own wave casts every candidate (RATE_FLAGS=9: no help) over the same frames -- svc_rate.py
takes frames 0 .. 63 -- `outer` for the library as it is built, `chained` for a build with -DSMH_CULL_CHAIN."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

T = 15


def condensed(tab, CC):
    """The dense table with every pixel's units replaced by what its byte code stands for (unit_code, smh_runtime.cpp)."""
    NU = CC.UNITS
    out = tab.copy()
    cache = {}
    for iy, ix in zip(*np.nonzero(tab)):
        m = int(tab[iy, ix] & CC.UNIT_MASK)
        if m not in cache:
            first, cnt, best_gap = 0, NU, 0
            for st in range(NU):
                if not (m >> st) & 1:
                    continue
                gap = 0
                while gap < NU - 1 and not (m >> ((st + 1 + gap) % NU)) & 1:
                    gap += 1
                if gap > best_gap:
                    best_gap, first, cnt = gap, (st + 1 + gap) % NU, NU - gap
            if best_gap == 0 or cnt > 4:
                cache[m] = (1 << NU) - 1
            else:
                r = ((1 << cnt) - 1) << first
                cache[m] = (r | (r >> NU)) & ((1 << NU) - 1)
        out[iy, ix] = (tab[iy, ix] & ~CC.UNIT_MASK) | np.uint64(cache[m])
    return out


def count(masks, w, tab, CC):
    rounds = units_outer = units_chain = rejected_by_chain = 0
    for mask in masks:
        for xs, ys, _, _ in CC.candidates(mask, T):
            outer, live = CC.live_units(mask, xs, ys, w, tab)
            rounds += 1
            units_outer += bin(outer).count("1")
            units_chain += bin(live).count("1")
            rejected_by_chain += int(outer != 0 and live == 0)
    return dict(frames=len(masks), rounds=rounds, units_outer=units_outer, units_chained=units_chain, rejected_by_the_chain_alone=rejected_by_chain)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080
    n_lines = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    import cull_chain_cases as CC
    import fixtures
    from oracle import oracle as o
    from squad_mortar_helper_amd import synth
    with tempfile.TemporaryDirectory() as d:
        w, tab = CC.header_table(CC.checker(d), T)
    assert w["middle"] is not None
    tab = condensed(tab, CC)
    out = {}
    bench = [o.process_frame(synth.make_frame(W, H, i, n_lines=n_lines)[0], stages=0x1, max_gap=T, want_images=True)["lsd"] for i in range(n)]
    stems = [s_ for s_ in fixtures.OPEN_STEMS if (fixtures.MANIFEST[s_]["W"], fixtures.MANIFEST[s_]["H"]) == (2560, 1440)]
    shots = [o.process_frame(fixtures.load_fixture(s_)[0], stages=0x1, max_gap=T, want_images=True)["lsd"] for s_ in stems]
    for name, masks in (("bench scene %d x %d, frames 0 .. %d" % (W, H, n - 1), bench), ("2560 x 1440 open-map fixtures (%s)" % ", ".join(stems), shots)):
        if not masks:
            continue
        c = count(masks, w, tab, CC)
        c["rounds_per_frame"] = c["rounds"] / c["frames"]
        for k in ("outer", "chained"):
            c["units_per_candidate_" + k] = c["units_" + k] / max(c["rounds"], 1)
            c["units_per_frame_" + k] = c["units_" + k] / c["frames"]
        out[name] = c
        print("%s: %d rounds, %.1f per frame" % (name, c["rounds"], c["rounds_per_frame"]))
        print("  rule                     live units per candidate   per frame")
        print("  outer annulus alone      %24.2f   %9.1f" % (c["units_per_candidate_outer"], c["units_per_frame_outer"]))
        print("  AND the middle annulus   %24.2f   %9.1f   (%+.1f %%; %d candidates rejected by the chain alone)" % (
            c["units_per_candidate_chained"], c["units_per_frame_chained"], 100.0 * (c["units_chained"] / max(c["units_outer"], 1) - 1.0), c["rejected_by_the_chain_alone"]))
    print(json.dumps(dict(T=T, windows=w, counts=out)))


if __name__ == "__main__":
    main()
