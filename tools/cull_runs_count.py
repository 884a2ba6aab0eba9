"""What the culling scan of cand_setup (csrc/smh_lsd_wave.inc) waits for per candidate: LDS round trips of the wave and look-ups of its
busiest lane, for the walk pixel by pixel and for the walk by runs (csrc/smh_cull_rule.h), with the outer annulus alone and with both (CPU only).

  python tools/cull_runs_count.py [frames=64] [W=1920 H=1080] [n_lines=2]

The frames, masks and candidates are those of tools/cull_chain_count.py: bench.py's scene, then the 2560 x 1440 open-map fixtures; the
annuli are the header's own (tests/cull_runs_check.cpp, `codes`).  A lane owns the cells lane + 64 it, it = 0 .. 6, of the 105 x 4 cells
of 32 pixels about the candidate, and the wave moves from one `it` to the next together:

  pixels        four white annulus pixels of a lane's cell per round trip (the scan before the runs): an `it` costs the wave
                max over lanes of ceil(pixels / 4) round trips, four look-ups each
  runs, looped  a run of either annulus per round trip (its two ends: four look-ups): max over lanes of max(outer runs, middle runs)
  runs          the scan as it is: the first run of either annulus of all seven cells in ONE round trip (28 look-ups), then the loop
                over what is left

Prints per candidate and per frame, and one JSON line.  The issue's gate: the walk by runs with two annuli has to come out below the walk
pixel by pixel with one."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

T = 15
R = 52
DIM = 2 * R + 1
WALKS = ("pixels", "runs_looped", "runs")


def annuli(exe, t):
    """-> (in_outer, in_middle) bool[105, 128] (columns padded to four cells) of threshold t, from the check program's table."""
    rows = subprocess.run([exe, "codes", str(t)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    head = rows[0].split()
    assert head[0] == "windows" and head[5:] == ["1", "1", "1"], head      # chained, both annuli by runs
    out = np.zeros((2, DIM, 128), bool)
    for r_, ln in enumerate(rows[1:]):
        for c_, e in enumerate(ln.split()):
            out[0, r_, c_], out[1, r_, c_] = e[0] == "1", e[1] == "1"
    return out[0], out[1]


def per_cell(hit):
    """hit bool[105, 128] -> (pixels, runs) per cell, int[420] in the scan's cell order (row * 4 + j)."""
    cells = hit.reshape(DIM, 4, 32)
    starts = cells & ~np.concatenate([np.zeros((DIM, 4, 1), bool), cells[:, :, :-1]], axis=2)   # (a run ends at its cell's border: so does the scan's)
    return cells.sum(2).reshape(-1), starts.sum(2).reshape(-1)


def by_it(v):
    """max over the lanes of each `it`: int[420] -> int[7]"""
    v = np.concatenate([v, np.zeros(7 * 64 - len(v), v.dtype)])
    return v.reshape(7, 64).max(1)


def cost(mask, xs, ys, in_o, in_m):
    """-> {(walk, annuli): (round trips, look-ups of the busiest lane)} of one candidate"""
    h, w = mask.shape
    fx, fy = int(np.floor(xs)), int(np.floor(ys))
    white = np.zeros((DIM, 128), bool)
    y0, y1, x0, x1 = max(fy - R, 0), min(fy + R + 1, h), max(fx - R, 0), min(fx - R + 128, w)
    white[y0 - fy + R:y1 - fy + R, x0 - fx + R:x1 - fx + R] = mask[y0:y1, x0:x1] == 255
    px_o, runs_o = per_cell(white & in_o)
    px_m, runs_m = per_cell(white & in_m)
    px_b, _ = per_cell(white & (in_o | in_m))                              # (the pixel walk takes a pixel of both annuli once)
    out = {}
    for n, px, runs in ((1, px_o, runs_o), (2, px_b, np.maximum(runs_o, runs_m))):
        trips = int(by_it((px + 3) // 4).sum())
        out["pixels", n] = (trips, 4 * trips)
        trips = int(by_it(runs).sum())
        out["runs_looped", n] = (trips, 4 * trips)
        trips = int(by_it(np.maximum(runs - 1, 0)).sum())
        out["runs", n] = (1 + trips, 28 + 4 * trips)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080
    n_lines = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    import cull_chain_cases as CC
    import fixtures
    import test_cull_runs_host as TH
    from oracle import oracle as o
    from squad_mortar_helper_amd import synth
    with tempfile.TemporaryDirectory() as d:
        in_o, in_m = annuli(TH.checker(d), T)
    res = {}
    bench = [o.process_frame(synth.make_frame(W, H, i, n_lines=n_lines)[0], stages=0x1, max_gap=T, want_images=True)["lsd"] for i in range(n)]
    stems = [s_ for s_ in fixtures.OPEN_STEMS if (fixtures.MANIFEST[s_]["W"], fixtures.MANIFEST[s_]["H"]) == (2560, 1440)]
    shots = [o.process_frame(fixtures.load_fixture(s_)[0], stages=0x1, max_gap=T, want_images=True)["lsd"] for s_ in stems]
    for name, masks in (("bench scene %d x %d, frames 0 .. %d" % (W, H, n - 1), bench), ("2560 x 1440 open-map fixtures (%s)" % ", ".join(stems), shots)):
        if not masks:
            continue
        tot = {}
        rounds = 0
        for mask in masks:
            for xs, ys, _, _ in CC.candidates(mask, T):
                rounds += 1
                for k, v in cost(mask, xs, ys, in_o, in_m).items():
                    t_ = tot.setdefault(k, [0, 0])
                    t_[0] += v[0]; t_[1] += v[1]
        c = dict(frames=len(masks), rounds=rounds, rounds_per_frame=rounds / len(masks))
        print("%s: %d rounds, %.1f per frame" % (name, rounds, c["rounds_per_frame"]))
        print("  walk          annuli   round trips per candidate   per frame   look-ups of the busiest lane per candidate   per frame")
        for walk in WALKS:
            for na in (1, 2):
                tr, lu = tot[walk, na]
                c["%s_%d" % (walk, na)] = dict(round_trips_per_candidate=tr / rounds, round_trips_per_frame=tr / len(masks), lookups_per_candidate=lu / rounds, lookups_per_frame=lu / len(masks))
                print("  %-13s %6d   %25.2f   %9.1f   %42.2f   %9.1f" % (walk, na, tr / rounds, tr / len(masks), lu / rounds, lu / len(masks)))
        c["gate_runs_2_below_pixels_1"] = tot["runs", 2][0] < tot["pixels", 1][0]
        print("  the walk by runs with two annuli %s the walk pixel by pixel with one" % ("comes out below" if c["gate_runs_2_below_pixels_1"] else "DOES NOT come out below"))
        res[name] = c
    print(json.dumps(dict(T=T, counts=res)))


if __name__ == "__main__":
    main()
