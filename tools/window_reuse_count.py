"""How often the search service's wave has to fill its candidate window on the benchmark's frames (CPU only).

  python tools/window_reuse_count.py [frames=48] [W=1920 H=1080] [n_lines=2]

The frames are bench.py's scene, synth.make_frame(W, H, i, n_lines); the mask is the oracle's; the candidates are those of the sequential
scan (tests/independent_lsd.py, through tests/window_reuse_cases.visited); the rule is the one the device applies
(csrc/smh_window_place.h; tests/window_reuse_cases.model, held against the header by tests/test_window_reuse_host.py).  Prints, for
every window height a build may choose (E extra rows below: SVC_WIN_EXTRA), rounds and window fills per frame as ONE wave casting every
candidate of its frame meets them -- what the -DSMH_LSD_WDEBUG build counts per frame (tools/svc_rate.py, `window_fills`) when no
helper takes candidates off the owner (RATE_FLAGS=9) -- and one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080
    n_lines = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    import window_reuse_cases as WR
    from oracle import oracle as o
    from squad_mortar_helper_amd import synth
    assert WR.header_constants() == {"SMH_WIN_R": WR.R, "SMH_WIN_WORDS": WR.WORDS}
    rounds, fills = 0, {e: 0 for e in WR.E_CHOICES}
    for i in range(n):
        frame, _ = synth.make_frame(W, H, i, n_lines=n_lines)
        r = o.process_frame(frame, stages=0x1, max_gap=15, want_images=True)
        seq = WR.visited(r["lsd"])
        assert len(seq) == r["rounds"], (i, len(seq), r["rounds"])
        rounds += len(seq)
        for e in WR.E_CHOICES:
            fills[e] += sum(WR.model([(x, y) for x, y, _ in seq], e))
    print("%d frames of %d x %d: %d rounds, %.1f per frame" % (n, W, H, rounds, rounds / n))
    print("  E   rows   fills   per frame   share of the rounds")
    for e in WR.E_CHOICES:
        print("%3d   %4d   %5d   %9.2f   %5.1f %%" % (e, WR.BASE_ROWS + e, fills[e], fills[e] / n, 100.0 * fills[e] / max(rounds, 1)))
    print(json.dumps(dict(frames=n, frame=[W, H], rounds=rounds, rounds_per_frame=rounds / n, built_extra=WR.built_extra(),
                          fills={str(e): fills[e] for e in WR.E_CHOICES}, fills_per_frame={str(e): fills[e] / n for e in WR.E_CHOICES})))


if __name__ == "__main__":
    main()
