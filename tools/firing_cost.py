"""Cost of SMHV_STAGE_FIRING and of the heightmap colour map, measured on one GPU.

  python tools/firing_cost.py [--rounds 5] [--submissions 128] [--out profiles/firing_cost.json]

Pipeline rate (256 x 1080p synthetic frames per submission, depth 12) for three stage sets: STAGE_ALL, STAGE_ALL | MINIMAP and
STAGE_ALL | MINIMAP | FIRING with a 4096^2 heightmap bound.  Each line-search schedule is pinned and measured on its own
(search = "batch" and "frame"): under SMHV_SEARCH_AUTO a new stage set is a new workload shape, and the pipeline would re-measure
its two searches inside the timed windows.  The three stage sets are interleaved round by round (the order alternates), so that
clock and neighbour drift hits all three alike; every window is preceded by 2 x depth untimed submissions of its stage set.
Then smhv_heightmap_color_map's two device passes at 4096^2 and 8192^2 (2 bytes read by each pass + 4 bytes written: 8 bytes
per texel) against the 8 TB/s HBM peak.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--submissions", type=int, default=128)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth

    W, H, N = 1920, 1080, a.frames
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, N, first_idx=0)
    d = torch.from_numpy(frames).cuda()
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos])
    rng = np.random.default_rng(0)
    hm = smh.Heightmap(v, rng.integers(0, 65536, size=(4096, 4096), dtype=np.uint16), ((0, 0), (0, 0)), (1.0, 1.0, 50.0))
    sets = {"all": smh.STAGE_ALL, "all_minimap": smh.STAGE_ALL | smh.STAGE_MINIMAP,
            "all_minimap_firing": smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_FIRING}
    out = {"depth": a.depth, "frames_per_submission": N, "submissions_per_window": a.submissions, "rounds": a.rounds, "schedules": {}}
    for search in ("batch", "frame"):
        p = smh.Pipeline(v, W, H, N, depth=a.depth, search=search)
        p.set_firing(hm)

        def run(stages, k):
            for _ in range(2 * a.depth):                              # warm-up
                p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
            p.wait()
            t0 = time.perf_counter()
            for _ in range(k):
                p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
            p.wait()
            return k * N / (time.perf_counter() - t0)

        rates = {k: [] for k in sets}
        for r in range(a.rounds):
            order = list(sets) if r % 2 == 0 else list(reversed(list(sets)))
            for name in order:
                rates[name].append(run(sets[name], a.submissions))
        p.close()
        med = {k: float(np.median(x)) for k, x in rates.items()}
        paired = [100.0 * (f / m - 1.0) for f, m in zip(rates["all_minimap_firing"], rates["all_minimap"])]
        out["schedules"][search] = {"frames_per_s": rates, "median_frames_per_s": med,
                                    "firing_vs_minimap_pct_by_round": paired,
                                    "firing_vs_minimap_pct_median": float(np.median(paired)),
                                    "minimap_vs_all_pct": 100.0 * (med["all_minimap"] / med["all"] - 1.0)}
    cm = {}
    for side in (4096, 8192):
        h2 = hm if side == 4096 else smh.Heightmap(v, rng.integers(0, 65536, size=(side, side), dtype=np.uint16), ((0, 0), (0, 0)), (1.0, 1.0, 50.0))
        buf = torch.empty(side * side * 4, dtype=torch.uint8, device="cuda")
        h2.color_map_device_ms(buf.data_ptr())
        ms = sorted(h2.color_map_device_ms(buf.data_ptr()) for _ in range(10))[5]
        gb = side * side * (2 + 2 + 4) / 1e9
        cm[str(side)] = {"ms": ms, "GBps": gb / (ms / 1e3), "pct_of_8TBps": 100.0 * gb / (ms / 1e3) / 8000.0}
        if h2 is not hm:
            h2.close()
    out["color_map"] = cm
    out["device"] = torch.cuda.get_device_name(0)
    hm.close()
    v.shutdown()
    s = json.dumps(out)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
