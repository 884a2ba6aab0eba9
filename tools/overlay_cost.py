"""Cost of SMHV_STAGE_HEIGHTMAP_OVERLAY, measured on one GPU.

  python tools/overlay_cost.py [--rounds 5] [--submissions 96] [--out profiles/overlay_cost.json] [--kernel-stats STATS.csv]
  python tools/overlay_cost.py --trace-only        (the workload for a kernel trace: a few batch runs with the stage)
  --map random | smooth: the heightmap's texels (uniform random, the colour table's worst case, or terrain-like)

Pipeline rate (256 x 1080p synthetic frames per submission, depth 12) for STAGE_ALL | MINIMAP and STAGE_ALL | MINIMAP |
HEIGHTMAP_OVERLAY with a 4096^2 heightmap bound.  Each line-search schedule is pinned and measured on its own (search = "batch"
and "frame"): under SMHV_SEARCH_AUTO a new stage set is a new workload shape, and the pipeline would re-measure its two searches
inside the timed windows.  The two stage sets are interleaved round by round (the order alternates); every window is preceded by
2 x depth untimed submissions of its stage set.

The overlay kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of --trace-only (its
*_kernel_stats.csv, passed with --kernel-stats): the ui-slab bytes it reads plus the overlay bytes it writes (2 x ui_stride per
open frame) over that time, against 6.29 TB/s achievable and 8 TB/s peak HBM bandwidth.  Prints one JSON object."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBPS, PEAK_TBPS = 6.29, 8.0


def kernel_stats(path, name="k_hm_overlay"):
    """-> (calls, average ns) of the kernel in a rocprofv3 *_kernel_stats.csv, or None."""
    with open(path) as f:
        for row in csv.DictReader(f):
            if row.get("Name", "").split("(")[0].split("<")[0].strip().endswith(name):
                return int(row["Calls"]), float(row["AverageNs"])
    return None


def heightmap_data(kind, side, rng):
    """"random": uniform u16 texels (every lane of a gather reads another colour-table line: the worst case); "smooth": terrain-like
    (a few long waves plus a little noise), neighbouring texels close in value as in a real heightmap."""
    import numpy as np
    if kind == "random":
        return rng.integers(0, 65536, size=(side, side), dtype=np.uint16)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    h = 32768.0 + 12000.0 * np.sin(x / 300.0) * np.cos(y / 410.0) + 8000.0 * np.sin((x + y) / 170.0) + rng.uniform(0.0, 64.0, size=(side, side))
    return np.clip(h, 0, 65535).astype(np.uint16)


def setup(frames_n, kind, side=4096):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    W, H = 1920, 1080
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, frames_n, first_idx=0)
    d = torch.from_numpy(frames).cuda()
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos])
    rng = np.random.default_rng(0)
    hm = smh.Heightmap(v, heightmap_data(kind, side, rng), ((0, 0), (0, 0)), (1.0, 1.0, 50.0))
    return v, d, anchors, hm, W, H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--submissions", type=int, default=96)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--map", choices=("random", "smooth"), default="random")
    a = ap.parse_args()
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh

    N = a.frames
    v, d, anchors, hm, W, H = setup(N, a.map)
    base = smh.STAGE_ALL | smh.STAGE_MINIMAP
    ovl = base | smh.STAGE_HEIGHTMAP_OVERLAY
    if a.trace_only:
        fb = smh.FrameBatch(v, W, H, N)
        fb.set_firing(hm)
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(6):
            fb.run(d.data_ptr(), N, stages=ovl, anchors=anchors, stream=s)
        recs = smh.results_to_dicts(fb.read_results(0, N))
        print(json.dumps({"open_frames": sum(1 for r in recs if r["map_open"]), "ui_stride": int(fb.layout.ui_stride)}))
        fb.close()
        hm.close()
        v.shutdown()
        return
    sets = {"all_minimap": base, "all_minimap_overlay": ovl}
    out = {"depth": a.depth, "frames_per_submission": N, "submissions_per_window": a.submissions, "rounds": a.rounds, "heightmap": [4096, 4096], "map": a.map,
           "schedules": {}}
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
        paired = [100.0 * (o / m - 1.0) for o, m in zip(rates["all_minimap_overlay"], rates["all_minimap"])]
        out["schedules"][search] = {"frames_per_s": rates, "median_frames_per_s": med, "overlay_vs_minimap_pct_by_round": paired,
                                    "overlay_vs_minimap_pct_median": float(np.median(paired))}
    fb = smh.FrameBatch(v, W, H, 1)
    ui_stride = int(fb.layout.ui_stride)
    fb.close()
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        if ks is not None:
            calls, ns = ks
            byts = 2.0 * ui_stride * N                                  # every synthetic frame is open: ui read + overlay written
            tbps = byts / ns / 1e3
            out["kernel"] = {"name": "k_hm_overlay", "calls": calls, "frames_per_launch": N, "avg_us": ns / 1e3,
                             "ui_plus_overlay_bytes": byts, "TBps": tbps, "pct_of_achievable_6p29": 100.0 * tbps / ACHIEVABLE_TBPS,
                             "pct_of_peak_8": 100.0 * tbps / PEAK_TBPS,
                             "floor_us_at_6p29": byts / (ACHIEVABLE_TBPS * 1e12) * 1e6}
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
