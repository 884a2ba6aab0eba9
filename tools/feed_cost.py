"""Cost of the remote-viewer feed (smhv_batch_feed), measured on one GPU.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/feed_cost.py --trace-only --labels LABELS.json
  python tools/feed_cost.py --kernel-trace DIR/.../*_kernel_trace.csv --labels LABELS.json [--out profiles/feed_cost.json]

The first form is the workload, run under the profiler in a run of its own (no counters in it): 256 resident 1080p frames, fed
five times each (the feed reset before every call, so every call starts without a texture) in three workloads --
  equal      every map equal to the first: one Map per call
  sixteenth  one map in sixteen differs from its predecessor: 16 Maps per call
  all        every map differs: 256 Maps per call
-- and then, alternated five times, k_map_crc over the 256 frames (a feed call on the `equal` batch) and k_crc32 over one
contiguous buffer of the same size (smhv_crc32_device).  It checks every entry's CRC of the `all` workload against zlib.crc32 of
the ui_map read back, and writes LABELS.json: the order of the launches, the shapes, and what crossed to the host.

With --views both forms measure a debug view as the Map instead (smhv_batch_feed_view; --out profiles/feed_views_cost.json): the
256 all-different frames run once in colour with every stage, then five alternated rounds of one call per source -- the ui_map,
the five views, and the two plane views whose rows fit 64 groups once more with the four-lookup form of the plane's CRC
(smhv_debug_feed_gray_form) -- the feed reset before every call.  The summary gives per source the CRC kernel's and the Maps
kernel's times, the MESSAGE bytes (what is hashed / written, not what is read) and ps per message byte next to k_map_crc's and
k_feed_maps' over the ui_map in the same run, whose alternated spread is the yardstick's.

The second form needs no GPU: it reads the trace's per-dispatch times in launch order, and reports for each kernel and workload
the time, the bytes computed from the shapes (k_map_crc reads n*w*h*4; k_feed_maps reads and writes the changed maps' bytes) and
the share of the 6.29 TB/s achievable HBM rate; the device-to-host bytes of the feed against reading every ui_map; and
k_map_crc against k_crc32 per byte with the spread of the alternated launches.  Prints one JSON object."""
import argparse
import csv
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBPS = 6.29
WORKLOADS = ("equal", "sixteenth", "all")
REPEATS = 5


def workload(a):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    W, H, N = 1920, 1080, a.frames
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, N, first_idx=0)
    d_all = torch.from_numpy(frames).cuda()
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos])
    idx = torch.arange(N, device="cuda")
    batches = {"equal": (d_all[idx * 0].contiguous(), smh.make_anchors([(infos[0]["scales_start_y"], infos[0]["anchors"])] * N)),
               "sixteenth": (d_all[(idx // 16) * 16].contiguous(), smh.make_anchors([(infos[(i // 16) * 16]["scales_start_y"], infos[(i // 16) * 16]["anchors"]) for i in range(N)])),
               "all": (d_all, anchors)}
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    _, _, rw, rh = fb.roi
    map_bytes = rw * rh * 4
    feed = smh.WebFeed(v, 6 + N * (32 + ((10 + map_bytes + 15) & ~15) + 7 + 16 * 32 + 16), N)
    labels = {"frames": N, "map_w": rw, "map_h": rh, "map_bytes": map_bytes, "launches": [], "workloads": {}}
    for name in WORKLOADS:
        d, an = batches[name]
        fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, anchors=an, stream=s)
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            feed.reset()
            fb.feed(feed, stream=s)
            torch.cuda.synchronize()
            labels["launches"].append(name)
        h, msgs = feed.read()
        labels["workloads"][name] = {"n_maps": int(h.n_maps), "n_entries": int(h.n_entries), "frames_done": int(h.frames_done),
                                     "d2h_bytes": 32 + 24 * int(h.n_entries) + int(h.bytes_used), "all_ui_maps_bytes": N * map_bytes}
        if name == "all":                                             # the CRCs at the size the timing is taken at
            crcs = {e.frame: e.crc for e in feed.entries}
            bad = [f for f in range(N) if crcs.get(f) != zlib.crc32(fb.read_image(smh._lib.IMAGE_UI_MAP, f).tobytes())]
            labels["crc_mismatches_of_%d" % N] = len(bad)
            assert not bad, bad[:8]
    # k_map_crc over 256 frames against k_crc32 over a contiguous buffer of the same size, alternated
    d, an = batches["equal"]
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, anchors=an, stream=s)
    flat = torch.randint(0, 2 ** 31 - 1, (N * map_bytes // 4,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        feed.reset()
        fb.feed(feed, stream=s)
        torch.cuda.synchronize()
        labels["launches"].append("versus")
        smh.crc32_device(v, flat.data_ptr(), N * map_bytes)
        torch.cuda.synchronize()
    labels["device"] = torch.cuda.get_device_name(0)
    with open(a.labels, "w") as f:
        json.dump(labels, f)
    print(json.dumps({k: labels[k] for k in labels if k != "launches"}))
    feed.close()
    fb.close()
    v.shutdown()


VIEW_SOURCES = (("ui_map", 0, 0), ("ocr_input", 1, 0), ("find_scales_input", 2, 0), ("lsd_preprocess", 3, 0), ("lsd_input", 4, 0), ("cropped_brq", 5, 0),
                ("ocr_input/four_lookups", 1, 4), ("lsd_input/four_lookups", 4, 4))


def workload_views(a):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    L = smh._lib
    W, H, N = 1920, 1080, a.frames
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, N, first_idx=0)
    d = torch.from_numpy(frames).cuda()
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos])
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    _, _, rw, rh = fb.roi
    map_bytes = rw * rh * 4
    feed = smh.WebFeed(v, 6 + N * (32 + ((10 + map_bytes + 15) & ~15) + 7 + 16 * 32 + 16), N)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors, stream=s)
    torch.cuda.synchronize()
    labels = {"frames": N, "map_w": rw, "map_h": rh, "launches": [], "sources": {}}
    for rnd in range(REPEATS):
        for name, which, form in VIEW_SOURCES:
            L.check(L.load().smhv_debug_feed_gray_form(form))
            feed.reset()
            fb.feed(feed, stream=s, map_source=which)
            torch.cuda.synchronize()
            labels["launches"].append(name)
            if rnd == 0:
                h = feed.header()
                w, hh = (rw, rh) if which in (0, 3, 4) else (rw // 2, rh // 2)
                labels["sources"][name] = {"map_source": which, "gray_form": form, "w": w, "h": hh, "n_maps": int(h.n_maps), "frames_done": int(h.frames_done)}
    L.check(L.load().smhv_debug_feed_gray_form(0))
    labels["device"] = torch.cuda.get_device_name(0)
    with open(a.labels, "w") as f:
        json.dump(labels, f)
    print(json.dumps({k: labels[k] for k in labels if k != "launches"}))
    feed.close()
    fb.close()
    v.shutdown()


def summarise_views(a):
    import statistics
    with open(a.labels) as f:
        lab = json.load(f)
    rows = sorted(csv.DictReader(open(a.kernel_trace)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    crc = [(r["Kernel_Name"], us(r)) for r in rows if "k_map_crc" in r["Kernel_Name"] or "k_view_crc" in r["Kernel_Name"]]
    maps = [(r["Kernel_Name"], us(r)) for r in rows if "k_feed_maps" in r["Kernel_Name"] or "k_feed_view_maps" in r["Kernel_Name"]]
    n_calls = len(lab["launches"])
    assert len(crc) == n_calls and len(maps) == n_calls, (len(crc), len(maps), n_calls)
    N = lab["frames"]
    out = {"device": lab.get("device"), "frames": N, "map": [lab["map_w"], lab["map_h"]], "repeats": REPEATS, "sources": {}}

    def stat(times, byts):
        med = statistics.median(times)
        return {"us": times, "median_us": med, "message_bytes": byts, "ps_per_message_byte": med * 1e6 / byts if byts else None,
                "spread_pct": 100.0 * (max(times) - min(times)) / med}

    for name, info in lab["sources"].items():
        ix = [i for i, l in enumerate(lab["launches"]) if l == name]
        px = info["w"] * info["h"] * 4
        e = dict(info)
        e["crc_kernel"] = sorted({crc[i][0] for i in ix})
        e["crc"] = stat([crc[i][1] for i in ix], N * px)
        e["maps_kernel"] = sorted({maps[i][0] for i in ix})
        e["maps"] = stat([maps[i][1] for i in ix], info["n_maps"] * px)
        out["sources"][name] = e
    y = out["sources"]["ui_map"]
    for name, e in out["sources"].items():
        for part in ("crc", "maps"):
            if e[part]["ps_per_message_byte"] is not None:
                ratio = e[part]["ps_per_message_byte"] / y[part]["ps_per_message_byte"]
                e[part]["against_ui_map_per_message_byte"] = ratio
                e[part]["slower_beyond_the_yardsticks_spread"] = ratio > 1.0 + y[part]["spread_pct"] / 100.0
    for plane in ("ocr_input", "lsd_input"):
        one, four = out["sources"][plane]["crc"], out["sources"][plane + "/four_lookups"]["crc"]
        out["sources"][plane]["crc"]["one_lookup_against_four_lookups"] = one["median_us"] / four["median_us"]
    s = json.dumps(out)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


def summarise(a):
    import statistics
    with open(a.labels) as f:
        lab = json.load(f)
    rows = sorted(csv.DictReader(open(a.kernel_trace)), key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        for k in ("k_map_crc", "k_feed_plan", "k_feed_maps", "k_feed_tables", "k_crc32"):
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    n_calls = len(lab["launches"])
    assert all(len(by.get(k, [])) == n_calls for k in ("k_map_crc", "k_feed_plan", "k_feed_maps")), {k: len(v) for k, v in by.items()}
    N, mb = lab["frames"], lab["map_bytes"]
    out = {"device": lab.get("device"), "frames": N, "map": [lab["map_w"], lab["map_h"]], "repeats": REPEATS, "achievable_TBps": ACHIEVABLE_TBPS, "workloads": {},
           "crc_mismatches": lab.get("crc_mismatches_of_%d" % N)}

    def rate(us, byts):
        return {"us": us, "median_us": statistics.median(us), "bytes": byts, "TBps": byts / statistics.median(us) / 1e6,
                "pct_of_achievable": 100.0 * byts / statistics.median(us) / 1e6 / ACHIEVABLE_TBPS}

    for name in WORKLOADS:
        ix = [i for i, l in enumerate(lab["launches"]) if l == name]
        w = dict(lab["workloads"][name])
        w["k_map_crc"] = rate([by["k_map_crc"][i] for i in ix], N * mb)
        w["k_feed_plan"] = {"us": [by["k_feed_plan"][i] for i in ix], "median_us": statistics.median(by["k_feed_plan"][i] for i in ix)}
        w["k_feed_maps"] = rate([by["k_feed_maps"][i] for i in ix], 2 * w["n_maps"] * mb)
        w["d2h_share_of_all_ui_maps_pct"] = 100.0 * w["d2h_bytes"] / w["all_ui_maps_bytes"]
        out["workloads"][name] = w
    ix = [i for i, l in enumerate(lab["launches"]) if l == "versus"]
    ours, theirs = [by["k_map_crc"][i] for i in ix], by.get("k_crc32", [])[-len(ix):]
    out["versus_k_crc32"] = {"bytes": N * mb, "k_map_crc_us": ours, "k_crc32_us": theirs,
                             "k_map_crc_ps_per_byte": statistics.median(ours) * 1e6 / (N * mb), "k_crc32_ps_per_byte": statistics.median(theirs) * 1e6 / (N * mb),
                             "ratio_of_medians": statistics.median(ours) / statistics.median(theirs),
                             "spread_pct": {"k_map_crc": 100.0 * (max(ours) - min(ours)) / statistics.median(ours),
                                            "k_crc32": 100.0 * (max(theirs) - min(theirs)) / statistics.median(theirs)}}
    out["k_feed_tables_us"] = by.get("k_feed_tables", [])
    s = json.dumps(out)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--labels", required=True)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", action="store_true", help="a debug view as the Map: smhv_batch_feed_view per source")
    a = ap.parse_args()
    if a.trace_only:
        (workload_views if a.views else workload)(a)
    else:
        if not a.kernel_trace:
            ap.error("--kernel-trace is required without --trace-only")
        (summarise_views if a.views else summarise)(a)


if __name__ == "__main__":
    main()
