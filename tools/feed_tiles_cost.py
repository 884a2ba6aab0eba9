"""Cost of the feed's map tiles (smhv_batch_feed_tiles) against the plain feed (smhv_batch_feed) on the same frames, on one GPU.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/feed_tiles_cost.py --trace-only --labels LABELS.json
  python tools/feed_tiles_cost.py --kernel-trace DIR/.../*_kernel_trace.csv --labels LABELS.json [--out profiles/feed_tiles_cost.json]

The first form is the workload, run under the profiler in a run of its own (no counters in it): 256 resident 1080p frames in three
scenes, each frame made from its predecessor on the device --
  one     one more tile changed (one pixel of it)
  tenth   every tenth tile changed (83 of 832), another tenth in every frame
  all     every tile changed
-- and per scene, after one warm-up call of each kind, five alternated rounds of one smhv_batch_feed_tiles call and one
smhv_batch_feed call over the 256 frames, the feed reset before every call.  For the scenes `one` and `tenth` it replays the tile
call's messages through MapTexture and holds the texture against the last frame's ui_map read back.  It writes LABELS.json: the
order of the calls and what each left in the header.

The second form needs no GPU: it reads the trace's per-dispatch times in launch order and reports per scene the median time of
every kernel of both paths, their sums and the ratio, bytes_used of both, k_tiles_diff's bytes (two maps per frame that has a base
and another CRC) and rate, and k_tiles_diff against k_map_crc.  Prints one JSON object."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBPS = 6.29
SCENES = ("one", "tenth", "all")
REPEATS = 5
TILE_KERNELS = ("k_map_crc", "k_tiles_base", "k_tiles_diff", "k_tiles_plan", "k_tiles_copy", "k_feed_maps", "k_tiles_keep")
PLAIN_KERNELS = ("k_map_crc", "k_feed_plan", "k_feed_maps")


def scene_frames(base, roi, which, n):
    """n frames on the device, frame i made from frame i - 1: (v, v, v) written into the first pixel of the scene's tiles."""
    import torch
    rx, ry, rw, rh = roi
    tx, ty = -(-rw // 64), -(-rh // 16)
    ys = (ry + 16 * torch.arange(ty, device="cuda")).repeat_interleave(tx)
    xs = (rx + 64 * torch.arange(tx, device="cuda")).repeat(ty)
    t = torch.arange(tx * ty, device="cuda")
    frames = base.unsqueeze(0).repeat(n, 1, 1, 1)
    for i in range(1, n):
        sel = (t == (i - 1) % (tx * ty)) if which == "one" else ((t + i) % 10 == 0) if which == "tenth" else (t >= 0)
        frames[i:, ys[sel], xs[sel], :3] = 60 + i % 80                # (terrain grey: never a marker colour; another value than ten frames ago)
    return frames, int(((t + 1) % 10 == 0).sum()) if which == "tenth" else (1 if which == "one" else tx * ty)


def workload(a):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    W, H, N = 1920, 1080, a.frames
    v = smh.HipVision.init(0)
    frame, _ = synth.make_frame(W, H, frame_idx=0)
    base = torch.from_numpy(frame).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    roi = tuple(fb.roi)
    map_bytes = roi[2] * roi[3] * 4
    feed = smh.WebFeed(v, 6 + N * (32 + ((10 + map_bytes + 15) & ~15) + 7 + 16 * 32 + 16), N)
    labels = {"frames": N, "map_w": roi[2], "map_h": roi[3], "map_bytes": map_bytes, "launches": [], "scenes": {}}
    for name in SCENES:
        frames, per_frame = scene_frames(base, roi, name, N)
        fb.run(frames.data_ptr(), N, stages=smh.STAGE_MARKERS | smh.STAGE_UI_MAP, grayscale=False, stream=s)
        torch.cuda.synchronize()
        heads = {}
        for rnd in range(REPEATS + 1):                                # round 0 warms both paths up and is not timed
            for kind in ("tiles", "plain"):
                feed.reset()
                (fb.feed_tiles if kind == "tiles" else fb.feed)(feed, stream=s)
                torch.cuda.synchronize()
                labels["launches"].append([name, kind, rnd])
                if rnd == 0:
                    h = feed.header()
                    heads[kind] = {"n_entries": int(h.n_entries), "n_maps": int(h.n_maps), "frames_done": int(h.frames_done), "bytes_used": int(h.bytes_used)}
                    if kind == "tiles" and name != "all":             # the stream at the size the timing is taken at
                        tex = smh.MapTexture()
                        _, msgs = feed.read()
                        for _, k, _, data in msgs:
                            if k in (smh.WEB_MAP, smh.WEB_MAP_TILES):
                                tex.apply(data)
                        assert tex.map.tobytes() == fb.read_image(smh._lib.IMAGE_UI_MAP, N - 1).tobytes(), name
                        heads["replayed"] = True
        heads["tiles_changed_per_frame"] = per_frame
        labels["scenes"][name] = heads
        del frames
    labels["device"] = torch.cuda.get_device_name(0)
    with open(a.labels, "w") as f:
        json.dump(labels, f)
    print(json.dumps({k: labels[k] for k in labels if k != "launches"}))
    feed.close()
    fb.close()
    v.shutdown()


def summarise(a):
    with open(a.labels) as f:
        lab = json.load(f)
    rows = sorted(csv.DictReader(open(a.kernel_trace)), key=lambda r: int(r["Start_Timestamp"]))
    names = sorted(set(TILE_KERNELS) | set(PLAIN_KERNELS), key=len, reverse=True)
    seq = []
    for r in rows:
        k = next((k for k in names if k in r["Kernel_Name"]), None)
        if k:
            seq.append((k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    calls, at = [], 0
    for name, kind, rnd in lab["launches"]:                           # the kernels of every call, in launch order
        want = TILE_KERNELS if kind == "tiles" else PLAIN_KERNELS
        got = seq[at:at + len(want)]
        assert [k for k, _ in got] == list(want), (name, kind, rnd, got)
        calls.append((name, kind, rnd, dict(got)))
        at += len(want)
    assert at == len(seq), (at, len(seq))
    N, mb = lab["frames"], lab["map_bytes"]
    out = {"device": lab.get("device"), "frames": N, "map": [lab["map_w"], lab["map_h"]], "repeats": REPEATS, "achievable_TBps": ACHIEVABLE_TBPS, "scenes": {}}
    for name in SCENES:
        e = dict(lab["scenes"][name])
        for kind, kernels in (("tiles", TILE_KERNELS), ("plain", PLAIN_KERNELS)):
            mine = [c[3] for c in calls if c[0] == name and c[1] == kind and c[2] > 0]
            per = {k: [c[k] for c in mine] for k in kernels}
            sums = [sum(c.values()) for c in mine]
            e[kind + "_path"] = {"kernels_median_us": {k: statistics.median(v) for k, v in per.items()}, "sum_us": sums, "sum_median_us": statistics.median(sums),
                                 "sum_spread_pct": 100.0 * (max(sums) - min(sums)) / statistics.median(sums)}
        t, p = e["tiles_path"], e["plain_path"]
        e["tiles_over_plain_kernel_time"] = t["sum_median_us"] / p["sum_median_us"]
        e["tiles_over_plain_bytes_used"] = e["tiles"]["bytes_used"] / e["plain"]["bytes_used"]
        diff_bytes = 2 * (N - 1) * mb                                  # every frame but the first has a base and another CRC
        d_us, c_us = t["kernels_median_us"]["k_tiles_diff"], t["kernels_median_us"]["k_map_crc"]
        e["k_tiles_diff"] = {"bytes_read": diff_bytes, "TBps": diff_bytes / d_us / 1e6, "pct_of_achievable": 100.0 * diff_bytes / d_us / 1e6 / ACHIEVABLE_TBPS,
                             "over_k_map_crc_time": d_us / c_us, "ps_per_byte": d_us * 1e6 / diff_bytes, "k_map_crc_ps_per_byte": c_us * 1e6 / (N * mb)}
        out["scenes"][name] = e
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
    a = ap.parse_args()
    if a.trace_only:
        workload(a)
    else:
        if not a.kernel_trace:
            ap.error("--kernel-trace is required without --trace-only")
        summarise(a)


if __name__ == "__main__":
    main()
