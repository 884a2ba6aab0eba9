"""Cost of the map view (k_render_map, smhv_batch_render), measured on one GPU, one box.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/render_cost.py --workload --plan PLAN.json
  python tools/render_cost.py --rates --out RATES.json                         (profiler off)
  python tools/render_cost.py --parse DIR --plan PLAN.json --rates-json RATES.json [--bench BENCH.json] [--resources FILE] --out profiles/render_cost.json

256 x 1080p synthetic frames (16 distinct ones, repeated), the minimap rectangle = the whole ROI, three heightmaps: a uniformly
random and a terrain-like 4096^2 one and a random 1024^2 one.

--workload runs, `--reps` times over and alternated within the call, per map: one batch run with SMHV_STAGE_HEIGHTMAP_OVERLAY
(k_hm_overlay, the parent's kernel for the same picture) and one render at the identity viewport with SMHV_RENDER_HEIGHTMAP
(k_render_map: both write 256 ui-sized images from the same inputs); then the windows 1280 x 720 and 2560 x 1440 without
heightmap, with each map in each form of the tap fetch (gathers, LDS staging, the colour table in LDS), and with 32 lines per frame.  It writes the order
of its render launches to --plan; --parse matches the k_render_map dispatches of the kernel trace to it (they run on one stream,
in order) and reports every kernel time as a distribution.
--rates times the same renders with the profiler off (events around each launch) and reports frames per second.

The yardstick: k_render_map at the identity viewport against k_hm_overlay of the same run; both distributions are reported, and
`identity_vs_overlay` says whether the render's median lies within the overlay's own spread (max - min over its launches) of the
overlay's median.  Byte floor of a render without heightmap: sampled ui rows read + image written, over 6.29 TB/s."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBPS = 6.29
W, H, N = 1920, 1080, 256
MAPS = (("random4096", "random", 4096), ("smooth4096", "smooth", 4096), ("random1024", "random", 1024))
WINDOWS = ((1280, 720), (2560, 1440))


def heightmap_data(kind, side, rng):
    import numpy as np
    if kind == "random":
        return rng.integers(0, 65536, size=(side, side), dtype=np.uint16)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    h = 32768.0 + 12000.0 * np.sin(x / 300.0) * np.cos(y / 410.0) + 8000.0 * np.sin((x + y) / 170.0) + rng.uniform(0.0, 64.0, size=(side, side))
    return np.clip(h, 0, 65535).astype(np.uint16)


def setup():
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    v = smh.HipVision.init(0)
    rng = np.random.default_rng(0)
    out = {}
    for key, n_lines in (("plain", 2), ("lines32", 36)):
        frames, infos = synth.make_batch(W, H, 16, first_idx=5000 if n_lines > 2 else 0, n_lines=n_lines)
        d = torch.from_numpy(np.tile(frames, (N // 16, 1, 1, 1))).cuda()
        anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
        out[key] = (d, anchors)
    hms = {name: smh.Heightmap(v, heightmap_data(kind, side, rng), ((0, 0), (0, 0)), (1.0, 1.0, 50.0)) for name, kind, side in MAPS}
    return v, out, hms


def render_plan(rw, rh, reps):
    """The render launches of one call, in order: (label, window, zoom, map or None, markers, form, frames key)."""
    plan = []
    for _ in range(reps):
        for name, _, _ in MAPS:
            plan.append(dict(label="identity/%s" % name, out=[rw, rh], identity=True, map=name, markers=False, form=0, frames="plain", after_overlay=True))
    for _ in range(reps):
        for ow, oh in WINDOWS:
            plan.append(dict(label="%dx%d/none" % (ow, oh), out=[ow, oh], map=None, markers=False, form=0, frames="plain"))
            plan.append(dict(label="%dx%d/none/lines32" % (ow, oh), out=[ow, oh], map=None, markers=True, form=0, frames="lines32"))
            for name, _, _ in MAPS:
                for form in (1, 2, 3):
                    plan.append(dict(label="%dx%d/%s/form%d" % (ow, oh, name, form), out=[ow, oh], map=name, markers=False, form=form, frames="plain"))
        for name, _, _ in MAPS:
            for form in (1, 2, 3):
                plan.append(dict(label="identity/%s/form%d" % (name, form), out=[rw, rh], identity=True, map=name, markers=False, form=form, frames="plain"))
    return plan


def run_plan(a, timed):
    import torch
    import squad_mortar_helper_amd as smh
    L = smh._lib
    v, data, hms = setup()
    s = torch.cuda.current_stream().cuda_stream
    fbs = {}
    for key, (d, anchors) in data.items():
        fb = smh.FrameBatch(v, W, H, N)
        fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, anchors=anchors, stream=s)
        fbs[key] = fb
    _, _, rw, rh = fbs["plain"].roi
    recs = {k: smh.results_to_dicts(fb.read_results(0, N)) for k, fb in fbs.items()}
    info = dict(map=[rw, rh], ui_stride=int(fbs["plain"].layout.ui_stride), open_frames=sum(1 for r in recs["plain"] if r["map_open"]),
                frames_with_minimap=sum(1 for r in recs["plain"] if r["minimap"] is not None), minimap_of_frame_0=list(recs["plain"][0]["minimap"] or ()),
                lines_per_frame_lines32=float(sum(r["n_lines"] for r in recs["lines32"])) / N, device=torch.cuda.get_device_name(0) or getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""))
    plan = render_plan(rw, rh, a.reps)
    times = []
    ovl = smh.STAGE_UI_MAP | smh.STAGE_MARKERS | smh.STAGE_MINIMAP | smh.STAGE_HEIGHTMAP_OVERLAY
    d_plain, an_plain = data["plain"]
    for p in plan:
        fb = fbs[p["frames"]]
        hm = hms[p["map"]] if p["map"] else None
        if p.get("after_overlay"):
            fb.set_firing(hm)
            fb.run(d_plain.data_ptr(), N, stages=ovl, anchors=None, stream=s)     # k_hm_overlay of the same inputs
        ow, oh = p["out"]
        vp = smh.MapViewport.identity(rw, rh) if p.get("identity") else smh.MapViewport.calc(ow, oh, rw, rh)
        L.check(L.load().smhv_debug_render_form(p["form"]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed:
            e0.record()
        fb.render(vp, ow, oh, heightmap=hm, markers=p["markers"], stream=s)
        if timed:
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    L.check(L.load().smhv_debug_render_form(0))
    rules = {}
    for name, _, side in MAPS:
        for label, sw in (("identity", 1.0), ("1280x720", smh.MapViewport.calc(1280, 720, rw, rh).scale_factor_w), ("2560x1440", smh.MapViewport.calc(2560, 1440, rw, rh).scale_factor_w)):
            import ctypes as C
            ra, sr, tx, fm = C.c_float(), C.c_float(), C.c_uint32(), C.c_uint32()
            L.check(L.load().smhv_debug_render_rule(rw, rh, sw, sw, side, side, C.byref(ra), C.byref(sr), C.byref(tx), C.byref(fm)))
            rules["%s/%s" % (label, name)] = dict(texels_per_pixel=ra.value, switch_at=sr.value, lds_bytes=4 * tx.value, form=fm.value)
    info["rule"] = rules
    for fb in fbs.values():
        fb.close()
    for hm in hms.values():
        hm.close()
    v.shutdown()
    return plan, times, info


def dist(xs):
    xs = sorted(xs)
    n = len(xs)
    return dict(n=n, min=xs[0], median=xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2]), max=xs[-1], all=xs)


def floor_us(rw, rh, ow, oh, scale, ui_pitch_px):
    """Byte floor of a render without heightmap: the ui rows the quad samples (whole padded rows) + the image, at 6.29 TB/s."""
    rows = min(rh, int(min(oh, rh * scale)))
    byts = N * (rows * ui_pitch_px * 4.0 + ow * oh * 4.0)
    return byts, byts / (ACHIEVABLE_TBPS * 1e12) * 1e6


def parse(a):
    with open(a.plan) as f:
        saved = json.load(f)
    plan, info = saved["plan"], saved["info"]
    paths = glob.glob(os.path.join(a.parse, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_trace.csv under %s" % a.parse)
    rend, ovl, names = [], [], {}
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            k = r["Kernel_Name"]
            t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            short = k.split("(")[0].strip()
            names[short] = names.get(short, 0) + 1
            if "k_render_map" in k:
                rend.append((t0, (t1 - t0) / 1e3))
            elif "k_hm_overlay" in k:
                ovl.append((t0, (t1 - t0) / 1e3))
    rend.sort()
    ovl.sort()
    if len(rend) != len(plan):
        raise SystemExit("%d k_render_map dispatches in the trace, %d in the plan" % (len(rend), len(plan)))
    by = {}
    for p, (_, us) in zip(plan, rend):
        by.setdefault(p["label"], []).append(us)
    rw, rh = info["map"]
    out = dict(what="k_render_map against k_hm_overlay and its own variants; kernel times in us from one rocprofv3 --kernel-trace run, launches alternated",
               frames_per_launch=N, frame=[W, H], **info)
    out["kernel_us"] = {k: dist(v) for k, v in by.items()}
    n_id = sum(1 for p in plan if p.get("after_overlay"))
    per_map = {}
    for i, (name, _, _) in enumerate(MAPS):
        o = [us for j, (_, us) in enumerate(ovl[-n_id:]) if j % len(MAPS) == i]
        r_ = by["identity/%s" % name]
        do, dr = dist(o), dist(r_)
        spread = do["max"] - do["min"]
        per_map[name] = dict(k_hm_overlay_us=do, k_render_map_us=dr, overlay_spread_us=spread, render_minus_overlay_median_us=dr["median"] - do["median"],
                             speedup=do["median"] / dr["median"], not_slower_within_overlay_spread=bool(dr["median"] <= do["median"] + spread))
    out["identity_vs_overlay"] = per_map
    ui_pitch_px = info["ui_stride"] // 4 // rh
    floors = {}
    for ow, oh in WINDOWS:
        scale = min(ow / rw, oh / rh)
        byts, fl = floor_us(rw, rh, ow, oh, scale, ui_pitch_px)
        med = dist(by["%dx%d/none" % (ow, oh)])["median"]
        floors["%dx%d" % (ow, oh)] = dict(bytes=byts, floor_us_at_6p29=fl, kernel_us=med, pct_of_floor_rate=100.0 * fl / med)
    out["no_heightmap_byte_floor"] = floors
    if a.rates_json and os.path.exists(a.rates_json):
        with open(a.rates_json) as f:
            out["rates_profiler_off"] = json.load(f)
    if a.bench and os.path.exists(a.bench):
        with open(a.bench) as f:
            out["bench_default_run"] = json.load(f)
    if a.resources and os.path.exists(a.resources):
        with open(a.resources) as f:
            out["resources"] = json.load(f)
    out["kernels_in_trace"] = names
    s = json.dumps(out)
    print(s[:2000])
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--parse", default=None)
    ap.add_argument("--plan", default="render_plan.json")
    ap.add_argument("--rates-json", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parse:
        return parse(a)
    plan, times, info = run_plan(a, timed=a.rates)
    if a.workload:
        with open(a.plan, "w") as f:
            json.dump(dict(plan=plan, info=info), f)
        print(json.dumps(dict(render_launches=len(plan))))
        return
    by = {}
    for p, ms in zip(plan, times):
        by.setdefault(p["label"], []).append(ms)
    out = {k: dict(median_ms=dist(v)["median"], frames_per_s=N / (dist(v)["median"] * 1e-3), n=len(v)) for k, v in by.items()}
    s = json.dumps(out)
    print(s[:1500])
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
