"""What the reach map costs: smhv_batch_reach (k_reach) over 256 frames at a 1920 x 1080 window with a 4096 x 4096 heightmap, rings
every 100 m -- PAINT, CLASSES and both -- beside a plain device copy that reads and writes the same number of bytes and beside
smhv_batch_render of the same window.

  python tools/reach_cost.py --out profiles/reach_cost.json

Every leg (paint, classes, both, and both without rings) is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends
the job.  Inside a leg the three launches -- reach, copy, render -- take turns in every round, each between two events on one
stream, after WARMUP rounds that are not counted; the figure is the median microseconds per launch.  Bytes: PAINT reads and writes
4 per pixel, CLASSES writes 1; the copy (hipMemcpyAsync, device to device) moves half of the sum so that it reads and writes as
much in all.  The origin is a point in the middle of the map, so the window holds the heightmap's ranges inside the minimap
rectangle and the scales' outside it; the JSON says which sources and classes the frames held.  Nothing depends on these figures."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
HM = 4096
WARMUP, REPS = 3, 15
LEGS = {"paint": (True, False, 8.0), "classes": (False, True, 1.0), "both": (True, True, 9.0), "both, no rings": (True, True, 9.0)}   # paint, classes, bytes per pixel


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    paint, classes, bpp = LEGS[name]
    v = smh.HipVision.init(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    frames16, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=4)
    few = torch.from_numpy(frames16).cuda()
    frames = few[torch.arange(N, device="cuda") % 16].contiguous()
    del few
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    torch.cuda.synchronize()
    fb.run(frames.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors, stream=s)
    st.synchronize()
    recs = smh.results_to_dicts(fb.read_results(0, N))
    _, _, rw, rh = fb.roi
    yy, xx = np.mgrid[0:HM, 0:HM]
    data = ((np.sin(xx / 310.0) * np.cos(yy / 170.0) * 0.5 + 0.5) * 30000.0 + ((xx * 7 + yy * 13) % 512)).astype(np.uint16)
    hm = smh.Heightmap(v, data, ((0, 0), (0, 0)), (1.0, 1.0, 60.0))
    vp = smh.MapViewport.calc(W, H, rw, rh)
    opt = smh.render_options(vp, W, H, markers=True)
    ro = smh.ReachOptions(origin=(rw / 2.0, rh / 2.0), ring_m=0.0 if name.endswith("no rings") else 100.0, paint=paint, classes=classes)
    cls = torch.zeros(N * W * H if classes else 4, dtype=torch.uint8, device="cuda")
    half = int(N * W * H * bpp) // 2
    scratch = torch.zeros(2 * half + 512, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fb.render(vp, W, H, options=opt, stream=s)
    st.synchronize()
    t = dict(reach=[], copy=[], render=[])
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            e[0].record()
            fb.reach(opt, ro, heightmap=hm, classes_ptr=cls.data_ptr() if classes else None, stream=s)
            e[1].record()
            e[2].record()
            assert hip.hipMemcpyAsync(C.c_void_p(scratch.data_ptr() + half + (-half) % 256), C.c_void_p(scratch.data_ptr()), half, 3, C.c_void_p(s)) == 0
            e[3].record()
            e[4].record()
            fb.render(vp, W, H, options=opt, stream=s)
            e[5].record()
            e[5].synchronize()
            if rep >= WARMUP:
                t["reach"].append(e[0].elapsed_time(e[1]) * 1e3)
                t["copy"].append(e[2].elapsed_time(e[3]) * 1e3)
                t["render"].append(e[4].elapsed_time(e[5]) * 1e3)
    res = fb.read_reach(0, N)
    counts = [sum(int(res[f].count[c]) for f in range(N)) for c in range(9)]
    out = dict(leg=name, device=torch.cuda.get_device_name(0), roi=[rw, rh], bytes_per_pixel=bpp, bytes=int(N * W * H * bpp),
               frames_with_origin=sum(int(res[f].valid) for f in range(N)), frames_with_minimap=sum(r["minimap"] is not None for r in recs),
               frames_with_mpx=sum(r["mpx"] is not None for r in recs), source_masks=sorted(set(int(res[f].source_mask) for f in range(N))),
               pixels_per_class_1_to_9=counts, ring_pixels=sum(int(res[f].ring) for f in range(N)))
    for k, xs in t.items():
        xs = sorted(xs)
        out[k + "_us"] = dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])
    out["reach_over_copy"] = out["reach_us"]["median"] / out["copy_us"]["median"]
    out["reach_over_render"] = out["reach_us"]["median"] / out["render_us"]["median"]
    out["reach_gb_per_s"] = out["bytes"] / (out["reach_us"]["median"] * 1e-6) / 1e9
    out["copy_gb_per_s"] = out["bytes"] / (out["copy_us"]["median"] * 1e-6) / 1e9
    out["reach_ns_per_pixel"] = out["reach_us"]["median"] * 1e3 / (N * W * H)
    print(json.dumps(out))
    hm.close()
    fb.close()
    v.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.leg:
        return leg(a.leg)
    t0 = time.time()
    legs = {}
    for name in LEGS:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--leg", name], cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit("leg %s: exit %d: the measurement failed%s" % (name, r.returncode, " (the time limit)" if r.returncode in (124, 137) else ""))
        legs[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    out = dict(what="smhv_batch_reach: %d frames per launch at a %d x %d window, a %d x %d heightmap, rings every 100 m; median microseconds per launch of %d "
                    "timed rounds after %d warm-up rounds; reach, a device copy of the same bytes and smhv_batch_render in turn; one child process per leg"
                    % (N, W, H, HM, HM, REPS, WARMUP), legs=legs, wall_s=round(time.time() - t0, 1))
    print(json.dumps({k: dict(reach_us=round(x["reach_us"]["median"], 1), copy_us=round(x["copy_us"]["median"], 1), render_us=round(x["render_us"]["median"], 1),
                              reach_ns_per_pixel=round(x["reach_ns_per_pixel"], 4), source_masks=x["source_masks"]) for k, x in legs.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
