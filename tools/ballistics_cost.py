"""What the ballistic map costs: smhv_batch_ballistic_map (k_ballistic_map + k_ballistic_finish) over 256 frames at a 1920 x 1080 window
with a 4096 x 4096 heightmap -- tools/reach_cost.py's job and size -- beside smhv_batch_reach (k_reach) with the same outputs in the same
process, the two taking turns in every round.

  python tools/ballistics_cost.py --out profiles/ballistics_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  Inside a leg the
two launches take turns in every round, each between two events on one stream, after WARMUP rounds that are not counted; the figure is
the median microseconds per call (the ballistic call is its kernel and the one-block-per-64-frames finish kernel behind it).  The weapon
is the library's default (the reach map's mortar), so both passes see the same ranges, the same out-of-range set and the same texels;
rings every 100 m for the reach map, isochrones every second for the ballistic map.  Bytes per pixel: PAINT reads and writes 4, the
class plane writes 1, the time-of-flight plane 4.  Per pixel the ballistic map adds one square root and one division (the time of
flight) and, with isochrones, a second division where the reach map's ring takes one; the JSON records both times and their ratio, and
sets no target.  Nothing depends on these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
HM = 4096
WARMUP, REPS = 3, 15
# paint, classes, tof -> bytes per pixel of the ballistic map, of the reach map
LEGS = {"classes": (False, True, False, 1.0, 1.0), "classes, tof": (False, True, True, 5.0, 1.0), "paint, classes": (True, True, False, 9.0, 9.0),
        "paint, classes, tof": (True, True, True, 13.0, 9.0), "classes, no isochrones or rings": (False, True, False, 1.0, 1.0)}


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    paint, classes, tof, bpp, reach_bpp = LEGS[name]
    lines = not name.endswith("or rings")
    v = smh.HipVision.init(0)
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
    _, _, rw, rh = fb.roi
    yy, xx = np.mgrid[0:HM, 0:HM]
    data = ((np.sin(xx / 310.0) * np.cos(yy / 170.0) * 0.5 + 0.5) * 30000.0 + ((xx * 7 + yy * 13) % 512)).astype(np.uint16)
    hm = smh.Heightmap(v, data, ((0, 0), (0, 0)), (1.0, 1.0, 60.0))
    vp = smh.MapViewport.calc(W, H, rw, rh)
    opt = smh.render_options(vp, W, H, markers=True)
    origin = (rw / 2.0, rh / 2.0)
    ro = smh.ReachOptions(origin=origin, ring_m=100.0 if lines else 0.0, paint=paint, classes=classes)
    bo = smh.BallisticOptions(origin=origin, iso_s=1.0 if lines else 0.0, paint=paint, classes=classes, tof=tof)
    weapon = smh.Weapon()
    cls = torch.zeros(N * W * H, dtype=torch.uint8, device="cuda")
    tofs = torch.zeros(N * W * H if tof else 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fb.render(vp, W, H, options=opt, stream=s)
    st.synchronize()
    t = dict(ballistic=[], reach=[])
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            fb.ballistic_map(opt, weapon, bo, heightmap=hm, classes_ptr=cls.data_ptr(), tof_ptr=tofs.data_ptr() if tof else None, stream=s)
            e[1].record()
            e[2].record()
            fb.reach(opt, ro, heightmap=hm, classes_ptr=cls.data_ptr(), stream=s)
            e[3].record()
            e[3].synchronize()
            if rep >= WARMUP:
                t["ballistic"].append(e[0].elapsed_time(e[1]) * 1e3)
                t["reach"].append(e[2].elapsed_time(e[3]) * 1e3)
    res, rres = fb.read_ballistic_map(0, N), fb.read_reach(0, N)
    out = dict(leg=name, device=torch.cuda.get_device_name(0), roi=[rw, rh], bytes_per_pixel=bpp, reach_bytes_per_pixel=reach_bpp,
               frames_with_origin=sum(int(res[f].valid) for f in range(N)), source_masks=sorted(set(int(res[f].source_mask) for f in range(N))),
               pixels_per_class_1_to_12=[sum(int(res[f].count[c]) for f in range(N)) for c in range(12)], isochrone_pixels=sum(int(res[f].iso) for f in range(N)),
               reach_pixels_per_class_1_to_9=[sum(int(rres[f].count[c]) for f in range(N)) for c in range(9)])
    for k, xs in t.items():
        xs = sorted(xs)
        out[k + "_us"] = dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])
    out["ballistic_over_reach"] = out["ballistic_us"]["median"] / out["reach_us"]["median"]
    out["ballistic_gb_per_s"] = N * W * H * bpp / (out["ballistic_us"]["median"] * 1e-6) / 1e9
    out["reach_gb_per_s"] = N * W * H * reach_bpp / (out["reach_us"]["median"] * 1e-6) / 1e9
    out["ballistic_ns_per_pixel"] = out["ballistic_us"]["median"] * 1e3 / (N * W * H)
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
    out = dict(what="smhv_batch_ballistic_map beside smhv_batch_reach: %d frames per call at a %d x %d window, a %d x %d heightmap, the default weapon, isochrones "
                    "every second and rings every 100 m; median microseconds per call of %d timed rounds after %d warm-up rounds, the two in turn; one child "
                    "process per leg" % (N, W, H, HM, HM, REPS, WARMUP), legs=legs, wall_s=round(time.time() - t0, 1))
    print(json.dumps({k: dict(ballistic_us=round(x["ballistic_us"]["median"], 1), reach_us=round(x["reach_us"]["median"], 1),
                              ratio=round(x["ballistic_over_reach"], 3), device=x["device"]) for k, x in legs.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
