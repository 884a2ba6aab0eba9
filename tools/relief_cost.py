"""What the terrain relief costs: smhv_batch_relief (k_relief) over 256 frames at a 1920 x 1080 window with a 4096 x 4096 heightmap
in each of its forms, beside smhv_batch_reach with PAINT and CLASSES (k_reach<PAINT, CLASSES>, rings every 100 m) of the same window.

  python tools/relief_cost.py --out profiles/relief_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  Inside a leg the
two launches -- relief, reach -- take turns in every round, each between two events on one stream, after WARMUP rounds that are not
counted; the figure is the median microseconds per launch and per frame.  Bytes: PAINT reads and writes 4 per pixel, the flag and
the shade planes write 1 each, the heights 4; the PAINT leg's rate is held against the HBM peak.  The JSON names the box (host and
device) the figures are from: they hold for that box, and boxes differ by a few per cent.  Nothing depends on these figures."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
HM = 4096
WARMUP, REPS = 3, 15
HBM_PEAK_GB_S = 8000.0                                            # the MI355X's HBM3E, spec
# paint, (bytes, shades, heights), bytes moved per pixel, further options
LEGS = {
    "paint": (True, (False, False, False), 8.0, {}),
    "planes": (False, (True, True, True), 6.0, {}),
    "paint and planes": (True, (True, True, True), 14.0, {}),
    "summary alone": (False, (False, False, False), 0.0, {}),
    "paint, nearest": (True, (False, False, False), 8.0, dict(nearest=True)),
    "paint, no contours": (True, (False, False, False), 8.0, dict(interval_m=0.0)),
    "paint, no shade": (True, (False, False, False), 8.0, dict(shade_weight=0)),
}


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    paint, planes, bpp, extra = LEGS[name]
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
    del frames
    recs = smh.results_to_dicts(fb.read_results(0, N))
    _, _, rw, rh = fb.roi
    yy, xx = np.mgrid[0:HM, 0:HM]
    data = ((np.sin(xx / 310.0) * np.cos(yy / 170.0) * 0.5 + 0.5) * 30000.0 + ((xx * 7 + yy * 13) % 512)).astype(np.uint16)
    hm = smh.Heightmap(v, data, ((0, 0), (0, 0)), (1.0, 1.0, 60.0))
    vp = smh.MapViewport.calc(W, H, rw, rh)
    opt = smh.render_options(vp, W, H, markers=True)
    lo = smh.ReliefOptions(paint=paint, bytes=planes[0], shades=planes[1], heights=planes[2], **extra)
    ro = smh.ReachOptions(origin=(rw / 2.0, rh / 2.0), ring_m=100.0, paint=True, classes=True)
    cls = torch.zeros(N * W * H, dtype=torch.uint8, device="cuda")
    ptrs = dict(bytes_ptr=torch.zeros(N * W * H, dtype=torch.uint8, device="cuda") if planes[0] else None,
                shades_ptr=torch.zeros(N * W * H, dtype=torch.uint8, device="cuda") if planes[1] else None,
                heights_ptr=torch.zeros(N * W * H, dtype=torch.float32, device="cuda") if planes[2] else None)
    torch.cuda.synchronize()
    fb.render(vp, W, H, options=opt, stream=s)
    st.synchronize()
    t = dict(relief=[], reach=[])
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            fb.relief(opt, lo, heightmap=hm, stream=s, **{k: (p.data_ptr() if p is not None else None) for k, p in ptrs.items()})
            e[1].record()
            e[2].record()
            fb.reach(opt, ro, heightmap=hm, classes_ptr=cls.data_ptr(), stream=s)
            e[3].record()
            e[3].synchronize()
            if rep >= WARMUP:
                t["relief"].append(e[0].elapsed_time(e[1]) * 1e3)
                t["reach"].append(e[2].elapsed_time(e[3]) * 1e3)
    res = fb.read_relief(0, N)
    out = dict(leg=name, box=socket.gethostname(), device=torch.cuda.get_device_name(0), roi=[rw, rh], bytes_per_pixel=bpp, bytes=int(N * W * H * bpp),
               frames_valid=sum(int(res[f].valid) for f in range(N)), frames_with_minimap=sum(r["minimap"] is not None for r in recs),
               pixels_with_height=sum(int(res[f].n_height) for f in range(N)), contour_pixels=sum(int(res[f].n_contour) for f in range(N)),
               major_pixels=sum(int(res[f].n_major) for f in range(N)), pixels=N * W * H)
    for k, xs in t.items():
        xs = sorted(xs)
        out[k + "_us"] = dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])
        out[k + "_us_per_frame"] = xs[len(xs) // 2] / N
    out["relief_over_reach"] = out["relief_us"]["median"] / out["reach_us"]["median"]
    out["relief_ns_per_pixel"] = out["relief_us"]["median"] * 1e3 / (N * W * H)
    if bpp:
        out["relief_gb_per_s"] = out["bytes"] / (out["relief_us"]["median"] * 1e-6) / 1e9
        out["share_of_hbm_peak"] = out["relief_gb_per_s"] / HBM_PEAK_GB_S
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
        print(json.dumps({name: dict(relief_us_per_frame=round(legs[name]["relief_us_per_frame"], 2), reach_us_per_frame=round(legs[name]["reach_us_per_frame"], 2),
                                     relief_over_reach=round(legs[name]["relief_over_reach"], 3))}), flush=True)
    first = next(iter(legs.values()))
    out = dict(what="smhv_batch_relief: %d frames per launch at a %d x %d window, a %d x %d heightmap, the library's default options but for each leg's own; "
                    "median microseconds per launch of %d timed rounds after %d warm-up rounds; relief and smhv_batch_reach (PAINT | CLASSES, rings every "
                    "100 m) in turn; one child process per leg; hbm peak %g GB/s" % (N, W, H, HM, HM, REPS, WARMUP, HBM_PEAK_GB_S),
               box=first["box"], device=first["device"], legs=legs, wall_s=round(time.time() - t0, 1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
