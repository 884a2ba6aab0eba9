"""What the terrain clearance costs: smhv_batch_clearance_map (k_clear_map<false, true>: BYTES, no paint) at a 1920 x 1080 and a
1280 x 720 window for S = 16, 64 and 256 on a 4096 x 4096 heightmap, beside smhv_batch_reach with CLASSES (k_reach<false, true>) of
the same window from the same process, and smhv_batch_clearance (k_clear_lines) over 256 frames x 32 line slots.

  python tools/clearance_cost.py --out profiles/clearance_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  Inside a leg
the launches -- the three sample counts and the reach map -- take turns in every round, each between two events on one stream, after
WARMUP rounds that are not counted; the figure is the median microseconds per launch.  A map launch covers FRAMES frames of the
256-frame batch.  Frames whose record has no minimap rectangle have no heightmap branch and march nothing: the ns per sample is
taken over the frames that have one.  The leg "1920x1080, 64 x 64 heightmap" repeats the first with a heightmap that fits a CU's L1
many times over: where its times equal the 4096 x 4096 leg's, the gathers are not what bounds the kernel.  The origin is a point in
the middle of the map.  Nothing depends on these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
FRAMES = 64
WARMUP, REPS = 2, 7
SAMPLES = (16, 64, 256)
LEGS = {"1920x1080": (1920, 1080, 4096), "1280x720": (1280, 720, 4096), "1920x1080, 64 x 64 heightmap": (1920, 1080, 64), "lines": None}


def _stat(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    v = smh.HipVision.init(0)
    frames16, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=4)
    few = torch.from_numpy(frames16).cuda()
    frames = few[torch.arange(N, device="cuda") % 16].contiguous()
    del few
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    torch.cuda.synchronize()
    fb.run(frames.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors, stream=s)
    st.synchronize()
    recs = smh.results_to_dicts(fb.read_results(0, N))
    _, _, rw, rh = fb.roi
    hm_n = 4096 if LEGS[name] is None else LEGS[name][2]
    yy, xx = np.mgrid[0:hm_n, 0:hm_n]
    data = ((np.sin(xx / 310.0) * np.cos(yy / 170.0) * 0.5 + 0.5) * 30000.0 + ((xx * 7 + yy * 13) % 512)).astype(np.uint16)
    hm = smh.Heightmap(v, data, ((0, 0), (0, 0)), (1.0, 1.0, 60.0))
    out = dict(leg=name, device=torch.cuda.get_device_name(0), roi=[rw, rh], heightmap=[hm_n, hm_n])
    if LEGS[name] is None:                                         # k_clear_lines: every frame of the batch, S = 64 and 256, with and without profiles
        prof = torch.zeros((N, 32, 257), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t = {}
        with torch.cuda.stream(st):
            for rep in range(WARMUP + REPS):
                for S in (64, 256):
                    for with_prof in (False, True):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fb.clearance(smh.ClearanceOptions(samples=S), heightmap=hm, profiles_ptr=prof.data_ptr() if with_prof else None, stream=s)
                        e1.record()
                        e1.synchronize()
                        if rep >= WARMUP:
                            t.setdefault("S=%d%s" % (S, ", profiles" if with_prof else ""), []).append(e0.elapsed_time(e1) * 1e3)
        res = fb.read_clearance(0, N)
        live = sum(int(res[f].n_lines) for f in range(N))
        verdicts = sum(1 for f in range(N) for l in range(int(res[f].n_lines)) if res[f].line[l].dir[0].status != 0)
        out.update(frames=N, line_slots=N * 32, lines_in_the_records=live, lines_with_a_verdict=verdicts, launch_us={k: _stat(x) for k, x in t.items()})
        out["ns_per_line_slot"] = {k: x["median"] * 1e3 / (N * 32) for k, x in out["launch_us"].items()}
    else:
        w, h, _ = LEGS[name]
        vp = smh.MapViewport.calc(w, h, rw, rh)
        opt = smh.render_options(vp, w, h, markers=True)
        origin = (rw / 2.0, rh / 2.0)
        buf = torch.zeros(FRAMES * w * h, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ro = smh.ReachOptions(origin=origin, ring_m=0.0, paint=False, classes=True)
        t = {}
        with torch.cuda.stream(st):
            for rep in range(WARMUP + REPS):
                for S in SAMPLES + ("reach",):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if S == "reach":
                        fb.reach(opt, ro, first=0, n=FRAMES, heightmap=hm, classes_ptr=buf.data_ptr(), stream=s)
                    else:
                        fb.clearance_map(opt, smh.ClearanceOptions(samples=S, origin=origin, paint=False, bytes=True), first=0, n=FRAMES, heightmap=hm,
                                         bytes_ptr=buf.data_ptr(), stream=s)
                    e1.record()
                    e1.synchronize()
                    if rep >= WARMUP:
                        t.setdefault(S, []).append(e0.elapsed_time(e1) * 1e3)
        res = fb.read_clearance_map(0, FRAMES)                     # (of the last clearance launch: S = 256)
        marching = sum(1 for r in recs[:FRAMES] if r["minimap"] is not None and r["map_open"])
        out.update(window=[w, h], frames=FRAMES, frames_that_march=marching,
                   pixels_per_status_1_to_3=[sum(int(res[f].count[c]) for f in range(FRAMES)) for c in range(3)],
                   los_pixels=sum(int(res[f].los_blocked) for f in range(FRAMES)), reach_us=_stat(t["reach"]), clear_us={"S=%d" % S: _stat(t[S]) for S in SAMPLES})
        out["reach_us_per_frame"] = out["reach_us"]["median"] / FRAMES
        out["clear_us_per_frame"] = {k: x["median"] / FRAMES for k, x in out["clear_us"].items()}
        out["clear_over_reach"] = {k: x["median"] / out["reach_us"]["median"] for k, x in out["clear_us"].items()}
        out["ns_per_sample"] = {"S=%d" % S: (_stat(t[S])["median"] * 1e3 / (marching * w * h * (S - 1)) if marching else None) for S in SAMPLES}
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
    out = dict(what="smhv_batch_clearance_map with BYTES (k_clear_map<false, true>): %d frames per launch of a batch of %d 1080p frames, S = 16 / 64 / 256, beside "
                    "smhv_batch_reach with CLASSES (k_reach<false, true>) of the same window; smhv_batch_clearance (k_clear_lines) over %d frames x 32 line slots; "
                    "median microseconds per launch of %d timed rounds after %d warm-up rounds, the launches of a leg in turn; one child process per leg"
                    % (FRAMES, N, N, REPS, WARMUP), legs=legs, wall_s=round(time.time() - t0, 1))
    print(json.dumps({k: (dict(clear_us_per_frame={s: round(x, 1) for s, x in leg_["clear_us_per_frame"].items()}, reach_us_per_frame=round(leg_["reach_us_per_frame"], 1),
                               ns_per_sample=leg_["ns_per_sample"]) if "window" in leg_ else leg_["launch_us"]) for k, leg_ in legs.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
