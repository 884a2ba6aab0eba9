"""What the ballistic clearance costs beside the one-arc kernel: smhv_batch_ballistic_clearance_map with BYTES (k_bclear_map<false,
true>) at a 1920 x 1080 and a 1280 x 720 window for S = 16, 64 and 256 on a 4096 x 4096 heightmap, and smhv_batch_clearance_map with
BYTES (k_clear_map<false, true>) with the same inputs and launches, interleaved in the same process; smhv_batch_ballistic_clearance
(k_bclear_lines) beside smhv_batch_clearance (k_clear_lines) over 256 frames x 32 line slots.  The weapon is smhv_weapon_defaults, so
the high arc both kernels march is the same arc.

  python tools/ballistic_clearance_cost.py --out profiles/ballistic_clearance_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  Inside a leg the
launches -- both kernels at the three sample counts -- take turns in every round, each between two events on one stream, after WARMUP
rounds that are not counted; the figure is the median microseconds per launch.  A map launch covers FRAMES frames of the 256-frame
batch.  The number that matters is `ratio`: two arcs over one at equal S.  A caller's alternative is two one-arc passes, so the design
goal is a ratio below 2.0; it is a goal and not a gate, and nothing depends on these figures."""
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
LEGS = {"1920x1080": (1920, 1080), "1280x720": (1280, 720), "lines": None}


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
    yy, xx = np.mgrid[0:4096, 0:4096]
    data = ((np.sin(xx / 310.0) * np.cos(yy / 170.0) * 0.5 + 0.5) * 30000.0 + ((xx * 7 + yy * 13) % 512)).astype(np.uint16)
    hm = smh.Heightmap(v, data, ((0, 0), (0, 0)), (1.0, 1.0, 60.0))
    weapon = smh.Weapon()
    out = dict(leg=name, device=torch.cuda.get_device_name(0), roi=[rw, rh], heightmap=[4096, 4096])
    t = {}

    def timed(key, rep, call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if rep >= WARMUP:
            t.setdefault(key, []).append(e0.elapsed_time(e1) * 1e3)
    if LEGS[name] is None:                                         # the lines kernels: every frame of the batch, S = 64 and 256
        with torch.cuda.stream(st):
            for rep in range(WARMUP + REPS):
                for S in (64, 256):
                    timed(("one", S), rep, lambda: fb.clearance(smh.ClearanceOptions(samples=S), heightmap=hm, stream=s))
                    timed(("two", S), rep, lambda: fb.ballistic_clearance(weapon, smh.BallisticClearanceOptions(samples=S), heightmap=hm, stream=s))
        res = fb.read_ballistic_clearance(0, N)
        live = sum(int(res[f].n_lines) for f in range(N))
        verdicts = sum(1 for f in range(N) for l in range(int(res[f].n_lines)) if res[f].line[l].dir[0].valid)
        out.update(frames=N, line_slots=N * 32, lines_in_the_records=live, lines_with_a_verdict=verdicts,
                   one_arc_us={"S=%d" % S: _stat(t[("one", S)]) for S in (64, 256)}, two_arc_us={"S=%d" % S: _stat(t[("two", S)]) for S in (64, 256)})
        out["ratio"] = {k: out["two_arc_us"][k]["median"] / out["one_arc_us"][k]["median"] for k in out["one_arc_us"]}
    else:
        w, h = LEGS[name]
        vp = smh.MapViewport.calc(w, h, rw, rh)
        opt = smh.render_options(vp, w, h, markers=True)
        origin = (rw / 2.0, rh / 2.0)
        buf = torch.zeros(FRAMES * w * h, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for rep in range(WARMUP + REPS):
                for S in SAMPLES:
                    timed(("one", S), rep, lambda: fb.clearance_map(opt, smh.ClearanceOptions(samples=S, origin=origin, paint=False, bytes=True), first=0, n=FRAMES,
                                                                    heightmap=hm, bytes_ptr=buf.data_ptr(), stream=s))
                    timed(("two", S), rep, lambda: fb.ballistic_clearance_map(opt, weapon, smh.BallisticClearanceOptions(samples=S, origin=origin, paint=False, bytes=True),
                                                                              first=0, n=FRAMES, heightmap=hm, bytes_ptr=buf.data_ptr(), stream=s))
        res = fb.read_ballistic_clearance_map(0, FRAMES)           # (of the last launch: S = 256)
        ref = fb.read_clearance_map(0, FRAMES)
        marching = sum(1 for r in recs[:FRAMES] if r["minimap"] is not None and r["map_open"])
        own = [sum(int(res[f].own[c]) for f in range(FRAMES)) for c in range(4)]
        one = [sum(int(ref[f].count[c]) for f in range(FRAMES)) for c in range(3)]
        # the tie of the tests, on the measured launches: out of range, clear and blocked pixels of the high arc are the one-arc kernel's
        assert (own[0], own[2], own[3]) == tuple(one) and own[1] == 0, (own, one)
        out.update(window=[w, h], frames=FRAMES, frames_that_march=marching, own_pixels_per_class_1_to_4=own,
                   other_pixels_per_class_1_to_4=[sum(int(res[f].other[c]) for f in range(FRAMES)) for c in range(4)],
                   one_arc_us={"S=%d" % S: _stat(t[("one", S)]) for S in SAMPLES}, two_arc_us={"S=%d" % S: _stat(t[("two", S)]) for S in SAMPLES})
        out["ratio"] = {k: out["two_arc_us"][k]["median"] / out["one_arc_us"][k]["median"] for k in out["one_arc_us"]}
        out["two_arc_us_per_frame"] = {k: x["median"] / FRAMES for k, x in out["two_arc_us"].items()}
        out["ns_per_sample"] = {kind: {"S=%d" % S: (_stat(t[(kind, S)])["median"] * 1e3 / (marching * w * h * (S - 1)) if marching else None) for S in SAMPLES}
                                for kind in ("one", "two")}
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
    out = dict(what="smhv_batch_ballistic_clearance_map with BYTES (k_bclear_map<false, true>, both arcs) beside smhv_batch_clearance_map with BYTES (k_clear_map<false, "
                    "true>, one arc): %d frames per launch of a batch of %d 1080p frames, S = 16 / 64 / 256, the default weapon; smhv_batch_ballistic_clearance beside "
                    "smhv_batch_clearance over %d frames x 32 line slots; median microseconds per launch of %d timed rounds after %d warm-up rounds, the launches of a "
                    "leg in turn; one child process per leg; ratio = two arcs over one at equal S (design goal, not a gate: below 2.0)" % (FRAMES, N, N, REPS, WARMUP),
               legs=legs, ratio={k: leg_["ratio"] for k, leg_ in legs.items()}, wall_s=round(time.time() - t0, 1))
    print(json.dumps(out["ratio"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
