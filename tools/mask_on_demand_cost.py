"""What making the marker mask's byte form on demand buys and costs, against the PARENT commit's build on the same box in one job.

  python tools/mask_on_demand_cost.py --parent <checkout of the parent commit, built> --rounds 3 --out profiles/mask_on_demand_cost.json

Per round, the parent first and this build second (so the rounds interleave), every measurement a fresh child process with a
time limit of its own; a child that fails or runs out of time ends the job, nothing is started after it.
  (a) the isolated launch: rocprofv3 --kernel-trace --stats over `bench.py --pipeline-depth 1` (the mean duration of k_map_brq_pass),
      and roofline.launch_ms of `bench.py --full`
  (b) the headline: `value` of the default bench.py run (config 2)
  (c) `bench.py --config 3`, and the real-samples leg of the --full run (1440p screenshots through k_map_pass)
  (d) this build only: k_mask_expand alone over 256 x 1080p frames (events round 20 launches), and a depth-12 frame-granular
      pipeline over the headline's shape with every slot lazy / every slot switched to eager (smhv_batch_device_ptrs with d_mask)
"faster" = every round of this build above every round of the parent, same box (ranges that do not overlap); the JSON says which
of (a), (b) hold that and lists every round's figure.  Nothing depends on these figures."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = ["--full", "--cpu-sample", "0", "--ingest-frames", "0", "--side-probe", "0", "--no-traffic-probe", "--no-depth1", "--no-back-to-back", "--steps", "10"]
W, H, N, DEPTH = 1920, 1080, 256, 12


def child(cmd, cwd, limit):
    """One measurement in a process of its own -> its stdout.  Any failure ends the job."""
    env = dict(os.environ)
    env.pop("SMH_VISION_HIP_LIB", None)
    try:
        r = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, text=True)
    except subprocess.TimeoutExpired:
        sys.exit("time limit of %d s: %s (in %s) -- nothing more is started" % (limit, " ".join(cmd), cwd))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit("exit %d: %s (in %s) -- nothing more is started" % (r.returncode, " ".join(cmd), cwd))
    return r.stdout


def bench(root, args, limit=400):
    out = child([sys.executable, os.path.join(root, "bench.py")] + args, root, limit)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def traced_pass_us(root, limit=300):
    """Mean duration of the fused streaming pass's launches of a depth-1 run, from the profiler's kernel statistics."""
    with tempfile.TemporaryDirectory() as d:
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.join(root, "bench.py"),
               "--pipeline-depth", "1", "--steps", "4", "--warmup", "1"], root, limit)
        hits = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not hits:
            sys.exit("no kernel statistics under %s" % d)
        with open(hits[0], newline="") as f:
            rows = [r for r in csv.DictReader(f) if "k_map_brq_pass" in r["Name"]]
    rows.sort(key=lambda r: -int(r["Calls"]))
    r = rows[0]
    return dict(kernel=r["Name"], calls=int(r["Calls"]), mean_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)


def leg_expand():
    """k_mask_expand alone: 20 launches between two events, after 3 that are not counted."""
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=2)
    d = torch.from_numpy(frames).cuda().repeat(N // 16, 1, 1, 1)
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL, anchors=anchors, stream=s)
    lib = smh._lib.load()
    ms = []
    for rep in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20 if rep else 3):
            smh._lib.check(lib.smhv_debug_mask_expand(fb._b, N, s))
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1) / 20)
    ly = fb.layout
    written = int(ly.mask_stride) * N
    print(json.dumps(dict(ms_per_launch=ms, bytes_written=written, bytes_read=written // 8, GBps=[(written + written // 8) / (m * 1e-3) / 1e9 for m in ms])))
    fb.close()
    v.shutdown()


def leg_pipeline(eager):
    """The headline's shape through a depth-12 frame-granular pipeline, 3 x 96 passes timed after 96: frames per second."""
    import time
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=2)
    d = torch.from_numpy(frames).cuda().repeat(N // 16, 1, 1, 1)
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    pipe = smh.Pipeline(v, W, H, N, DEPTH, search="frame")
    if eager:
        for b in pipe.slots:
            assert b.device_ptrs()["mask"]
    rates = []
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(96):
            pipe.submit(d.data_ptr(), N, stages=smh.STAGE_ALL, anchors=anchors)
        pipe.wait()
        torch.cuda.synchronize()
        if rep:
            rates.append(96 * N / (time.perf_counter() - t0))
    print(json.dumps(dict(eager=bool(eager), frames_per_s=rates, mask_state=[list(b.mask_state()) for b in pipe.slots[:2]])))
    pipe.close()
    v.shutdown()


def own_leg(name, limit=300):
    out = child([sys.executable, os.path.abspath(__file__), "--leg", name], ROOT, limit)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def real_value(j):
    rs = j.get("real_samples") or {}
    return rs.get("value", rs.get("frames_per_s"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.leg:
        return {"expand": leg_expand, "lazy": lambda: leg_pipeline(False), "eager": lambda: leg_pipeline(True)}[a.leg]()
    if not a.parent or not os.path.exists(os.path.join(a.parent, "bench.py")):
        ap.error("--parent: a checkout of the parent commit")
    builds = (("parent", os.path.abspath(a.parent)), ("this", ROOT))
    rounds = []
    for k in range(a.rounds):
        rec = {}
        for name, root in builds:
            head = bench(root, [])
            full = bench(root, FULL)
            c3 = bench(root, ["--config", "3", "--steps", "10"])
            rec[name] = dict(headline_value=head["value"], traced_pass=traced_pass_us(root), full_launch_ms=full["roofline"]["launch_ms"],
                             full_launch_is=full["roofline"].get("launch_is"), full_value=full["value"], config3_value=c3["value"],
                             real_samples_value=real_value(full), real_samples=full.get("real_samples"))
            print("round %d %s: headline %.0f, pass %.1f us traced / %.4f ms isolated, config 3 %.0f, real samples %s" % (
                k, name, head["value"], rec[name]["traced_pass"]["mean_us"], rec[name]["full_launch_ms"], c3["value"], rec[name]["real_samples_value"]), flush=True)
        rounds.append(rec)
        if a.out:                                             # (a job that is cut short keeps the rounds it has)
            with open(a.out + ".partial", "w") as f:
                f.write(json.dumps(rounds) + "\n")
    cost = dict(mask_expand_alone=own_leg("expand"), pipeline_lazy=own_leg("lazy"), pipeline_eager=own_leg("eager"))

    def col(name, key, sub=None):
        return [(r[name][key][sub] if sub else r[name][key]) for r in rounds]

    def apart(this, parent, higher_is_better):
        this, parent = [x for x in this if x is not None], [x for x in parent if x is not None]
        if not this or not parent:
            return None
        return min(this) > max(parent) if higher_is_better else max(this) < min(parent)
    verdict = {
        "a_traced_pass_shorter_in_every_round": apart(col("this", "traced_pass", "mean_us"), col("parent", "traced_pass", "mean_us"), False),
        "a_isolated_launch_ms_shorter_in_every_round": apart(col("this", "full_launch_ms"), col("parent", "full_launch_ms"), False),
        "b_headline_above_in_every_round": apart(col("this", "headline_value"), col("parent", "headline_value"), True),
        "c_config3_no_round_below_parents_lowest": min(col("this", "config3_value")) >= min(col("parent", "config3_value")),
        "c_real_samples_no_round_below_parents_lowest": (None if None in col("this", "real_samples_value") + col("parent", "real_samples_value")
                                                          else min(col("this", "real_samples_value")) >= min(col("parent", "real_samples_value"))),
    }
    import torch
    out = dict(what="the byte mask on demand against the parent commit: one job, one box, %d interleaved rounds (parent, this), every figure a child process" % a.rounds,
               device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, rounds=rounds, verdict=verdict, cost_to_a_host_that_asks=cost,
               summary={k: dict(parent=col("parent", k), this=col("this", k)) for k in ("headline_value", "full_launch_ms", "config3_value", "real_samples_value", "full_value")})
    out["summary"]["traced_pass_mean_us"] = dict(parent=col("parent", "traced_pass", "mean_us"), this=col("this", "traced_pass", "mean_us"))
    print(json.dumps(dict(verdict=verdict, summary=out["summary"], cost={k: {x: y for x, y in v.items() if x in ("ms_per_launch", "frames_per_s")} for k, v in cost.items()})))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        if os.path.exists(a.out + ".partial"):
            os.remove(a.out + ".partial")


if __name__ == "__main__":
    main()
