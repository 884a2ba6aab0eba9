"""What writing the grey ui_map as a luma plane buys and costs, against the PARENT commit's build on the same box in one job.

  python tools/ui_on_demand_cost.py --parent <checkout of the parent commit> --rounds 3 --out profiles/ui_on_demand_cost.json \\
      --pmc-out profiles/ui_on_demand_pmc_summary.txt

Both trees are built first where their library is missing (make in csrc: build where no GPU time is spent if you can).  Per round, the
parent first and this build second (so the rounds interleave), every measurement a fresh child process under `timeout -k 10` with a
limit of its own; a child that fails or runs out of time ends the job, nothing is started after it.
  (a) the isolated launch: rocprofv3 --kernel-trace --stats over `bench.py --pipeline-depth 1` (the mean duration of the grey fused
      streaming kernel: k_map_brq_pass in the parent, k_map_brq_pass_luma here), and roofline.launch_ms of `bench.py --full`
  (b) the headline: `value` of the default bench.py run (config 2)
  (c) `bench.py --config 3`
  (d) the real-samples leg of the --full run (1440p screenshots in COLOUR: the path this change must not slow down)
  once: `bench.py --config 4` on one GPU, both builds
  a pair of runs of their own per build: rocprofv3 --pmc WRITE_SIZE / --pmc FETCH_SIZE over bench.py's traffic child (three plain
      256 x 1080p passes, nothing else): the bytes of the launch, reads = 2 x FETCH_SIZE (the gfx950 correction)
  this build only, what a host pays that does ask: k_ui_expand alone over 256 x 1080p frames, and a depth-12 frame-granular pipeline
      over the headline's shape with every slot lazy / every slot switched to eager (smhv_batch_device_ptrs with d_ui)
The verdict: (a) shorter in every round, (b) higher in every round with ranges apart, (c) / (d) no round below the parent's lowest.
Nothing depends on these figures."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = ["--full", "--cpu-sample", "0", "--ingest-frames", "0", "--side-probe", "0", "--no-traffic-probe", "--no-depth1", "--no-back-to-back", "--steps", "10"]
W, H, N, DEPTH = 1920, 1080, 256, 12
T0 = time.time()
SPENT = []                                                             # (what, seconds) of every child, for whoever sizes the next job


def child(cmd, cwd, limit, what):
    """One measurement in a process of its own, under `timeout -k 10` -> its stdout.  Any failure ends the job."""
    env = dict(os.environ)
    env.pop("SMH_VISION_HIP_LIB", None)
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    SPENT.append((what, round(time.time() - t, 1)))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit("exit %d%s: %s (in %s) -- nothing more is started" % (r.returncode, " (the time limit of %d s)" % limit if r.returncode in (124, 137) else "",
                                                                          " ".join(cmd), cwd))
    return r.stdout


def ensure_built(root):
    lib = os.path.join(root, "squad-mortar-helper_amd", "libsmh_vision_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(root, "squad-mortar-helper_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", os.path.join(root, "oracle"), "-s"])


def bench(root, args, what, limit=400):
    out = child([sys.executable, os.path.join(root, "bench.py")] + args, root, limit, what)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def traced_pass_us(root, what, limit=300):
    """Mean duration of the grey fused streaming kernel's launches of a depth-1 run, from the profiler's kernel statistics."""
    with tempfile.TemporaryDirectory() as d:
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.join(root, "bench.py"),
               "--pipeline-depth", "1", "--steps", "4", "--warmup", "1"], root, limit, what)
        hits = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not hits:
            sys.exit("no kernel statistics under %s" % d)
        with open(hits[0], newline="") as f:
            rows = [r for r in csv.DictReader(f) if "k_map_brq_pass" in r["Name"]]
    rows.sort(key=lambda r: -int(r["Calls"]))
    r = rows[0]
    return dict(kernel=r["Name"], calls=int(r["Calls"]), mean_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)


def pmc_bytes(root, what, limit=200):
    """WRITE_SIZE and 2 x FETCH_SIZE of the fused streaming kernel per 256 x 1080p launch: a profiler run per counter, nothing else
    collected but the kernels' names -> dict(kernel, write_MB, read_MB, n)."""
    got = {}
    for counter in ("WRITE_SIZE", "FETCH_SIZE"):
        with tempfile.TemporaryDirectory() as d:
            child(["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.join(root, "bench.py"),
                   "--traffic-child", "--config", "2"], root, limit, "%s %s" % (what, counter))
            vals, names = [], set()
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                with open(f, newline="") as fh:
                    for row in csv.DictReader(fh):
                        if row.get("Counter_Name") == counter and "k_map_brq_pass" in row.get("Kernel_Name", ""):
                            vals.append(float(row["Counter_Value"]))
                            names.add(row["Kernel_Name"])
            vals = [v for v in vals if v > 0.0]                        # (a dispatch occasionally comes back with a counter of exactly 0: a dropped sample)
            if not vals:
                sys.exit("rocprofv3 --pmc %s gave no sample of the streaming kernel (%s)" % (counter, root))
            got[counter] = dict(n=len(vals), mean_KB=sum(vals) / len(vals), kernels=sorted(names))
    return dict(kernel=got["WRITE_SIZE"]["kernels"], write_MB=got["WRITE_SIZE"]["mean_KB"] * 1024 / 1e6, read_MB=2.0 * got["FETCH_SIZE"]["mean_KB"] * 1024 / 1e6,
                n_write=got["WRITE_SIZE"]["n"], n_fetch=got["FETCH_SIZE"]["n"])


def _workload():
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=2)
    d = torch.from_numpy(frames).cuda().repeat(N // 16, 1, 1, 1)
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    return v, d, anchors


def leg_expand():
    """k_ui_expand alone (with the clearing of its flags behind it): a lazy grey run, then the expansion between two events, 10 times
    after 2 that are not counted."""
    import torch
    import squad_mortar_helper_amd as smh
    v, d, anchors = _workload()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    ms = []
    for rep in range(12):
        fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL, anchors=anchors, stream=s)
        torch.cuda.synchronize()
        assert fb.ui_state() == (N, False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fb.materialize_ui(s)
        e1.record()
        e1.synchronize()
        if rep >= 2:
            ms.append(e0.elapsed_time(e1))
    ly = fb.layout
    written = int(ly.ui_stride) * N
    print(json.dumps(dict(ms_per_launch=ms, bytes_written=written, bytes_read=written // 4, GBps=[(written + written // 4) / (m * 1e-3) / 1e9 for m in ms])))
    fb.close()
    v.shutdown()


def leg_pipeline(eager):
    """The headline's shape through a depth-12 frame-granular pipeline, 3 x 96 passes timed after 96: frames per second."""
    import torch
    import squad_mortar_helper_amd as smh
    v, d, anchors = _workload()
    pipe = smh.Pipeline(v, W, H, N, DEPTH, search="frame")
    if eager:
        for b in pipe.slots:
            assert b.device_ptrs()["ui"]
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
    print(json.dumps(dict(eager=bool(eager), frames_per_s=rates, ui_state=[list(b.ui_state()) for b in pipe.slots[:2]])))
    pipe.close()
    v.shutdown()


def own_leg(name, limit=300):
    out = child([sys.executable, os.path.abspath(__file__), "--leg", name], ROOT, limit, "this " + name)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def real_value(j):
    rs = j.get("real_samples") or {}
    return rs.get("value", rs.get("frames_per_s"))


def pmc_text(pmc):
    p, t = pmc["parent"], pmc["this"]
    return "\n".join([
        "The grey ui_map as a luma plane: HBM bytes of the fused streaming pass, this build against the parent commit.",
        "rocprofv3 --pmc WRITE_SIZE and --pmc FETCH_SIZE, a run per counter with nothing else collected but the kernels' names, over",
        "bench.py --traffic-child --config 2 (three plain passes over 256 x 1080p, grey).  Both builds in one job on one box; tools/ui_on_demand_cost.py.",
        "reads = 2 x FETCH_SIZE (the gfx950 correction for wide coalesced reads).",
        "",
        "per 256-frame launch (mean over the dispatches with a non-zero sample):",
        "  parent      %s" % "; ".join(p["kernel"])[:150],
        "  this build  %s" % "; ".join(t["kernel"])[:150],
        "  WRITE_SIZE  parent %7.1f MB   this build %7.1f MB   %+7.1f MB   (n = %d / %d)" % (p["write_MB"], t["write_MB"], t["write_MB"] - p["write_MB"], p["n_write"], t["n_write"]),
        "  FETCH_SIZE  parent %7.1f MB   this build %7.1f MB   %+7.1f MB   (x2 corrected; n = %d / %d)" % (p["read_MB"], t["read_MB"], t["read_MB"] - p["read_MB"], p["n_fetch"], t["n_fetch"]),
        "  total       parent %7.1f MB   this build %7.1f MB" % (p["write_MB"] + p["read_MB"], t["write_MB"] + t["read_MB"]),
        "expected from the layout: the ui_map's 986 x 822 px x 4 B in rows of 988 px are 0.83 GB per launch as RGBA and 0.21 GB as luma bytes: -0.62 GB.",
        "k_ui_expand does not appear: nothing in this run reads the RGBA slab."]) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit (built here if its library is missing)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc-out", default=None)
    ap.add_argument("--skip", default="", help="comma-separated: pmc, config4, cost")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.leg:
        return {"expand": leg_expand, "lazy": lambda: leg_pipeline(False), "eager": lambda: leg_pipeline(True)}[a.leg]()
    if not a.parent or not os.path.exists(os.path.join(a.parent, "bench.py")):
        ap.error("--parent: a checkout of the parent commit")
    skip = set(x for x in a.skip.split(",") if x)
    builds = (("parent", os.path.abspath(a.parent)), ("this", ROOT))
    for _, root in builds:
        ensure_built(root)
    state = dict(rounds=[], pmc=None, config4=None, cost=None)

    def save_partial():
        if a.out:                                             # (a job that is cut short keeps what it has)
            with open(a.out + ".partial", "w") as f:
                f.write(json.dumps(dict(state, spent_s=SPENT, wall_s=round(time.time() - T0, 1))) + "\n")
    for k in range(a.rounds):
        rec = {}
        for name, root in builds:
            tag = "round %d %s" % (k, name)
            head = bench(root, [], tag + " headline")
            full = bench(root, FULL, tag + " full")
            c3 = bench(root, ["--config", "3", "--steps", "10"], tag + " config 3")
            rec[name] = dict(headline_value=head["value"], traced_pass=traced_pass_us(root, tag + " trace"), full_launch_ms=full["roofline"]["launch_ms"],
                             full_launch_is=full["roofline"].get("launch_is"), full_value=full["value"], config3_value=c3["value"],
                             real_samples_value=real_value(full), real_samples=full.get("real_samples"))
            print("%s: headline %.0f, pass %.1f us traced / %.4f ms isolated, config 3 %.0f, real samples %s  [%d s so far]" % (
                tag, head["value"], rec[name]["traced_pass"]["mean_us"], rec[name]["full_launch_ms"], c3["value"], rec[name]["real_samples_value"], time.time() - T0), flush=True)
        state["rounds"].append(rec)
        save_partial()
        if k == 0 and "pmc" not in skip:
            state["pmc"] = {name: pmc_bytes(root, name + " pmc") for name, root in builds}
            print("pmc: %s" % json.dumps(state["pmc"]), flush=True)
            if a.pmc_out:
                with open(a.pmc_out, "w") as f:
                    f.write(pmc_text(state["pmc"]))
            save_partial()
    if "cost" not in skip:
        state["cost"] = dict(ui_expand_alone=own_leg("expand"), pipeline_lazy=own_leg("lazy"), pipeline_eager=own_leg("eager"))
        save_partial()
    if "config4" not in skip:
        state["config4"] = {name: bench(root, ["--config", "4", "--gpus", "1", "--steps", "10"], name + " config 4")["value"] for name, root in builds}
        save_partial()
    rounds = state["rounds"]

    def col(name, key, sub=None):
        return [(r[name][key][sub] if sub else r[name][key]) for r in rounds]

    def apart(this, parent, higher_is_better):
        this, parent = [x for x in this if x is not None], [x for x in parent if x is not None]
        if not this or not parent:
            return None
        return min(this) > max(parent) if higher_is_better else max(this) < min(parent)
    rsv = col("this", "real_samples_value") + col("parent", "real_samples_value")
    verdict = {
        "a_traced_pass_shorter_in_every_round": apart(col("this", "traced_pass", "mean_us"), col("parent", "traced_pass", "mean_us"), False),
        "a_isolated_launch_ms_shorter_in_every_round": apart(col("this", "full_launch_ms"), col("parent", "full_launch_ms"), False),
        "b_headline_above_in_every_round_ranges_apart": apart(col("this", "headline_value"), col("parent", "headline_value"), True),
        "c_config3_no_round_below_parents_lowest": min(col("this", "config3_value")) >= min(col("parent", "config3_value")),
        "d_real_samples_no_round_below_parents_lowest": None if None in rsv else min(col("this", "real_samples_value")) >= min(col("parent", "real_samples_value")),
    }
    import torch
    out = dict(what="the grey ui_map as a luma plane against the parent commit: one job, one box, %d interleaved rounds (parent, this), every figure a child process" % a.rounds,
               device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, rounds=rounds, verdict=verdict, pmc_per_launch=state["pmc"],
               config4_one_gpu=state["config4"], cost_to_a_host_that_asks=state["cost"],
               summary={k: dict(parent=col("parent", k), this=col("this", k)) for k in ("headline_value", "full_launch_ms", "config3_value", "real_samples_value", "full_value")},
               spent_s=SPENT, wall_s=round(time.time() - T0, 1))
    out["summary"]["traced_pass_mean_us"] = dict(parent=col("parent", "traced_pass", "mean_us"), this=col("this", "traced_pass", "mean_us"))
    print(json.dumps(dict(verdict=verdict, summary=out["summary"], pmc=state["pmc"], config4=state["config4"],
                          cost={k: {x: y for x, y in v.items() if x in ("ms_per_launch", "frames_per_s")} for k, v in (state["cost"] or {}).items()})))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        if os.path.exists(a.out + ".partial"):
            os.remove(a.out + ".partial")


if __name__ == "__main__":
    main()
