"""What keeping the search service's candidate window between candidates buys, against the PARENT commit's build on the same box in one job
(the protocol of tools/ui_on_demand_cost.py).

  python tools/window_reuse_cost.py --parent <checkout of the parent commit> --rounds 3 --out profiles/window_reuse_cost.json \\
      [--variant e8=<library built with -DSVC_WIN_EXTRA=8u> ...] [--wprof parent=<lib> --wprof this=<lib>]

Builds: "parent" (the checkout's library), "this" (this tree's library) and any --variant NAME=LIB (this tree's Python over another
library: the window heights tried, -DSVC_WIN_EXTRA=8u / 16u / 24u, and -DSMH_NO_WINDOW_REUSE).  Per round the parent first and the others
after it (so the rounds interleave), every figure a fresh child process under `timeout -k 10` with a limit of its own; a child that
fails or runs out of time ends the job, nothing is started after it.
  (1) once, where --wprof names `make wprof` libraries: tools/svc_rate.py over 256 x 1080p at depth 12, as the pipeline runs it and
      with no help (RATE_FLAGS=9: the owner casts every candidate, which is what tools/window_reuse_count.py predicts fills for):
      s_window_fill, setup, search and help cycles per frame, window fills per frame, and the split inside the units (first batches,
      long rays, end points)
  (2) the headline: `value` of the default bench.py run (config 2)
  (3) `bench.py --config 3`, the real-samples leg of a --full run; once: `bench.py --config 4` on one GPU
The verdict: (2) every round of a build above every round of the parent; (3) a loss is every round below every round of the parent.
Nothing depends on these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = ["--full", "--cpu-sample", "0", "--ingest-frames", "0", "--side-probe", "0", "--no-traffic-probe", "--no-depth1", "--no-back-to-back", "--steps", "10"]
T0 = time.time()
SPENT = []


def child(cmd, cwd, lib, limit, what, env_extra=None):
    env = dict(os.environ)
    env.pop("SMH_VISION_HIP_LIB", None)
    if lib:
        env["SMH_VISION_HIP_LIB"] = lib
    env.update(env_extra or {})
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    SPENT.append((what, round(time.time() - t, 1)))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit("exit %d%s: %s (in %s) -- nothing more is started" % (r.returncode, " (the time limit of %d s)" % limit if r.returncode in (124, 137) else "", " ".join(cmd), cwd))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def real_value(j):
    rs = j.get("real_samples") or {}
    return rs.get("value", rs.get("frames_per_s"))


def pairs(items):
    out = []
    for it in items or []:
        name, _, path = it.partition("=")
        if not path or not os.path.exists(path):
            sys.exit("--variant / --wprof NAME=LIB: %r" % it)
        out.append((name, os.path.abspath(path)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit, built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", action="append", help="NAME=LIB: this tree over another build of the library")
    ap.add_argument("--wprof", action="append", help="NAME=LIB: a `make wprof` library of build NAME (parent, this or a variant)")
    ap.add_argument("--skip", default="", help="comma-separated: config4, full, config3")
    ap.add_argument("--what", default="the search service's candidate window kept between candidates", help="the change under test, for the record's first line (other changes use this protocol: tools/cull_chain_count.py names one)")
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(",") if x)
    parent = os.path.abspath(a.parent)
    lib_of = lambda root: os.path.join(root, "squad-mortar-helper_amd", "libsmh_vision_hip.so")
    builds = [("parent", parent, lib_of(parent)), ("this", ROOT, lib_of(ROOT))] + [(n, ROOT, p) for n, p in pairs(a.variant)]
    for n, root, lib in builds:
        if not os.path.exists(lib):
            sys.exit("%s: %s is not built" % (n, lib))
    state = dict(wprof={}, rounds=[], config4=None)

    def save_partial():
        if a.out:
            with open(a.out + ".partial", "w") as f:
                f.write(json.dumps(dict(state, spent_s=SPENT, wall_s=round(time.time() - T0, 1))) + "\n")
    for n, lib in pairs(a.wprof):
        root = parent if n == "parent" else ROOT
        rec = {}
        for leg, flags in (("pipeline", "0"), ("no_help", "9")):
            j = child([sys.executable, os.path.join(root, "tools", "svc_rate.py"), "256", "12", "120"], root, lib, 300, "%s wprof %s" % (n, leg),
                      dict(SVC_RATE_WPROF="1", RATE_SEARCH="frame", RATE_FLAGS=flags))
            p, st = j["scan_profile_cycles_per_frame"], j["search_service"]
            rec[leg] = dict(s_window_fill=p["s_window_fill"], s_cull_scan=p["s_cull_scan"], setup=p["setup"], units=p["units"], verdict=p["verdict"], rounds=p["rounds"],
                            window_fills=p.get("window_fills"), cast_by_owner=p.get("cast_by_owner"), n_units=p.get("n_units"), cycles_per_unit=p.get("cycles_per_unit"),
                            u_first_batches=p.get("u_first_batches"), u_long_rays=p.get("u_long_rays"), u_end_points=p.get("u_end_points"), search=st["cycles_per_frame_by_phase"]["search"],
                            help_cycles_per_frame=st["help_cycles_per_frame"], frames_per_s=j["frames_per_s"], equal=j["slots_equal_plain_run"])
            print("wprof %s %s: %s" % (n, leg, json.dumps(rec[leg])), flush=True)
        state["wprof"][n] = rec
        save_partial()
    for k in range(a.rounds):
        rec = {}
        for n, root, lib in builds:
            tag = "round %d %s" % (k, n)
            r = dict(headline_value=child([sys.executable, os.path.join(root, "bench.py")], root, lib, 400, tag + " headline")["value"])
            if "config3" not in skip:
                r["config3_value"] = child([sys.executable, os.path.join(root, "bench.py"), "--config", "3", "--steps", "10"], root, lib, 400, tag + " config 3")["value"]
            if "full" not in skip:
                full = child([sys.executable, os.path.join(root, "bench.py")] + FULL, root, lib, 400, tag + " full")
                r["real_samples_value"], r["full_value"] = real_value(full), full["value"]
            rec[n] = r
            print("%s: %s  [%d s so far]" % (tag, json.dumps(r), time.time() - T0), flush=True)
        state["rounds"].append(rec)
        save_partial()
    if "config4" not in skip:
        state["config4"] = {n: child([sys.executable, os.path.join(root, "bench.py"), "--config", "4", "--gpus", "1", "--steps", "10"], root, lib, 400, n + " config 4")["value"]
                            for n, root, lib in builds}
        save_partial()
    names = [n for n, _, _ in builds]
    keys = [k for k in ("headline_value", "config3_value", "real_samples_value", "full_value") if k in state["rounds"][0]["parent"]]
    summary = {k: {n: [r[n][k] for r in state["rounds"]] for n in names} for k in keys}
    verdict = {}
    for n in names[1:]:
        v = {}
        for k in keys:
            mine, par = [x for x in summary[k][n] if x is not None], [x for x in summary[k]["parent"] if x is not None]
            if mine and par:
                v[k] = "above in every round" if min(mine) > max(par) else ("below in every round" if max(mine) < min(par) else "ranges overlap")
        verdict[n] = v
    import torch
    out = dict(what="%s, against the parent commit: one job, one box, %d interleaved rounds, every figure a child process" % (a.what, a.rounds),
               device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, builds={n: os.path.relpath(lib, ROOT) for n, _, lib in builds},
               wprof_cycles_per_frame=state["wprof"], rounds=state["rounds"], summary=summary, verdict=verdict, config4_one_gpu=state["config4"], spent_s=SPENT, wall_s=round(time.time() - T0, 1))
    print(json.dumps(dict(verdict=verdict, summary=summary, config4=state["config4"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        if os.path.exists(a.out + ".partial"):
            os.remove(a.out + ".partial")


if __name__ == "__main__":
    main()
