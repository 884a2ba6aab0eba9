"""What the 4:2:0 video layouts cost and buy: the conversion alone, and the ingest queue's rate per layout, in one job on one box.

  python tools/yuv_cost.py --rounds 3 --out profiles/yuv_cost.json [--parent <checkout of the parent commit, built>]

Every leg is a fresh child process under `timeout -k 10` with a limit of its own; a child that fails or runs out of time ends the
job and nothing is started after it.  Per round the legs run in turn, so the rounds interleave:
  conversion: smhv_yuv_to_bgra_device over 256 x 1080p resident frames -- NV12 and I420, nearest and bilinear, the whole frame and
      SMHV_YUV_ROI_ONLY -- each timed between two events beside a plain device copy that moves the same number of bytes (half of
      them read, half written), configuration after configuration inside every repetition.  Microseconds, and the algorithmic bytes
      (1.5 in + 4 out per converted pixel) as a share of the 8.0 TB/s HBM peak.
  queue: frames per second of the ingest queue alone (a native capture loop, every frame a new one, two slabs in turn) for BGRA
      plain, BGRA with SMHV_INGEST_ROI_UPLOAD, NV12 plain and NV12 with SMHV_INGEST_ROI_UPLOAD.  With --parent the two BGRA legs
      also run on the parent commit's build, in the same rounds: the ratio NV12 ROI upload / parent BGRA ROI upload is the
      figure the byte counts (about 1.2 MB against 3.3 MB per frame) promise something about.
Nothing depends on these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
HBM_PEAK = 8.0e12
T0 = time.time()
SPENT = []

QUEUE_LEG = r'''
import json, sys, time
sys.path.insert(0, %(root)r)
import numpy as np
import torch
import squad_mortar_helper_amd as smh
from squad_mortar_helper_amd import synth
W, H, layout, roi, total = %(w)d, %(h)d, %(layout)r, %(roi)r, %(total)d
v = smh.HipVision.init(0)
cap, slots = 64, 8
qs = [smh.IngestQueue(v, W, H, slots=slots, capacity=cap, roi_upload=roi) for _ in range(2)]
frame = synth.make_frame(W, H, 3, n_lines=2)[0]
kw = {} if layout == "bgra" else {"layout": layout}
for q in qs:                                                   # prime the staging buffers: their content persists
    for i in range(slots):
        buf = q.acquire()
        if layout == "bgra":
            buf[...] = frame
            q.commit()
        else:
            buf.reshape(-1)[:W * H * 3 // 2] = np.resize(frame[..., 1].reshape(-1), W * H * 3 // 2)
            q.commit(layout)
    q.batch(); q.reset()
counter, rates = 1, []
for rep in range(4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < total:
        q = qs[(done // cap) %% 2]
        q.reset()
        counter = q.feed(cap, counter, **kw)
        assert q.batch()[1] == cap
        done += cap
    torch.cuda.synchronize()
    if rep:
        rates.append(done / (time.perf_counter() - t0))
print(json.dumps(dict(layout=layout, roi_upload=roi, frames_per_s=rates)))
for q in qs:
    q.close()
v.shutdown()
'''


def child(cmd, limit, what, cwd=ROOT):
    env = dict(os.environ)
    env.pop("SMH_VISION_HIP_LIB", None)
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    SPENT.append((what, round(time.time() - t, 1)))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit("exit %d%s: %s -- nothing more is started" % (r.returncode, " (the time limit of %d s)" % limit if r.returncode in (124, 137) else "", what))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def queue_leg(root, layout, roi, total, what):
    """The BGRA legs use nothing the parent commit lacks but IngestQueue.feed's layout keyword, which they do not pass."""
    code = QUEUE_LEG % dict(root=root, w=W, h=H, layout=layout, roi=roi, total=total)
    return child([sys.executable, "-c", code], 240, what, cwd=root)


def leg_conversion():
    """All configurations inside every repetition: 12 repetitions, the first 2 not counted."""
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import yuv
    v = smh.HipVision.init(0)
    rx, ry, rw, rh = smh.map_bounds(W, H)
    bx, by, bw, bh = smh.button_bounds(W, H)
    px_full, px_roi = W * H, rw * rh + bw * bh
    src = torch.randint(0, 256, (N, W * H * 3 // 2), dtype=torch.uint8, device="cuda")
    out = torch.zeros((N, H, W, 4), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(int(N * px_full * 5.5) + 16, dtype=torch.uint8, device="cuda")      # the plain copies' source and destination
    st = torch.cuda.Stream()
    configs = [(lay, chroma, roi) for lay in ("nv12", "i420") for chroma in ("nearest", "bilinear") for roi in (False, True)]
    res = {"%s %s %s" % (lay, chroma, "roi_only" if roi else "full"): dict(us=[], copy_us=[]) for lay, chroma, roi in configs}
    with torch.cuda.stream(st):
        for rep in range(12):
            for lay, chroma, roi in configs:
                key = "%s %s %s" % (lay, chroma, "roi_only" if roi else "full")
                nbytes = int(N * (px_roi if roi else px_full) * 5.5)
                half = nbytes // 2
                a, b = scratch[:half], scratch[half:2 * half]
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                yuv.yuv_to_bgra(v, src.data_ptr(), N, W, H, yuv.pixels(lay, chroma=chroma), out_ptr=out.data_ptr(), roi_only=roi, stream=st.cuda_stream)
                e[1].record()
                e[2].record()
                b.copy_(a)
                e[3].record()
                e[3].synchronize()
                if rep >= 2:
                    res[key]["us"].append(e[0].elapsed_time(e[1]) * 1e3)
                    res[key]["copy_us"].append(e[2].elapsed_time(e[3]) * 1e3)
                res[key]["algorithmic_bytes"] = nbytes
    for r in res.values():
        med = sorted(r["us"])[len(r["us"]) // 2]
        cmed = sorted(r["copy_us"])[len(r["copy_us"]) // 2]
        r.update(median_us=med, copy_median_us=cmed, share_of_hbm_peak=r["algorithmic_bytes"] / (med * 1e-6) / HBM_PEAK,
                 copy_share_of_hbm_peak=r["algorithmic_bytes"] / (cmed * 1e-6) / HBM_PEAK, frames_per_s=N / (med * 1e-6))
    print(json.dumps(res))
    v.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its BGRA queue legs run in the same rounds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=2048, help="frames per timed repetition of a queue leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.leg == "conversion":
        return leg_conversion()
    rounds = []
    for k in range(a.rounds):
        rec = dict(conversion=child([sys.executable, os.path.abspath(__file__), "--leg", "conversion"], 240, "round %d conversion" % k))
        legs = [("this", ROOT, "bgra", False), ("this", ROOT, "bgra", True), ("this", ROOT, "nv12", False), ("this", ROOT, "nv12", True)]
        if a.parent:
            legs += [("parent", os.path.abspath(a.parent), "bgra", False), ("parent", os.path.abspath(a.parent), "bgra", True)]
        for name, root, lay, roi in legs:
            key = "%s %s %s" % (name, lay, "roi_upload" if roi else "plain")
            rec[key] = queue_leg(root, lay, roi, a.frames, "round %d %s" % (k, key))["frames_per_s"]
            print("round %d %s: %s  [%d s so far]" % (k, key, ["%.0f" % x for x in rec[key]], time.time() - T0), flush=True)
        rounds.append(rec)
        if a.out:
            with open(a.out + ".partial", "w") as f:
                f.write(json.dumps(dict(rounds=rounds, spent_s=SPENT)) + "\n")

    def med(key):
        xs = sorted(x for r in rounds for x in r[key])
        return xs[len(xs) // 2]
    keys = [k for k in rounds[0] if k != "conversion"]
    summary = {k: dict(median=med(k), lo=min(x for r in rounds for x in r[k]), hi=max(x for r in rounds for x in r[k])) for k in keys}
    base = "parent bgra roi_upload" if a.parent else "this bgra roi_upload"
    ratios = {"nv12 roi_upload / %s" % base: summary["this nv12 roi_upload"]["median"] / summary[base]["median"],
              "nv12 plain / %s bgra plain" % ("parent" if a.parent else "this"): summary["this nv12 plain"]["median"] / summary[base.replace("roi_upload", "plain")]["median"]}
    conv = {k: dict(median_us=[r["conversion"][k]["median_us"] for r in rounds], copy_median_us=[r["conversion"][k]["copy_median_us"] for r in rounds],
                    share_of_hbm_peak=[r["conversion"][k]["share_of_hbm_peak"] for r in rounds], copy_share_of_hbm_peak=[r["conversion"][k]["copy_share_of_hbm_peak"] for r in rounds],
                    algorithmic_bytes=rounds[0]["conversion"][k]["algorithmic_bytes"]) for k in rounds[0]["conversion"]}
    import torch
    out = dict(what="NV12 / I420 -> BGRA on the device and through the ingest queue: one job, one box, %d interleaved rounds, every leg a child process" % a.rounds,
               device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, frame="%d x %d" % (W, H), frames_per_conversion=N,
               bytes_per_frame_on_the_link=dict(bgra_plain=W * H * 4, nv12_plain=W * H * 3 // 2), conversion=conv, queue_frames_per_s=summary, ratios=ratios,
               parent_measured=bool(a.parent), rounds=rounds, spent_s=SPENT, wall_s=round(time.time() - T0, 1))
    print(json.dumps(dict(conversion={k: v["median_us"] for k, v in conv.items()}, queue=summary, ratios=ratios)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        if os.path.exists(a.out + ".partial"):
            os.remove(a.out + ".partial")


if __name__ == "__main__":
    main()
