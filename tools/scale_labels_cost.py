"""What the scale labels cost: smhv_batch_scale_labels over 256 resident 1080p frames and 128 resident 1440p frames, beside what a
host OCR needs today -- smhv_batch_read_image of the ocr plane of every frame -- and beside the batch run itself.

  python tools/scale_labels_cost.py --out profiles/scale_labels_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  The frames are
the synthetic generator's (two scale bars each) with a white block over each bar for a label, so every frame has two proposals.
Inside a leg the four measurements take turns in every round after WARMUP rounds that are not counted: the run (STAGE_ALL with the
frames' anchors) and the labels' launch (the quadrant pass that makes S0, then k_scale_labels) each between two events on one stream;
the read of the label and crop slabs and the read of the ocr planes as host wall time (both synchronise).  The figure is the median.
Bytes per frame: what each way moves to the host.  Nothing depends on these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 2, 7
LEGS = {"256 x 1920x1080": (1920, 1080, 256), "128 x 2560x1440": (2560, 1440, 128)}


def _stat(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    from squad_mortar_helper_amd import synth
    W, H, N = LEGS[name]
    v = smh.HipVision.init(0)
    frames16, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=4)
    rx, ry, rw, rh = infos[0]["roi"]
    for f, info in zip(frames16, infos):                          # a label over each bar: a white block whose bottom is the anchor's row
        for (_, ax, ay) in info["anchors"]:
            f[ry + rh // 2 + ay - 10:ry + rh // 2 + ay, rx + rw // 2 + ax - 16:rx + rw // 2 + ax + 16, :3] = 255
    few = torch.from_numpy(frames16).cuda()
    frames = few[torch.arange(N, device="cuda") % 16].contiguous()
    del few
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    torch.cuda.synchronize()
    t = {"run_us": [], "scale_labels_us": [], "read_labels_wall_us": [], "read_ocr_planes_wall_us": []}
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            fb.run(frames.data_ptr(), N, stages=smh.STAGE_ALL, anchors=anchors, stream=s)
            e[1].record()
            e[1].synchronize()
            e[2].record()
            fb.scale_labels(frames.data_ptr(), N, stream=s)
            e[3].record()
            e[3].synchronize()
            t0 = time.perf_counter()
            recs, cells = fb.read_scale_labels(0, N)
            t1 = time.perf_counter()
            for f in range(N):
                fb.read_image(L.VIEW_OCR_INPUT, f)
            t2 = time.perf_counter()
            if rep >= WARMUP:
                t["run_us"].append(e[0].elapsed_time(e[1]) * 1e3)
                t["scale_labels_us"].append(e[2].elapsed_time(e[3]) * 1e3)
                t["read_labels_wall_us"].append((t1 - t0) * 1e6)
                t["read_ocr_planes_wall_us"].append((t2 - t1) * 1e6)
    qw, qh = rw // 2, rh // 2
    out = dict(leg=name, device=torch.cuda.get_device_name(0), frames=N, quadrant=[qw, qh],
               proposals_per_frame=sorted({int(r.n_found) for r in recs}), runs_per_frame=_stat([int(r.n_runs) for r in recs]),
               bytes_per_frame=dict(labels_and_crops=L.C.sizeof(L.ScaleLabelFrame) + L.MAX_SCALE_LABELS * L.LABEL_CROP_W * L.LABEL_CROP_H, ocr_plane=qw * qh),
               **{k: _stat(x) for k, x in t.items()})
    out["per_frame_us"] = {k: out[k]["median"] / N for k in t}
    print(json.dumps(out))
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
    out = dict(what="smhv_batch_scale_labels (the quadrant pass for S0, then k_scale_labels, one workgroup per frame) over every frame of a resident batch, "
                    "beside the batch run (STAGE_ALL) and beside reading every frame's ocr plane to the host (smhv_batch_read_image), which a host OCR "
                    "needs today; median of %d timed rounds after %d warm-up rounds, the measurements in turn; one child process per leg" % (REPS, WARMUP),
               legs=legs, wall_s=round(time.time() - t0, 1))
    print(json.dumps({k: dict(per_frame_us={m: round(x, 2) for m, x in leg_["per_frame_us"].items()}, bytes_per_frame=leg_["bytes_per_frame"]) for k, leg_ in legs.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
