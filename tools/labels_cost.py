"""Cost of the marker labels (k_label_plan + k_label_draw, smhv_batch_render_labels), measured on one GPU, one box, profiler off.

  python tools/labels_cost.py --out profiles/labels_cost.json

256 x 1080p synthetic frames (16 distinct ones, repeated) with 32 marker lines each, windows 1280 x 720 and 2560 x 1440, S = 2.
The yardstick is the render launch of the same run: smhv_batch_render with the marker lines (the kernel without layers, no
heightmap), which the labels are drawn over.  Every launch is timed with a pair of events on the stream; render and labels
alternate and the whole round is repeated `--reps` times after one round that is not counted; the figure is the median.  The
label call is timed whole: the wait on the render's event, k_label_plan and k_label_draw.  Nothing depends on these figures."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, LINES = 1920, 1080, 256, 32
WINDOWS = ((1280, 720), (2560, 1440))


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    v = smh.HipVision.init(0)
    frames, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=LINES)
    d = torch.from_numpy(np.tile(frames, (N // 16, 1, 1, 1))).cuda()
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors, stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    _, _, rw, rh = fb.roi
    lines_found = [r["n_lines"] for r in recs]
    with_mpx = sum(r["mpx"] is not None for r in recs)
    labels = smh.LabelOptions(detected=True, scale=2)
    times, n_labelled = {}, {}
    for ow, oh in WINDOWS:
        win = "%dx%d" % (ow, oh)
        vp = smh.MapViewport.calc(ow, oh, rw, rh)
        opt = smh.render_options(vp, ow, oh, markers=True)
        times[win + "/render with markers"], times[win + "/labels"] = [], []
        for rep in range(a.reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            fb.render(vp, ow, oh, options=opt, stream=s)
            ev[1].record()
            ev[2].record()
            fb.render_labels(opt, labels, stream=s)
            ev[3].record()
            ev[3].synchronize()
            if rep:
                times[win + "/render with markers"].append(ev[0].elapsed_time(ev[1]))
                times[win + "/labels"].append(ev[2].elapsed_time(ev[3]))
        res = fb.read_labels(0, N)
        n_labelled[win] = sum(1 for f in range(N) for i in range(res[f].n_labels) if res[f].label[i].n_runs)
    out = dict(what="smhv_batch_render_labels (k_label_plan + k_label_draw) against smhv_batch_render with markers of the same run; ms per launch of %d "
                    "frames between two events, profiler off, the two alternated, median of %d" % (N, a.reps),
               frames_per_launch=N, frame=[W, H], map=[rw, rh], lines_asked=LINES, lines_found=dict(min=min(lines_found), max=max(lines_found), total=sum(lines_found)),
               frames_with_mpx=with_mpx, labels_drawn=n_labelled, device=torch.cuda.get_device_name(0),
               ms={k: dict(median=median(t), min=min(t), max=max(t), all=t) for k, t in times.items()})
    out["ratio"] = {"%dx%d: labels / render with markers" % w: out["ms"]["%dx%d/labels" % w]["median"] / out["ms"]["%dx%d/render with markers" % w]["median"]
                    for w in WINDOWS}
    print(json.dumps(dict(ratio=out["ratio"], ms={k: m["median"] for k, m in out["ms"].items()}, labels_drawn=n_labelled)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    fb.close()
    v.shutdown()


if __name__ == "__main__":
    main()
