"""Cost of the vision debugger and the debug text (k_probe, k_debug_plan + k_debug_draw: smhv_batch_probe,
smhv_batch_render_debug), measured on one GPU, one box, profiler off.

  python tools/debug_text_cost.py --out profiles/debug_text_cost.json

256 x 1080p synthetic frames (16 distinct ones, repeated) with 32 marker lines each, a window of 1920 x 1080, S = 2.  Three
figures: the probe alone (16 points), the pass with 16 text runs (the Debug menu's overlays: 8 OCR captions of two lines and 8
scale captions), and the pass with 16 probe windows.  The yardstick is the labels pass of the same process on the same images,
smhv_batch_render_labels with the detected lines: its nearest relative -- both rewrite only the tiles that hold something.
Every call is timed whole with a pair of events on the stream; the four alternate and the whole round is repeated `--reps`
times after one round that is not counted; the figure is the median.  Nothing depends on these figures."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, LINES = 1920, 1080, 256, 32
WINDOW = (1920, 1080)


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
    fb.read_results(0, N)
    _, _, rw, rh = fb.roi
    ow, oh = WINDOW
    vp = smh.MapViewport.calc(ow, oh, rw, rh)
    opt = smh.render_options(vp, ow, oh, markers=True)
    labels = smh.LabelOptions(detected=True, scale=2)
    # the Debug menu's overlays as the app would have them: OCR captions under boxes in the bottom right quadrant, scale captions
    boxes = [(20 + 90 * (i % 4), 30 + 120 * (i // 4), 90 + 90 * (i % 4), 50 + 120 * (i // 4), 91.25 - 7 * i, "%d00m" % (i + 1)) for i in range(8)]
    bars = [(100 * (i + 1), 10 + 40 * i, 200 + 25 * i, 60 + 40 * i, True) for i in range(8)]
    runs = smh.ocr_text_runs(boxes, rw // 2, rh // 2) + smh.scale_text_runs(bars, rw // 2, rh // 2)
    assert len(runs) == 16
    points = [vp.translate_xy((rw * (0.1 + 0.2 * (i % 4)), rh * (0.1 + 0.2 * (i // 4)))) for i in range(16)]
    passes = {
        "labels": lambda: fb.render_labels(opt, labels, stream=s),
        "probe alone": lambda: fb.probe(opt, points, stream=s),
        "debug pass, 16 runs": lambda: fb.render_debug(opt, smh.DebugOptions(runs, scale=2), stream=s),
        "debug pass, 16 probe windows": lambda: fb.render_debug(opt, smh.DebugOptions(probes=points, draw_probes=True, scale=2), stream=s),
    }
    times = {k: [] for k in passes}
    for rep in range(a.reps + 1):
        fb.render(vp, ow, oh, options=opt, stream=s)
        for name, call in passes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    probes = fb.read_probes(0, N)
    out = dict(what="smhv_batch_probe and smhv_batch_render_debug against smhv_batch_render_labels of the same process on the same images; ms per call of %d "
                    "frames between two events, profiler off, the four alternated, median of %d" % (N, a.reps),
               frames_per_launch=N, frame=[W, H], map=[rw, rh], window=list(WINDOW), scale=2, runs=len(runs), probes=len(points),
               valid_probes=sum(1 for p in probes if p.valid), device=torch.cuda.get_device_name(0),
               ms={k: dict(median=median(t), min=min(t), max=max(t), all=t) for k, t in times.items()})
    out["ratio"] = {"%s / labels" % k: out["ms"][k]["median"] / out["ms"]["labels"]["median"] for k in passes if k != "labels"}
    print(json.dumps(dict(ratio=out["ratio"], ms={k: m["median"] for k, m in out["ms"].items()}, valid_probes=out["valid_probes"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    fb.close()
    v.shutdown()


if __name__ == "__main__":
    main()
