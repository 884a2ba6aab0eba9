"""Cost of the map view's layers (k_render_map_layers, smhv_batch_render_layers), measured on one GPU, one box, profiler off.

  python tools/render_layers_cost.py --out profiles/render_layers_cost.json

256 x 1080p synthetic frames (16 distinct ones, repeated), windows 1280 x 720 and 2560 x 1440, a random 1024^2 heightmap.  Every
launch is timed with a pair of events on the stream; the configurations are run one after the other and the whole round is repeated
`--reps` times (after one round that is not counted), so the launches that are compared alternate; the figure is the median.
  1. the layers' kernel with nothing to draw against the kernel without layers of the same form, in the same run: without a
     heightmap (the four-wave gathers) and with one in each form of the tap fetch
  2. 32 and 256 prims (short lines and small rectangle outlines, half of them on the foreground, spread over the window)
  3. each gray source (the ocr, scales and mask planes) against the ui_map as the map quad's texture
Nothing depends on these figures: smhv_batch_render / smhv_render_map keep the kernels without layers whatever they show."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N = 1920, 1080, 256
WINDOWS = ((1280, 720), (2560, 1440))


def make_prims(smh, vp, ow, oh, n, rng):
    import numpy as np
    out = []
    for i in range(n):
        x, y = rng.uniform(0.0, ow), rng.uniform(0.0, oh)
        if i % 2:
            a, ln = rng.uniform(0.0, 2 * np.pi), rng.uniform(10.0, 120.0)
            w = (x, y, x + ln * np.cos(a), y + ln * np.sin(a))
            kind = smh.PRIM_LINE
        else:
            w = (x, y, x + rng.uniform(8.0, 150.0), y + rng.uniform(8.0, 60.0))
            kind = smh.PRIM_RECT
        p0, p1 = vp.inverse_xy(w[:2]), vp.inverse_xy(w[2:])
        out.append(smh.prim(p0[0], p0[1], p1[0], p1[1], (255, 0, 255, 255), kind | (smh.PRIM_FOREGROUND if i % 4 < 2 else 0)))
    return out


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
    L = smh._lib
    v = smh.HipVision.init(0)
    rng = np.random.default_rng(0)
    frames, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=2)
    d = torch.from_numpy(np.tile(frames, (N // 16, 1, 1, 1))).cuda()
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    hm = smh.Heightmap(v, rng.integers(0, 65536, size=(1024, 1024), dtype=np.uint16), ((0, 0), (0, 0)), (1.0, 1.0, 50.0))
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors, stream=s)
    _, _, rw, rh = fb.roi
    configs = []                                                  # (label, window, viewport, heightmap, form, layers or None)
    for ow, oh in WINDOWS:
        vp = smh.MapViewport.calc(ow, oh, rw, rh)
        win = "%dx%d" % (ow, oh)
        empty = smh.RenderLayers()
        for name, h, form in (("none", None, 0), ("form1", hm, 1), ("form2", hm, 2), ("form3", hm, 3)):
            configs.append(("%s/%s/without layers" % (win, name), (ow, oh), vp, h, form, None))
            configs.append(("%s/%s/layers, nothing to draw" % (win, name), (ow, oh), vp, h, form, empty))
        for n in (32, 256):
            prims = smh.RenderLayers(make_prims(smh, vp, ow, oh, n, rng))
            configs.append(("%s/none/%d prims" % (win, n), (ow, oh), vp, None, 0, prims))
            configs.append(("%s/form3/%d prims" % (win, n), (ow, oh), vp, hm, 3, prims))
        configs.append(("%s/none/minimap bounds" % win, (ow, oh), vp, None, 0, smh.RenderLayers(minimap_bounds=True)))
        for name, src in (("ocr", L.VIEW_OCR_INPUT), ("scales", L.VIEW_FIND_SCALES_INPUT), ("mask", L.VIEW_LSD_INPUT),
                          ("isolated", L.VIEW_LSD_PREPROCESS), ("bottom right quarter", L.VIEW_CROPPED_BRQ)):
            configs.append(("%s/none/source %s" % (win, name), (ow, oh), vp, None, 0, smh.RenderLayers(map_source=src)))
    times = {c[0]: [] for c in configs}
    for rep in range(a.reps + 1):
        for label, (ow, oh), vp, h, form, layers in configs:
            L.check(L.load().smhv_debug_render_form(form))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fb.render(vp, ow, oh, heightmap=h, stream=s, layers=layers)
            e1.record()
            e1.synchronize()
            if rep:
                times[label].append(e0.elapsed_time(e1))
    L.check(L.load().smhv_debug_render_form(0))
    out = dict(what="k_render_map_layers against k_render_map of the same form and against itself; ms per launch of %d frames between two events, profiler off, "
                    "configurations alternated, median of %d" % (N, a.reps),
               frames_per_launch=N, frame=[W, H], map=[rw, rh], device=torch.cuda.get_device_name(0),
               ms={k: dict(median=median(t), min=min(t), max=max(t), all=t) for k, t in times.items()})
    ratio = {}
    for ow, oh in WINDOWS:
        win = "%dx%d" % (ow, oh)
        for name in ("none", "form1", "form2", "form3"):
            ratio["%s/%s: layers with nothing to draw / without layers" % (win, name)] = \
                out["ms"]["%s/%s/layers, nothing to draw" % (win, name)]["median"] / out["ms"]["%s/%s/without layers" % (win, name)]["median"]
        base = out["ms"]["%s/none/layers, nothing to draw" % win]["median"]
        for k in ("32 prims", "256 prims", "minimap bounds", "source ocr", "source scales", "source mask", "source isolated", "source bottom right quarter"):
            ratio["%s/none: %s / nothing to draw" % (win, k)] = out["ms"]["%s/none/%s" % (win, k)]["median"] / base
        base = out["ms"]["%s/form3/layers, nothing to draw" % win]["median"]
        for k in ("32 prims", "256 prims"):
            ratio["%s/form3: %s / nothing to draw" % (win, k)] = out["ms"]["%s/form3/%s" % (win, k)]["median"] / base
    out["ratio"] = ratio
    print(json.dumps(dict(ratio=ratio)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    fb.close()
    hm.close()
    v.shutdown()


if __name__ == "__main__":
    main()
