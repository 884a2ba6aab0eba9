"""What reading the scale labels on the device costs: smhv_batch_label_text alone, and the whole way from the ocr plane to meters per
pixel -- scale_labels + label_text + run_label_anchors(STAGE_SCALES) -- over 256 resident 1080p frames and 128 resident 1440p
frames, beside a STAGE_ALL run and beside the way through the host: scale_labels, read_scale_labels with the crops, (somebody reads
the glyphs: not counted), then smhv_batch_run(STAGE_SCALES) with the anchors from the host.

  python tools/label_text_cost.py --out profiles/label_text_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  The frames are
the synthetic generator's (two scale bars each) with "<meters>m" painted over each bar, on a grey block, in the glyphs of csrc/smh_font5x7_ascii.h at
scale 2; the atlas is made of the same glyphs, so every label reads and the two ways must give the same meters per pixel (checked).
Inside a leg the measurements take turns in every round after WARMUP rounds that are not counted; device times lie between two
events on one stream, the two ways to meters per pixel are also taken as host wall time from the first call to the end of a
synchronising read of the records.  The figure is the median.  Nothing depends on these figures."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 2, 7
LEGS = {"256 x 1920x1080": (1920, 1080, 256), "128 x 2560x1440": (2560, 1440, 128)}
SCALE = 2


def _stat(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def _font():
    import numpy as np
    with open(os.path.join(ROOT, "squad-mortar-helper_amd", "csrc", "smh_font5x7_ascii.h")) as f:
        rows = re.findall(r"\{((?:0x[0-9A-Fa-f]{2},? ?){7})\}", f.read())
    out = {}
    for i, r in enumerate(rows[:95]):
        vals = [int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]{2}", r)]
        b = np.array([[(v >> (4 - x)) & 1 for x in range(5)] for v in vals], bool)
        if b.any():
            xs = np.flatnonzero(b.any(axis=0))
            out[chr(0x20 + i)] = np.kron(b[:, xs[0]:xs[-1] + 1], np.ones((SCALE, SCALE), bool))
    return out


def _templates(font, chars):
    import numpy as np
    from squad_mortar_helper_amd import _lib as L
    out = []
    for ch in chars:
        b = font[ch]
        ys = np.flatnonzero(b.any(axis=1))
        b = b[ys[0]:ys[-1] + 1]
        t = L.GlyphTemplate()
        t.code, t.w, t.h = ord(ch), b.shape[1], b.shape[0]
        for y in range(b.shape[0]):
            t.rows[y] = sum(1 << int(x) for x in np.flatnonzero(b[y]))
        out.append(t)
    return out


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    from squad_mortar_helper_amd import synth
    W, H, N = LEGS[name]
    v = smh.HipVision.init(0)
    font = _font()
    frames16, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=4)
    rx, ry, rw, rh = infos[0]["roi"]
    for f, info in zip(frames16, infos):                          # "<meters>m" over each bar: its last row just above the anchor's row
        for (m, ax, ay) in info["anchors"]:
            pieces = [font[c] for c in "%dm" % m]
            wd = sum(p.shape[1] for p in pieces) + len(pieces) - 1
            x = rx + rw // 2 + ax - wd // 2
            y = ry + rh // 2 + ay
            f[y - 7 * SCALE - 3:y + 2, x - 6:x + wd + 6, :3] = 128   # (a marker line across the label would join its glyphs: grey is background)
            for p in pieces:
                ys, xs = np.nonzero(p)
                f[ry + rh // 2 + ay - 7 * SCALE + ys, x + xs, :3] = 255
                x += p.shape[1] + 1
    few = torch.from_numpy(frames16).cuda()
    frames = few[torch.arange(N, device="cuda") % 16].contiguous()
    del few
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    atlas = smh.GlyphAtlas.from_templates(v, _templates(font, "0123456789m"))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    torch.cuda.synchronize()
    keys = ("run_all_us", "label_text_us", "device_chain_us", "device_chain_wall_us", "host_chain_wall_us", "host_chain_device_us", "read_labels_wall_us")
    t = {k: [] for k in keys}
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
            e[0].record()
            fb.run(frames.data_ptr(), N, stages=smh.STAGE_ALL, anchors=anchors, stream=s)
            e[1].record()
            e[1].synchronize()
            # the device's way: labels, texts, the scales stage with the anchors where they are
            w0 = time.perf_counter()
            e[2].record()
            fb.scale_labels(frames.data_ptr(), N, stream=s)
            e[3].record()
            fb.label_text(atlas, N, stream=s)
            e[4].record()
            fb.run_label_anchors(frames.data_ptr(), N, stages=smh.STAGE_SCALES, stream=s)
            e[5].record()
            dev = [(r.has_mpx, r.mpx) for r in fb.read_results(0, N)]
            w1 = time.perf_counter()
            texts = fb.read_label_text(0, N)
            # the host's way: labels and crops down, (the glyphs are read: not counted), anchors up, the scales stage
            fb.run(frames.data_ptr(), N, stages=smh.STAGE_OCR, stream=s)
            torch.cuda.synchronize()
            w2 = time.perf_counter()
            e[6].record()
            fb.scale_labels(frames.data_ptr(), N, stream=s)
            e[7].record()
            recs, cells = fb.read_scale_labels(0, N)
            w3 = time.perf_counter()
            per_frame = []
            for i in range(N):
                an = texts[i].anchors                             # (what a reader would have typed: the device's own reading)
                per_frame.append((an.scales_start_y, [tuple(an.scales[k]) for k in range(an.n)]))
            host_anchors = smh.make_anchors(per_frame)
            w4 = time.perf_counter()
            e[8].record()
            fb.run(frames.data_ptr(), N, stages=smh.STAGE_SCALES, anchors=host_anchors, stream=s)
            e[9].record()
            host = [(r.has_mpx, r.mpx) for r in fb.read_results(0, N)]
            w5 = time.perf_counter()
            assert dev == host and all(h for h, _ in dev), "the two ways disagree, or a frame has no meters per pixel"
            if rep >= WARMUP:
                t["run_all_us"].append(e[0].elapsed_time(e[1]) * 1e3)
                t["label_text_us"].append(e[3].elapsed_time(e[4]) * 1e3)
                t["device_chain_us"].append(e[2].elapsed_time(e[5]) * 1e3)
                t["device_chain_wall_us"].append((w1 - w0) * 1e6)
                t["host_chain_device_us"].append((e[6].elapsed_time(e[7]) + e[8].elapsed_time(e[9])) * 1e3)
                t["host_chain_wall_us"].append((w3 - w2 + w5 - w4) * 1e6)
                t["read_labels_wall_us"].append((w3 - w2) * 1e6)
    out = dict(leg=name, device=torch.cuda.get_device_name(0), frames=N, quadrant=[rw // 2, rh // 2], labels_per_frame=sorted({int(r.n) for r in texts}),
               glyphs_per_label=sorted({int(r.label[k].n_glyphs) for r in texts for k in range(r.n)}), templates=len(atlas.templates),
               bytes_per_frame=dict(host_way_down=L.C.sizeof(L.ScaleLabelFrame) + L.MAX_SCALE_LABELS * L.LABEL_CROP_W * L.LABEL_CROP_H,
                                    host_way_up=L.C.sizeof(L.Anchors), device_way=0),
               **{k: _stat(x) for k, x in t.items()})
    out["per_frame_us"] = {k: out[k]["median"] / N for k in t}
    print(json.dumps(out))
    fb.close()
    atlas.close()
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
    out = dict(what="smhv_batch_label_text alone (k_label_text, one workgroup per frame), and the way from the ocr plane to meters per pixel on the device "
                    "(scale_labels + label_text + run_label_anchors(STAGE_SCALES): device_chain) beside a STAGE_ALL run and beside the way through the host "
                    "(scale_labels, read_scale_labels with crops, anchors from the host into smhv_batch_run(STAGE_SCALES): host_chain; the time somebody "
                    "takes to read the glyphs is not counted); wall figures run from the first call to the end of the synchronising read of the records; "
                    "median of %d timed rounds after %d warm-up rounds, the measurements in turn; one child process per leg" % (REPS, WARMUP),
               legs=legs, wall_s=round(time.time() - t0, 1))
    print(json.dumps({k: dict(per_frame_us={m: round(x, 3) for m, x in leg_["per_frame_us"].items()}) for k, leg_ in legs.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
