"""What video frames out cost: smhv_batch_video over 256 frames of a 1920 x 1080 window (the render slab) and of the 1080p ui_map,
colour (the RGBA slab) and grey (the luma plane), NV12 and I420, beside a plain device copy.

  python tools/video_out_cost.py --out profiles/video_out_cost.json

The measurement runs in one child process under `timeout -k 10`; a child that fails or runs out of time ends the job.  Every
configuration is warmed up, then timed REPS times between two events on one stream, the configurations in turn inside every
repetition, each beside a hipMemcpyAsync device-to-device copy that moves the same number of bytes (half of them read, half
written).  Reported: the median milliseconds per call, the algorithmic bytes (4 or 1 in + 1.5 out per pixel) per second, the copy's
the same way, and the ratio of the grey path's time to the RGBA path's.  Nothing depends on these figures."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
WARMUP, REPS = 3, 24
HBM_PEAK = 8.0e12


def leg():
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth, yuv
    v = smh.HipVision.init(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    few = torch.from_numpy(np.stack([synth.make_frame(W, H, i, n_lines=2)[0] for i in range(4)])).cuda()
    frames = few[torch.arange(N, device="cuda") % 4].contiguous()
    del few
    torch.cuda.synchronize()                                        # (the timed stream does not wait for torch's own)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    batches = {}
    for name, gray in (("colour", False), ("grey", True)):
        fb = smh.FrameBatch(v, W, H, N)
        torch.cuda.synchronize()                                    # (the batch's slabs are cleared on the null stream, which `st` does not wait for)
        fb.run(frames.data_ptr(), N, stages=0x3, grayscale=gray, stream=s)
        st.synchronize()
        n_open = sum(r["map_open"] for r in smh.results_to_dicts(fb.read_results(0, N)))
        assert n_open == N, "%d of %d maps open" % (n_open, N)
        assert fb.ui_state() == ((N, False) if gray else (0, False))
        batches[name] = fb
    rw, rh = batches["colour"].roi[2:]
    batches["colour"].render(smh.MapViewport.calc(W, H, rw, rh), W, H, markers=True, stream=s)
    st.synchronize()
    # (source, the batch, w, h, bytes read per pixel)
    sources = [("window 1920x1080", "render", batches["colour"], W, H, 4.0), ("ui_map %dx%d colour" % (rw, rh), "ui_map", batches["colour"], rw, rh, 4.0),
               ("ui_map %dx%d grey" % (rw, rh), "ui_map", batches["grey"], rw, rh, 1.0)]
    configs = [(name, src, fb, w, h, bpp, lay) for name, src, fb, w, h, bpp in sources for lay in ("nv12", "i420")]
    out = torch.zeros(N * yuv.video_bytes(W, H, yuv.pixels("nv12")), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(int(N * W * H * 5.5) + 64, dtype=torch.uint8, device="cuda")
    res = {"%s %s" % (name, lay): dict(ms=[], copy_ms=[]) for name, _, _, _, _, _, lay in configs}
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            for name, src, fb, w, h, bpp, lay in configs:
                key = "%s %s" % (name, lay)
                nbytes = int(N * w * h * bpp) + N * yuv.video_bytes(w, h, yuv.pixels(lay))
                half = nbytes // 2
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                fb.video(src, yuv.pixels(lay), out_ptr=out.data_ptr(), stream=s)
                e[1].record()
                e[2].record()
                assert hip.hipMemcpyAsync(C.c_void_p(scratch.data_ptr() + half + (-half) % 256), C.c_void_p(scratch.data_ptr()), half, 3, C.c_void_p(s)) == 0
                e[3].record()
                e[3].synchronize()
                if rep >= WARMUP:
                    res[key]["ms"].append(e[0].elapsed_time(e[1]))
                    res[key]["copy_ms"].append(e[2].elapsed_time(e[3]))
                res[key].update(algorithmic_bytes=nbytes, frames=N, size="%dx%d" % (w, h))
    assert batches["grey"].ui_state() == (N, False)                 # the grey path never made the RGBA slab
    for r in res.values():
        med, cmed = sorted(r["ms"])[len(r["ms"]) // 2], sorted(r["copy_ms"])[len(r["copy_ms"]) // 2]
        r.update(median_ms=med, lo_ms=min(r["ms"]), hi_ms=max(r["ms"]), algorithmic_gb_per_s=r["algorithmic_bytes"] / (med * 1e-3) / 1e9,
                 copy_median_ms=cmed, copy_gb_per_s=r["algorithmic_bytes"] / (cmed * 1e-3) / 1e9, time_over_copy=med / cmed,
                 share_of_hbm_peak=r["algorithmic_bytes"] / (med * 1e-3) / HBM_PEAK, frames_per_s=N / (med * 1e-3))
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), roi=[rw, rh], configs=res)))
    for fb in batches.values():
        fb.close()
    v.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.leg:
        return leg()
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--leg"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit("exit %d: the measurement failed%s" % (r.returncode, " (the time limit)" if r.returncode in (124, 137) else ""))
    m = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    c = m["configs"]
    grey_over_rgba = {lay: c["ui_map %dx%d grey %s" % (m["roi"][0], m["roi"][1], lay)]["median_ms"] / c["ui_map %dx%d colour %s" % (m["roi"][0], m["roi"][1], lay)]["median_ms"]
                      for lay in ("nv12", "i420")}
    out = dict(what="smhv_batch_video: %d frames per call, median of %d timed calls after %d warm-up calls, configurations in turn, one process" % (N, REPS, WARMUP),
               device=m["device"], configs=c, grey_time_over_rgba_time=grey_over_rgba, wall_s=round(time.time() - t0, 1))
    print(json.dumps({k: dict(median_ms=round(x["median_ms"], 4), algorithmic_gb_per_s=round(x["algorithmic_gb_per_s"], 1), copy_gb_per_s=round(x["copy_gb_per_s"], 1))
                      for k, x in c.items()} | dict(grey_time_over_rgba_time=grey_over_rgba)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
