"""What the map grid costs: smhv_batch_grid (k_grid) over 256 frames at a 1920 x 1080 window in each of its forms, beside the
same-shaped form of smhv_batch_relief (k_relief, a 4096 x 4096 heightmap, its default options) in the same process, and
smhv_batch_grid_refs (k_grid_refs) over the same frames.

  python tools/grid_cost.py --out profiles/grid_cost.json

Every leg is a child process of its own under `timeout -k 10`; a child that fails or runs out of time ends the job.  Inside a leg the
two launches -- grid, relief -- take turns in every round, each between two events on one stream, after WARMUP rounds that are not
counted; the figure is the median microseconds per launch and per frame.  Bytes: the grid's planes write 1 (flag byte) + 4 (cell word)
per pixel; its PAINT reads and writes only line and label pixels, so no rate is stated for it.  The planes leg also times, in the same
process, what tools/copy_ceiling.py times -- a device-to-device copy, a memset and a read of the planes' volume -- and holds the
planes-alone form against them.  The JSON names the box (host and device) the figures are from: they hold for that box, and boxes
differ by a few per cent.  Nothing depends on these figures."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 256
HM = 4096
WARMUP, REPS = 3, 15
# grid: paint, planes (bytes and cells); relief: paint, planes (bytes, shades, heights)
LEGS = {
    "paint": (True, False),
    "paint and planes": (True, True),
    "planes": (False, True),
    "refs": (False, False),
}
GRID_PLANE_BYTES = 5.0


def ceiling(torch, n):
    """tools/copy_ceiling.py's three figures at a volume of n bytes -> {name: GB/s}."""
    a = torch.empty(n, dtype=torch.uint8, device="cuda").random_(0, 255)
    b = torch.empty_like(a)
    out = {}
    for fn, name in ((lambda: b.copy_(a), "copy"), (lambda: b.zero_(), "memset"), (lambda: a.sum(dtype=torch.int64), "read")):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name + "_gb_per_s"] = n * (2 if name == "copy" else 1) / (e0.elapsed_time(e1) / 10 * 1e-3) / 1e9
    return out


def leg(name):
    import numpy as np
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import synth
    paint, planes = LEGS[name]
    refs = name == "refs"
    v = smh.HipVision.init(0)
    frames16, infos = synth.make_batch(W, H, 16, first_idx=0, n_lines=4)
    few = torch.from_numpy(frames16).cuda()
    frames = few[torch.arange(N, device="cuda") % 16].contiguous()
    del few
    anchors = smh.make_anchors([(i["scales_start_y"], i["anchors"]) for i in infos] * (N // 16))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fb = smh.FrameBatch(v, W, H, N)
    torch.cuda.synchronize()
    fb.run(frames.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=anchors, stream=s)
    st.synchronize()
    del frames
    recs = smh.results_to_dicts(fb.read_results(0, N))
    _, _, rw, rh = fb.roi
    yy, xx = np.mgrid[0:HM, 0:HM]
    data = ((np.sin(xx / 310.0) * np.cos(yy / 170.0) * 0.5 + 0.5) * 30000.0 + ((xx * 7 + yy * 13) % 512)).astype(np.uint16)
    hm = smh.Heightmap(v, data, ((0, 0), (0, 0)), (1.0, 1.0, 60.0))
    vp = smh.MapViewport.calc(W, H, rw, rh)
    opt = smh.render_options(vp, W, H, markers=True)
    go = smh.GridOptions(paint=paint, bytes=planes, cells=planes)
    lo = smh.ReliefOptions(paint=paint, bytes=planes, shades=planes, heights=planes)
    gp = dict(bytes_ptr=torch.zeros(N * W * H, dtype=torch.uint8, device="cuda") if planes else None,
              cells_ptr=torch.zeros(N * W * H, dtype=torch.int32, device="cuda") if planes else None)
    rp = dict(bytes_ptr=torch.zeros(N * W * H, dtype=torch.uint8, device="cuda") if planes else None,
              shades_ptr=torch.zeros(N * W * H, dtype=torch.uint8, device="cuda") if planes else None,
              heights_ptr=torch.zeros(N * W * H, dtype=torch.float32, device="cuda") if planes else None)
    torch.cuda.synchronize()
    fb.render(vp, W, H, options=opt, stream=s)
    st.synchronize()
    ptr = lambda d: {k: (p.data_ptr() if p is not None else None) for k, p in d.items()}
    t = dict(grid=[], relief=[])
    with torch.cuda.stream(st):
        for rep in range(WARMUP + REPS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            if refs:
                fb.grid_refs(opt, go, heightmap=hm, stream=s)
            else:
                fb.grid(opt, go, heightmap=hm, stream=s, **ptr(gp))
            e[1].record()
            e[2].record()
            if not refs:
                fb.relief(opt, lo, heightmap=hm, stream=s, **ptr(rp))
            e[3].record()
            e[3].synchronize()
            if rep >= WARMUP:
                t["grid"].append(e[0].elapsed_time(e[1]) * 1e3)
                t["relief"].append(e[2].elapsed_time(e[3]) * 1e3)
    out = dict(leg=name, box=socket.gethostname(), device=torch.cuda.get_device_name(0), roi=[rw, rh], pixels=N * W * H,
               frames_with_minimap=sum(r["minimap"] is not None for r in recs))
    if refs:
        rr = fb.read_grid_refs(0, N)
        out.update(lines=sum(int(r.n_lines) for r in rr), ends_with_a_cell=sum(int(r.ref[i][k].valid) for r in rr for i in range(int(r.n_lines)) for k in range(2)))
        del t["relief"]
    else:
        res = fb.read_grid(0, N)
        out.update(frames_valid=sum(int(r.valid) for r in res), drawn_levels=sorted(set(int(r.drawn_levels) for r in res)),
                   pixels_with_cell=sum(int(r.n_cell) for r in res), line_pixels=sum(sum(r.n_line) for r in res), label_pixels=sum(int(r.n_label) for r in res))
    for k, xs in t.items():
        xs = sorted(xs)
        out[k + "_us"] = dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])
        out[k + "_us_per_frame"] = xs[len(xs) // 2] / N
    if not refs:
        out["grid_over_relief"] = out["grid_us"]["median"] / out["relief_us"]["median"]
        out["grid_ns_per_pixel"] = out["grid_us"]["median"] * 1e3 / (N * W * H)
    if name == "planes":
        del gp, rp
        vol = int(N * W * H * GRID_PLANE_BYTES)
        out["plane_bytes"] = vol
        out["grid_gb_per_s"] = vol / (out["grid_us"]["median"] * 1e-6) / 1e9
        out["ceiling"] = ceiling(torch, vol)
        out["grid_over_memset_ceiling"] = out["grid_gb_per_s"] / out["ceiling"]["memset_gb_per_s"]
        out["grid_over_copy_ceiling"] = out["grid_gb_per_s"] / out["ceiling"]["copy_gb_per_s"]
    print(json.dumps(out))
    hm.close()
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
        print(json.dumps({name: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in legs[name].items()
                                 if k in ("grid_us_per_frame", "relief_us_per_frame", "grid_over_relief", "grid_gb_per_s", "ceiling")}}), flush=True)
    first = next(iter(legs.values()))
    out = dict(what="smhv_batch_grid: %d frames per launch at a %d x %d window, a %d x %d heightmap (the heightmap branch), the library's default options; median "
                    "microseconds per launch of %d timed rounds after %d warm-up rounds; the grid and the same-shaped form of smhv_batch_relief in turn; refs: "
                    "smhv_batch_grid_refs alone; one child process per leg; the planes leg holds its %g bytes per pixel against a copy, a memset and a read of "
                    "that volume in the same process" % (N, W, H, HM, HM, REPS, WARMUP, GRID_PLANE_BYTES),
               box=first["box"], device=first["device"], legs=legs, wall_s=round(time.time() - t0, 1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
