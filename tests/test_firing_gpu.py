"""Firing solutions on the device against the restatement (tests/firing_ref.py): the per-call path (random and edge-case lines,
the golden fixtures' lines), SMHV_STAGE_FIRING through a batch and both pipeline schedules, heightmap switching and lifetime, and
the heightmap colour map."""
import math
import os

import numpy as np
import pytest

import firing_ref as R
from fixtures import GOLDEN, MANIFEST

pytestmark = pytest.mark.gpu

HM_W, HM_H = 1000, 700
HM_BOUNDS = ((37, -21), (51000, 49000))
HM_SCALE = (100.0, 100.0, 25.0)


def _hm_data(seed=1, w=HM_W, h=HM_H):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, size=(h, w), dtype=np.uint16)


def _ulps(a, b):
    ia, ib = np.array([a], np.float64).view(np.int64)[0], np.array([b], np.float64).view(np.int64)[0]
    return abs(int(ia) - int(ib))


def _check_line(got, want, ctx):
    assert int(got["source"]) == want["source"], ctx
    assert float(got["meters"]) == want["meters"] or (math.isnan(got["meters"]) and math.isnan(want["meters"])), (ctx, got["meters"], want["meters"])
    assert float(got["alt_delta"]) == want["alt_delta"], (ctx, got["alt_delta"], want["alt_delta"])
    for k in range(2):
        g, w = float(got["mils"][k]), want["mils"][k]
        assert math.isnan(g) == math.isnan(w), (ctx, k, g, w)
        if not math.isnan(w):
            assert _ulps(g, w) <= 4, (ctx, k, g, w)
    gb = (float(got["bearing"][0]), float(got["bearing"][1]))
    wb = (float(want["bearing"][0]), float(want["bearing"][1]))
    if gb != wb:
        # the device's atan2f may differ from the host libm's by an ulp: only where that moves the rounding
        p0x, p0y, p1x, p1y = want["p"]
        a = R.atan2f(np.float32(p0y - p1y), np.float32(p0x - p1x))
        alt = {tuple(float(v) for v in R.bearings(p0x, p0y, p1x, p1y, angle=np.nextafter(a, np.float32(s)))) for s in (-10, 10)}
        assert gb in alt, (ctx, gb, wb)
        return 1
    return 0


def _random_lines(rng, n):
    lines = rng.uniform(-60.0, 820.0, size=(n, 4)).astype(np.float32)
    edge = np.array([[100, 50, 700, 650], [99.6, 50, 700, 649.4], [99.4, 49.4, 700.6, 650.6], [-3.5, -7.25, 120, 80], [100, 50, 100, 50],
                     [700, 650, 100, 50], [100, 349.5, 700, 349.5], [0, 0, 0, 0], [650, 60, 110, 640]], np.float32)
    return np.concatenate([edge, lines])


def test_per_call_matches_the_restatement(vision):
    import squad_mortar_helper_amd as smh
    rng = np.random.default_rng(11)
    lines = _random_lines(rng, 5000)
    data = _hm_data()
    hm = smh.Heightmap(vision, data, HM_BOUNDS, HM_SCALE)
    ref_hm = (data, HM_BOUNDS, HM_SCALE)
    mm = (100, 700, 50, 650)
    cases = [dict(mpx=None, minimap=mm, hm=True, fit=True, vp=None), dict(mpx=1.7, minimap=mm, hm=True, fit=False, vp=None),
             dict(mpx=3.9, minimap=mm, hm=True, fit=False, vp=(1.37, 0.81, -12.5, 33.0)), dict(mpx=0.9, minimap=None, hm=True, fit=True, vp=None),
             dict(mpx=2.3, minimap=mm, hm=False, fit=True, vp=(0.5, 0.5, 4.0, 4.0)), dict(mpx=None, minimap=None, hm=False, fit=True, vp=None)]
    seen, nan_ranges, ambiguous = set(), 0, 0
    for ci, c in enumerate(cases):
        got = vision.firing_solutions(lines, mpx=c["mpx"], minimap=c["minimap"], heightmap=hm if c["hm"] else None,
                                      fit_to_minimap=c["fit"], viewport=c["vp"])
        assert got.shape == (len(lines),)
        for i, ln in enumerate(lines):
            met = R.record_meters(ln, c["mpx"]) if c["mpx"] is not None else None
            want = R.firing_line(tuple(float(v) for v in ln), c["minimap"], met, ref_hm if c["hm"] else None, c["fit"], c["vp"])
            ambiguous += _check_line(got[i], want, (ci, i, ln))
            seen.add(want["source"])
            nan_ranges += math.isnan(want["mils"][0]) and math.isnan(want["mils"][1]) and want["meters"] > 1232.25
    assert seen == {R.NONE, R.SCALES, R.HEIGHTMAP} and nan_ranges > 100 and ambiguous <= 3
    # zero lines, and the options' validation
    assert vision.firing_solutions(np.zeros((0, 4), np.float32)).shape == (0,)
    hm.close()


def test_golden_fixture_lines_through_the_per_call_path(vision):
    import squad_mortar_helper_amd as smh
    data = _hm_data(seed=5, w=640, h=480)
    hm = smh.Heightmap(vision, data, ((-15, 9), (0, 0)), (1.0, 1.0, 40.0))
    n_fixtures = 0
    for stem, e in sorted(MANIFEST.items()):
        path = os.path.join(GOLDEN, stem + ".golden.npz")
        g = dict(np.load(path)) if os.path.exists(path) else {}
        if "lines" not in g or len(g["lines"]) == 0 or "map_rect" not in e:
            continue
        n_fixtures += 1
        lines = np.asarray(g["lines"], np.float32).reshape(-1, 4)
        w, h = e["map_rect"][2], e["map_rect"][3]
        mm = (w // 8, w - w // 8, h // 10, h - h // 7)
        for mpx in ([e["mpx"], None] if "mpx" in e else [None]):
            for fit in (True, False):
                got = vision.firing_solutions(lines, mpx=mpx, minimap=mm, heightmap=hm, fit_to_minimap=fit)
                for i, ln in enumerate(lines):
                    met = R.record_meters(ln, mpx) if mpx is not None else None
                    want = R.firing_line(tuple(float(v) for v in ln), mm, met, (data, ((-15, 9), (0, 0)), (1.0, 1.0, 40.0)), fit)
                    _check_line(got[i], want, (stem, mpx, fit, i))
    assert n_fixtures >= 10
    hm.close()


def _frames_with_minimaps(N, first_idx):
    """Synthetic 1080p frames; most get a flat minimap rectangle with a marker line drawn inside one quadrant of it (the four
    walks of find_minimap cross the centre row and column only), frame N-1 is closed."""
    from squad_mortar_helper_amd import synth
    import squad_mortar_helper_amd as smh
    W, H = 1920, 1080
    frames, infos = synth.make_batch(W, H, N, first_idx=first_idx)
    x, y, rw, rh = smh.map_bounds(W, H)
    rng = np.random.default_rng(first_idx)
    colour = np.array(synth.TEAM_RGB[0], np.uint8)[::-1]
    for i in range(N - 1):
        if i % 4 == 3:
            continue                                            # no rectangle: no minimap on this frame
        l, r = int(rng.integers(10, 60)), int(rng.integers(rw - 60, rw - 10))
        t, b = int(rng.integers(10, 60)), int(rng.integers(rh - 60, rh - 10))
        frames[i, y + t:y + b, x + l:x + r, :3] = (40 + 4 * i, 90, 120)
        # a marker line inside the top-left quadrant of the rectangle, clear of its edges and of the centre row / column
        p0 = np.array([l + 60 + 5 * i, t + 60 + 3 * i], float)
        p1 = np.array([rw // 2 - 40, rh // 2 - 50 - 2 * i], float)
        ts = np.linspace(0.0, 1.0, int(np.hypot(*(p1 - p0)) * 2) + 1)
        xs, ys = np.rint(p0[0] + (p1[0] - p0[0]) * ts).astype(int), np.rint(p0[1] + (p1[1] - p0[1]) * ts).astype(int)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                frames[i, y + ys + dy, x + xs + dx, :3] = colour
        cx, cy = int(p0[0]), int(p0[1])
        frames[i, y + cy - 11:y + cy + 11, x + cx - 11:x + cx + 11, :3] = colour
    frames[N - 1], _ = synth.make_frame(W, H, first_idx + N - 1, map_open=False)
    # frames 2 mod 3 have no scale labels: no m/px
    anchors = [(inf["scales_start_y"], inf["anchors"] if i % 3 != 2 else []) for i, inf in enumerate(infos)]
    return frames, smh.make_anchors(anchors)


def _check_slab(recs, n_lines, slab, ref_hm, fit, vp, ctx):
    seen, ambiguous = set(), 0
    for f, rec in enumerate(recs):
        assert int(n_lines[f]) == rec["n_lines"], (ctx, f)
        want = R.firing_frame(rec, ref_hm, fit, vp)
        for l, w in enumerate(want):
            ambiguous += _check_line(slab[f, l], w, (ctx, f, l))
            seen.add(w["source"])
        for l in range(len(want), slab.shape[1]):
            assert bytes(slab[f, l].tobytes()) == bytes(48), (ctx, f, l)
    assert ambiguous <= 1, (ctx, ambiguous)                   # a neighbouring degree only where atan2f's last ulp decides it
    return seen


def test_stage_firing_on_a_batch_without_a_binding(vision):
    """A batch nobody called set_firing on: no heightmap, default options (identity viewport) -- the scales branch or none."""
    import torch
    import squad_mortar_helper_amd as smh
    N = 16
    frames, anchors = _frames_with_minimaps(N, 1700)
    d = torch.from_numpy(frames).cuda()
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_FIRING, anchors=anchors, stream=torch.cuda.current_stream().cuda_stream)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    nl, slab = fb.read_firing(0, N)
    assert _check_slab(recs, nl, slab, None, True, None, "unbound batch") == {R.NONE, R.SCALES}
    # the bearings are the lines' own (a zero viewport scale would put every end point at the origin: 270 / 90 everywhere)
    bearings = {(float(slab[f, l]["bearing"][0]), float(slab[f, l]["bearing"][1])) for f in range(N) for l in range(int(nl[f]))}
    assert len(bearings) > 4, bearings
    fb.close()


def test_stage_firing_through_batch_and_both_pipeline_schedules(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 24
    frames, anchors = _frames_with_minimaps(N, 900)
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    data = _hm_data(seed=7, w=800, h=600)
    hm = smh.Heightmap(vision, data, ((-40, 25), (0, 0)), (1.0, 1.0, 30.0))
    ref_hm = (data, ((-40, 25), (0, 0)), (1.0, 1.0, 30.0))
    base = smh.STAGE_ALL | smh.STAGE_MINIMAP
    # a plain batch: records without and with FIRING are byte-identical
    fb = smh.FrameBatch(vision, 1920, 1080, N)
    fb.run(d.data_ptr(), N, stages=base, anchors=anchors, stream=s)
    plain = bytes(fb.read_results(0, N))
    vp = (1.25, 1.25, -30.0, 12.0)
    fb.set_firing(hm, fit_to_minimap=False, viewport=vp)
    fb.run(d.data_ptr(), N, stages=base | smh.STAGE_FIRING, anchors=anchors, stream=s)
    recs_raw = fb.read_results(0, N)
    assert bytes(recs_raw) == plain
    recs = smh.results_to_dicts(recs_raw)
    nl, slab = fb.read_firing(0, N)
    seen = _check_slab(recs, nl, slab, ref_hm, False, vp, "batch")
    assert seen == {R.NONE, R.SCALES, R.HEIGHTMAP}, seen
    # FIRING without MINIMAP: every line takes the scales branch (or none)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_FIRING, anchors=anchors, stream=s)
    recs2 = smh.results_to_dicts(fb.read_results(0, N))
    nl2, slab2 = fb.read_firing(0, N)
    assert R.HEIGHTMAP not in _check_slab(recs2, nl2, slab2, ref_hm, False, vp, "batch, no minimap")
    with pytest.raises(smh.VisionError):
        fb.run(d.data_ptr(), N, stages=smh.STAGE_UI_MAP | smh.STAGE_FIRING, stream=s)
    fb.close()
    # both pipeline schedules: depth 2 batch-granular, depth 3 frame-granular
    for depth, search in ((2, "batch"), (3, "frame")):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=depth, search=search)
        p.set_firing(hm)
        slots = [p.submit(d.data_ptr(), N, stages=base | smh.STAGE_FIRING, anchors=anchors) for _ in range(depth + 1)]
        p.wait()
        for sl in set(slots):
            raw = p.slots[sl].read_results(0, N)
            assert bytes(raw) == plain, (search, sl)
            nl, slab = p.slots[sl].read_firing(0, N)
            assert _check_slab(smh.results_to_dicts(raw), nl, slab, ref_hm, True, None, search) == {R.NONE, R.SCALES, R.HEIGHTMAP}
        p.close()
    hm.close()


def test_switching_heightmaps_between_submissions_and_destroying_a_bound_one(vision):
    import torch
    import squad_mortar_helper_amd as smh
    N = 12
    frames, anchors = _frames_with_minimaps(N, 1300)
    d = torch.from_numpy(frames).cuda()
    a_data, b_data = _hm_data(seed=21, w=500, h=400), _hm_data(seed=22, w=900, h=300)
    A = smh.Heightmap(vision, a_data, ((0, 0), (0, 0)), (1.0, 1.0, 10.0))
    B = smh.Heightmap(vision, b_data, ((0, 0), (0, 0)), (1.0, 1.0, 70.0))
    ref = {"A": (a_data, ((0, 0), (0, 0)), (1.0, 1.0, 10.0)), "B": (b_data, ((0, 0), (0, 0)), (1.0, 1.0, 70.0)), None: None}
    stages = smh.STAGE_ALL | smh.STAGE_MINIMAP | smh.STAGE_FIRING
    def check(p, sl, key, ctx):
        raw = p.slots[sl].read_results(0, N)
        nl, slab = p.slots[sl].read_firing(0, N)
        seen = _check_slab(smh.results_to_dicts(raw), nl, slab, ref[key], True, None, ctx)
        assert (R.HEIGHTMAP in seen) == (key is not None), (ctx, seen)

    for search in ("batch", "frame"):
        p = smh.Pipeline(vision, 1920, 1080, N, depth=3, search=search)
        A2 = smh.Heightmap(vision, a_data, ((0, 0), (0, 0)), (1.0, 1.0, 10.0))
        p.set_firing(A2)
        A2.close()                                              # destroyed while bound: the pipeline keeps its own reference
        s0 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        p.set_firing(B)
        s1 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        p.set_firing(None)
        s2 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        p.wait(s0)
        check(p, s0, "A", (search, "A"))
        # the fourth submission takes slot 0 again, with another heightmap than its first (s1 and s2 may still be at work):
        # the slot's parameter block is the new one, and the slot's last reference of A2 goes with this rebinding
        p.set_firing(B)
        s3 = p.submit(d.data_ptr(), N, stages=stages, anchors=anchors)
        assert s3 == s0
        p.wait()
        for sl, key in ((s1, "B"), (s2, None), (s3, "B")):
            check(p, sl, key, (search, sl, key))
        p.close()
    A.close(); B.close()


def test_color_map_matches_the_restatement(vision):
    import squad_mortar_helper_amd as smh
    rng = np.random.default_rng(4)
    maps = [rng.integers(1, 60000, size=(700, 1000), dtype=np.uint16), np.full((33, 17), 4242, np.uint16),
            rng.integers(0, 65536, size=(129, 257), dtype=np.uint16)]
    maps[2][5, 7] = 0
    for i, m in enumerate(maps):
        hm = smh.Heightmap(vision, m, ((0, 0), (0, 0)), (1.0, 1.0, 1.0))
        got = hm.color_map()
        assert got.shape == m.shape + (4,) and np.array_equal(got, R.color_map(m)), i
        hm.close()
