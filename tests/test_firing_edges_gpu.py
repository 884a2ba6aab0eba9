"""The crafted firing and label cases (tests/firing_edge_cases.py) on the device: smhv_firing_solutions on every case, the per-call
label path (smhv_render_map_labeled) on every case that prints, and the batch's label path (smhv_batch_render_labels, the
per_call == 0 side of k_label_plan) on the heightmap families under every scene's own rectangle.

Source, meters and alt_delta bit-equal to the restatement (NaN matching NaN), mils within 4 ulps of glibc's atan (the bound
tests/test_firing_gpu.py holds the device's atan to) with NaN exactly where the restatement has NaN, bearings equal with NO
allowance for atan2f's last ulp (every case's check, and the check of the batch's lines, asserts on the CPU for every line that an
ulp either way changes nothing and that no finite mils value is within 1e-6 of a .5), label rows equal to the literal bytes of the
case, where it types them, and to label_ref's rows and layout for the restated numbers."""
import math

import numpy as np
import pytest

import firing_edge_cases as E
import label_ref as LR
import minimap_scenes as S

pytestmark = pytest.mark.gpu

WINDOW = (257, 128)
BG = (12, 34, 56, 255)
N = S.N_SCENES
RW, RH = 360, 585
f32 = np.float32
CASES = E.cases()


def _bits(v):
    return np.array([v], np.float64).view(np.uint64)[0]


def _same_f64(got, want):
    return (got != got and want != want) or _bits(got) == _bits(want)


def _compare(got, want, ctx):
    """One smhv_firing (a numpy record) against the restatement's dict."""
    assert int(got["source"]) == want["source"], (ctx, int(got["source"]), want["source"])
    assert _same_f64(float(got["meters"]), float(want["meters"])), (ctx, "meters", float(got["meters"]).hex(), float(want["meters"]).hex())
    assert _same_f64(float(got["alt_delta"]), float(want["alt_delta"])), (ctx, "alt_delta", float(got["alt_delta"]), want["alt_delta"])
    for k in range(2):
        g, w = float(got["mils"][k]), float(want["mils"][k])
        assert math.isnan(g) == math.isnan(w), (ctx, "mils", k, g, w)
        if not math.isnan(w):
            assert abs(int(_bits(g)) - int(_bits(w))) <= 4, (ctx, "mils", k, g, w)
        gb, wb = float(got["bearing"][k]), float(want["bearing"][k])
        assert gb == wb or (gb != gb and wb != wb), (ctx, "bearing", k, gb, wb)


@pytest.fixture(scope="module")
def hms(vision):
    import squad_mortar_helper_amd as smh
    maps = {name: smh.Heightmap(vision, data, bounds, scale) for name, (data, bounds, scale) in E.heightmaps().items()}
    yield maps
    for hm in maps.values():
        hm.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s: %s" % (c.family, c.name))
def test_firing_solutions_on_every_case(vision, hms, case):
    wants = E.restate(case)
    case.check(case, wants)
    got = vision.firing_solutions(np.array(case.lines, np.float32), mpx=case.mpx, minimap=case.minimap, heightmap=hms[case.hm] if case.hm else None,
                                  fit_to_minimap=case.fit, viewport=case.viewport)
    assert got.shape == (len(case.lines),)
    for i, (want, _) in enumerate(wants):
        _compare(got[i], want, (case, i, case.lines[i]))


# ---- the label paths ------------------------------------------------------------------------------------------------------------
def _viewport(vp):
    import squad_mortar_helper_amd as smh
    sw, sh, tx, ty = vp or (1.0, 1.0, 0.0, 0.0)
    return smh.MapViewport((tx, ty, tx + RW * (sw or 1.0), ty + RH * (sh or 1.0)), (sw, sh), (tx, ty))


def _check_slot(lab, line, want, vp, rows, ctx):
    """A slot of the device against the restated numbers, label_ref's slot for THOSE numbers, and the literal rows (None: not given)."""
    from squad_mortar_helper_amd import _lib as L
    _compare(np.frombuffer(bytes(lab)[:48], L.firing_dtype(), count=1)[0], want, ctx)
    slot = LR.format_label(line, want, vp, E.MAGENTA)
    runs = [(r.x2, r.y2, bytes(r.text[:r.n])) for r in lab.run[:lab.n_runs]]
    assert runs == slot["runs"], (ctx, runs, slot["runs"])
    if rows is not None:
        assert [r[2] for r in runs] == rows, (ctx, runs, rows)
    for r in lab.run[:lab.n_runs]:                               # a row arrives whole: its bytes, then zeros
        assert r.n <= 16 and bytes(r.text[r.n:]) == bytes(16 - r.n), (ctx, bytes(r.text))
    for r in lab.run[lab.n_runs:]:
        assert (r.x2, r.y2, r.n, bytes(r.text)) == (0, 0, 0, bytes(16)), ctx
    got = np.array([lab.mid[0], lab.mid[1], lab.dir[0], lab.dir[1]], np.float32)
    ref = np.array([slot["mid"][0], slot["mid"][1], slot["dir"][0], slot["dir"][1]], np.float32)
    assert got.tobytes() == ref.tobytes() and tuple(lab.rgba) == E.MAGENTA, (ctx, got, ref)
    return len(runs)


@pytest.fixture(scope="module")
def scenes(vision):
    """The scenes of tests/minimap_scenes.py in a plain batch that has run once (records with the rectangles and the m/px), and
    scene 0 as the current frame of the per-call path."""
    import torch
    import squad_mortar_helper_amd as smh
    frames, anchor_list, rects, names = S.make_scenes()
    d = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, S.W, S.H, N)
    assert tuple(fb.roi[2:]) == (RW, RH)
    fb.run(d.data_ptr(), N, stages=smh.STAGE_ALL | smh.STAGE_MINIMAP, grayscale=False, anchors=smh.make_anchors(anchor_list), stream=s)
    recs = smh.results_to_dicts(fb.read_results(0, N))
    for f in range(N):
        assert not recs[f]["map_open"] or recs[f]["minimap"] == rects[f], (f, names[f])
    vision.load_frame(frames[0])
    assert vision.crop_to_map(grayscale=False) is not None
    assert vision.find_minimap() == E.SCENE_RECT
    yield dict(fb=fb, s=s, recs=recs, rects=rects, names=names, d=d)
    fb.close()


def _label_groups():
    groups = {}
    for c in CASES:
        if c.rows is not None:
            groups.setdefault(c.group + (c.silent,), []).append(c)
    return list(groups.values())


def test_the_per_call_label_path_on_every_case_that_prints(vision, hms, scenes):
    """One call per distinct (mpx, heightmap, fit, viewport); cases that print nothing go into calls of their own, whose image
    must be the render without labels."""
    import squad_mortar_helper_amd as smh
    ow, oh = WINDOW
    n_calls = n_16 = n_silent = tie_lines = 0
    base = {}
    for group in _label_groups():
        c0 = group[0]
        view = _viewport(c0.viewport)
        opt = smh.render_options(view, ow, oh, fit_to_minimap=c0.fit, background=BG)
        key = (c0.viewport, c0.fit)
        if key not in base:
            base[key] = vision.render_map(view, ow, oh, options=opt)
        lines = [ln for c in group for ln in c.lines]
        assert len(lines) <= 64
        hm = hms[c0.hm] if c0.hm else None
        lo = smh.LabelOptions([(ln, E.MAGENTA) for ln in lines], detected=False, scale=1, mpx=c0.mpx)
        got, res = vision.render_map(view, ow, oh, heightmap=hm, options=opt, labels=lo)
        n_calls += 1
        assert res.n_labels == len(lines), (group, res.n_labels)
        i = printed = 0
        for c in group:
            wants = E.restate(c, minimap=E.SCENE_RECT)
            for ln, (want, _), rows in zip(c.lines, wants, c.rows):
                n_runs = _check_slot(res.label[i], ln, want, E.label_viewport(c), rows, (c, ln))
                assert n_runs > 0 or rows == [], (c, ln)         # (rows is None: the line prints, its rows are label_ref's)
                printed += n_runs
                n_16 += sum(len(r) == 16 for r in rows or [])
                tie_lines += c.family == "ties" and want["source"] == LR.HEIGHTMAP
                i += 1
        if c0.silent:
            assert printed == 0 and np.array_equal(got, base[key]), group
            n_silent += 1
        else:
            assert printed > 0 and got.shape == base[key].shape
    assert n_calls == len(_label_groups()) >= 15 and n_16 == 4 and n_silent >= 4 and tie_lines >= 3 * 24, (n_calls, n_16, n_silent, tie_lines)


def test_the_batch_label_path_on_the_heightmap_families(vision, scenes):
    """Every open scene under two heightmaps of its own rectangle's size: texel ties found on that rectangle, altitudes that tell
    trunc from round and floor, RANGE! on one side, both saturations -- slots against the restatement with the record's rectangle
    and m/px."""
    import squad_mortar_helper_amd as smh
    fb, s, recs = scenes["fb"], scenes["s"], scenes["recs"]
    ow, oh = WINDOW
    view = _viewport(None)
    opt = smh.render_options(view, ow, oh, background=BG)
    fb.render(view, ow, oh, options=opt, stream=s)
    sources, sixteen = set(), 0
    for f in range(N):
        rec = recs[f]
        if not rec["map_open"]:
            continue
        rect = rec["minimap"]
        W, H = rect[1] - rect[0], rect[3] - rect[2]
        lines, check = E.batch_lines(rect, W, H)
        case = E.Case("frame %d" % f, "ties", lines, None, mpx=rec["mpx"], minimap=rect)
        maps = E.batch_heightmaps(W, H)
        wants = {k: E.restate(case, hm=maps[k]) for k in maps}
        check(wants["steep"], wants["sat"])
        lo = smh.LabelOptions([(ln, E.MAGENTA) for ln in case.lines], detected=False, scale=1)
        for k, (data, bounds, scale) in maps.items():
            hm = smh.Heightmap(vision, data, bounds, scale)
            fb.render_labels(opt, lo, first=f, n=1, heightmap=hm, stream=s)
            res = fb.read_labels(f, 1)[0]
            hm.close()
            assert res.n_labels == len(lines), (f, k)
            for i, (ln, (want, _)) in enumerate(zip(case.lines, wants[k])):
                _check_slot(res.label[i], ln, want, (1.0, 1.0, 0.0, 0.0), None, (scenes["names"][f], k, i, ln))
                sources.add(want["source"])
                sixteen += sum(r.n == 16 for r in res.label[i].run[:res.label[i].n_runs])
    assert sources == {LR.NONE, LR.SCALES, LR.HEIGHTMAP} and sixteen >= 2 * (N - 1), (sources, sixteen)
