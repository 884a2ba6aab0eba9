"""find_scale_width on the device (csrc/smh_record.inc) against the oracle, on every way the code is reached: the per-call
path (k_scale_ratio, with its `bars` output), a batch whose record is written by k_lsd_tile's workgroups, by
k_scales_finalize behind the minimap kernel and without any search, and both pipeline schedules (the search service's one
wave per frame included).  The cases are those of tests/scale_cases.py; tests/test_scale_host.py holds the oracle to the
sequential restatement of mpx_ratio.rs on the same cases.  Everything is exact: == on the f64 ratio, equality on integers."""
import numpy as np
import pytest

import scale_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


def _groups_of_cases(cases):
    """[(img, [[anchor, ...], ...])]: the single-anchor cases of one image, up to three to a call."""
    by_img = {}
    for c in cases:
        by_img.setdefault(id(c["img"]), (c["img"], []))[1].append(c["anchor"])
    return [(img, [an[j:j + 3] for j in range(0, len(an), 3)]) for img, an in by_img.values()]


def _per_call(vision, o, size, groups):
    """Every call of every group through load_frame / crop_to_map / find_scales_preprocess(0) / calc_meters_to_px_ratio:
    ratio == the oracle's, each bar row (left, y, right, 1), or (0, 0, 0, 0) where the oracle says None."""
    found = 0
    for i, (img, calls) in enumerate(groups):
        vision.load_frame(S.frame_of(img, size, i))
        assert vision.crop_to_map() is not None
        assert np.array_equal(vision.find_scales_preprocess(0), img), (size, i)
        for anchors in calls:
            got, bars = vision.calc_meters_to_px_ratio(anchors, want_bars=True)
            want = o.calc_meters_to_px_ratio(anchors, img)
            assert got == want and (got is None) == (want is None), (size, i, anchors, got, want)
            assert len(bars) == len(anchors)
            for (m, x, y), bar in zip(anchors, bars):
                one = o.find_scale_width(m, x, y, img)
                want_bar = (0, 0, 0, 0) if one is None else (one[1][0], one[1][1], one[1][2], 1)
                assert tuple(int(v) for v in bar) == want_bar, (size, i, (m, x, y), bar, want_bar)
                found += one is not None
    return found


@pytest.mark.parametrize("size", [S.BIG, S.SMALL])
def test_per_call_fixed_cases(vision, o, size):
    cases = S.fixed_cases(size)
    assert _per_call(vision, o, size, _groups_of_cases(cases)) == len(cases) - len(S.NONE_NAMES)


def test_per_call_ladder_outcomes(vision, o):
    img, calls = S.ladder()
    assert _per_call(vision, o, S.BIG, [(img, calls)]) == 12 + 4
    vision.load_frame(S.frame_of(img, S.BIG))
    assert vision.crop_to_map() is not None
    vision.find_scales_preprocess(0)
    assert vision.calc_meters_to_px_ratio(calls[7]) == S.LADDER_MEAN          # (all three succeed: summed in index order)


def test_per_call_random_images(vision, o):
    images, stats = S.random_images()
    groups = [(img, [an[j:j + 3] for j in range(0, len(an), 3)]) for img, an in images]
    assert _per_call(vision, o, S.BIG, groups) == stats["found"]


# ---- the batch paths -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(vision, o):
    """One batch at 2560 x 1440: frame i < 70 is fixed case i's frame with its one anchor; then the ladder's twelve outcomes
    (two or three anchors); then two random images with eight single-anchor frames each.  Every distinct frame is uploaded
    once and copied to its places on the device.  `white`: as many frames whose quadrant is all white."""
    import torch
    import squad_mortar_helper_amd as smh
    W, H = S.BIG
    plan = [(c["img"], [c["anchor"]]) for c in S.fixed_cases(S.BIG)]
    limg, lcalls = S.ladder()
    plan += [(limg, anchors) for anchors in lcalls]
    for img, anchors in S.random_images()[0][:2]:
        plan += [(img, [an]) for an in anchors[:8]]
    N = len(plan)
    want = [o.calc_meters_to_px_ratio(anchors, img) for img, anchors in plan]
    assert sum(w is not None for w in want) > N // 2 and sum(w is None for w in want) > 12
    places = {}
    for i, (img, _) in enumerate(plan):
        places.setdefault(id(img), (img, []))[1].append(i)
    d = torch.empty((N, H, W, 4), dtype=torch.uint8, device="cuda")
    for k, (img, idx) in enumerate(places.values()):
        d[torch.tensor(idx, device="cuda")] = torch.from_numpy(S.frame_of(img, S.BIG, k)).cuda()
    white = torch.from_numpy(S.frame_of(S.blank(S.BIG), S.BIG, 1)).cuda().unsqueeze(0).repeat(N, 1, 1, 1)
    torch.cuda.synchronize()
    w = dict(N=N, d=d, white=white, want=want, anchors=smh.make_anchors([(0, anchors) for _, anchors in plan]))
    yield w
    w.clear()
    del d, white
    torch.cuda.empty_cache()


def _check_records(recs, want, ctx):
    assert len(recs) == len(want)
    for i, (r, w) in enumerate(zip(recs, want)):
        assert r.map_open == 1 and r.status == 0, (ctx, i)
        assert bool(r.has_mpx) == (w is not None), (ctx, i, r.has_mpx, r.mpx, w)
        assert r.mpx == (w if w is not None else 0.0), (ctx, i, r.mpx, w)


@pytest.mark.parametrize("path", ["lsd_tile", "scales_finalize", "no_search"])
def test_batch_paths(vision, world, path):
    """STAGE_ALL: k_lsd_tile's workgroups write the record; with STAGE_MINIMAP: k_scales_finalize; OCR + SCALES only: no search
    at all.  Then the same batch object on all-white quadrants: no record keeps a ratio of the run before."""
    import torch
    import squad_mortar_helper_amd as smh
    stages = {"lsd_tile": smh.STAGE_ALL, "scales_finalize": smh.STAGE_ALL | smh.STAGE_MINIMAP, "no_search": smh.STAGE_OCR | smh.STAGE_SCALES}[path]
    N, s = world["N"], torch.cuda.current_stream().cuda_stream
    fb = smh.FrameBatch(vision, S.BIG[0], S.BIG[1], N)
    fb.run(world["d"].data_ptr(), N, stages=stages, anchors=world["anchors"], stream=s)
    _check_records(fb.read_results(0, N), world["want"], path)
    fb.run(world["white"].data_ptr(), N, stages=stages, anchors=world["anchors"], stream=s)
    _check_records(fb.read_results(0, N), [None] * N, (path, "white"))
    fb.close()


@pytest.mark.parametrize("search", ["batch", "frame"])
def test_pipeline_schedules(vision, world, search):
    """Pipeline(depth=4) with the batch-granular search and with the frame-granular search service (frame_record_tail_wave: one
    wave takes all three anchors); every slot, then every slot again on all-white quadrants."""
    import squad_mortar_helper_amd as smh
    N = world["N"]
    p = smh.Pipeline(vision, S.BIG[0], S.BIG[1], N, depth=4, search=search)
    for frames, want, tag in ((world["d"], world["want"], "cases"), (world["white"], [None] * N, "white")):
        slots = [p.submit(frames.data_ptr(), N, stages=smh.STAGE_ALL, anchors=world["anchors"]) for _ in range(4)]
        p.wait()
        assert sorted(slots) == [0, 1, 2, 3]
        for sl in slots:
            _check_records(p.slots[sl].read_results(0, N), want, (search, tag, sl))
    st = p.search_stats()
    if search == "frame":
        assert st is not None and st["mode"] == "frame-granular" and st["frames"] == 8 * N and st["submissions"] == 8, st
    else:
        assert st is None
    p.close()
