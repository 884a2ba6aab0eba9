"""The device against the oracle at the geometries of tests/geometry_sweep_cases.py: frame widths that are odd (rows and the
frames behind the first 4, 8 or 12 bytes off a 16-byte boundary), ROI widths and heights on the boundaries of the kernels'
layouts, every (m_xoff, q_xoff), random alpha bytes.  Everything byte for byte: no tolerance, no excluded case.

Per case three frames (open, CLOSED, open with random alpha): the per-call trait path (k_map_pass, k_brq_pass, k_lsd); plain
batches through the fused and the plain streaming pass with 8-row bands, and -- the frames repeated on the device until the
launch takes them -- full-height bands of 24 and 56 rows (smhv_debug_map_band_rows) and of the library's own rule, with both
line searches; both pipeline schedules for the width and the rh 899..902 groups; a base pointer 4, 8, 12 bytes off; the limits.
tests/test_geometry_sweep_host.py holds the oracle's outputs to the conditions that make these comparisons mean something."""
import ctypes as C

import numpy as np
import pytest

import geometry_sweep_cases as G
from tile_mask_check import check_tile_mask

pytestmark = pytest.mark.gpu
MINIMAP = 0x10


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", params=G.CASES, ids=G.IDS)
def world(request, vision, o):
    """One case: its frames on the host and on the device, the oracle's outputs (computed once), the anchors."""
    import torch
    import squad_mortar_helper_amd as smh
    c = request.param
    frames, infos, refs = G.oracle_of(c)
    d = torch.from_numpy(frames).cuda()
    w = dict(c=c, frames=frames, infos=infos, refs=refs, d=d, n=len(frames),
             per=[(i["scales_start_y"], i["anchors"]) for i in infos])
    w["anchors"] = smh.make_anchors(w["per"])
    yield w
    w.clear()
    del d
    torch.cuda.empty_cache()


def _band_rows(c, n, fused):
    from squad_mortar_helper_amd import _lib
    rows, bands, tiles = C.c_uint32(), C.c_uint32(), C.c_int()
    _lib.check(_lib.load().smhv_debug_band_rows(c.W, c.H, n, fused, C.byref(rows), C.byref(bands), C.byref(tiles)))
    return rows.value, bool(tiles.value)


def _frames_for_full_bands(c, fused, period):
    """The fewest frames (a multiple of the period) at which a launch takes the band height it takes for very many."""
    target = _band_rows(c, 1 << 16, fused)[0]
    n = period
    while _band_rows(c, n, fused)[0] != target:
        n += period
        assert n <= 1024, (c, fused, target)
    return n, target


def _check_record(r, ref, info, stages, ctx):
    assert r["status"] == 0 and r["map_open"] == ref["map_open"] and r["red_pixels"] == ref["red_pixels"], ctx
    if not ref["map_open"]:
        assert (r["n_lines"], r["n_mask_px"], r["rounds"], r["mpx"], r["minimap"]) == (0, 0, 0, None, None), ctx
        return
    if stages & 0x1:
        assert r["n_lines"] == ref["n_lines"] and np.array_equal(r["lines"], ref["lines"]), (ctx, r["n_lines"], ref["n_lines"])
        assert (r["rounds"], r["n_mask_px"]) == (ref["rounds"], ref["n_mask_px"]), (ctx, r["rounds"], ref["rounds"], r["n_mask_px"], ref["n_mask_px"])
    want_mpx = ref["mpx"] if (stages & 0x8) and info["anchors"] else None
    assert r["mpx"] == want_mpx, (ctx, r["mpx"], want_mpx)
    assert r["minimap"] == (ref["minimap"] if stages & MINIMAP else None), (ctx, r["minimap"], ref["minimap"])


def _check_images(fb, f, ref, info, stages, gray, ctx):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    if stages & 0x2:
        assert np.array_equal(fb.read_image(L.IMAGE_UI_MAP, f), ref["ui_map"] if gray else ref["ui_colour"]), (ctx, "ui_map")
    if stages & 0x1:
        assert np.array_equal(fb.read_image(L.VIEW_LSD_INPUT, f), ref["lsd"]), (ctx, "lsd")
    if stages & 0x4:
        assert np.array_equal(fb.read_image(L.VIEW_OCR_INPUT, f), ref["ocr"]), (ctx, "ocr")
    if (stages & 0x8) and info["anchors"]:
        y0 = info["scales_start_y"]
        assert np.array_equal(fb.read_image(L.VIEW_FIND_SCALES_INPUT, f)[y0:], ref["scales"][y0:]), (ctx, "scales")


def _run_and_check(vision, w, d, n, stages, gray, classic, expect_rows, image_frames, ctx):
    """One smhv_batch_run over n frames (the case's frames repeated) and everything it leaves, against the oracle."""
    import torch
    import squad_mortar_helper_amd as smh
    c, k = w["c"], w["n"]
    fused = 1 if stages & 0xE else 0
    rows, tiles = _band_rows(c, n, fused)
    assert rows == expect_rows, (ctx, rows, expect_rows)
    lib = smh._lib.load()
    lib.smhv_debug_lsd_classic(classic)
    fb = smh.FrameBatch(vision, c.W, c.H, n)
    try:
        anchors = smh.make_anchors([w["per"][i % k] for i in range(n)]) if stages & 0x8 else None
        fb.run(d.data_ptr(), n, stages=stages, grayscale=gray, max_gap=G.MAX_GAP, anchors=anchors, stream=torch.cuda.current_stream().cuda_stream)
        recs = smh.results_to_dicts(fb.read_results(0, n))
        for i in range(n):
            _check_record(recs[i], w["refs"][i % k], w["infos"][i % k], stages, (ctx, i))
        for f in image_frames:
            ref, info = w["refs"][f % k], w["infos"][f % k]
            if not ref["map_open"]:
                continue
            _check_images(fb, f, ref, info, stages, gray, (ctx, f))
            if stages & 0x1:
                check_tile_mask(fb, f, ref["lsd"], tiles, (ctx, f))
    finally:
        lib.smhv_debug_lsd_classic(0)
        fb.close()
    return recs


def test_per_call_trait_path(vision, o, world):
    """load_frame ... find_marker_lines, ocr_preprocess, find_scales_preprocess, find_minimap, calc_meters_to_px_ratio with its
    bars; grey and colour ui_map."""
    c = world["c"]
    for i, (frame, info, ref) in enumerate(zip(world["frames"], world["infos"], world["refs"])):
        vision.load_frame(frame)
        crop = vision.crop_to_map(True)
        assert vision.red_pixels() == ref["red_pixels"] and (crop is not None) == bool(ref["map_open"]), (c, i)
        if crop is None:
            continue
        assert tuple(crop[1])[2:] == (c.rw, c.rh) and np.array_equal(crop[0], ref["ui_map"]), (c, i)
        assert vision.find_minimap() == ref["minimap"], (c, i)
        vision.isolate_map_markers()
        vision.mask_marker_lines()
        assert np.array_equal(vision.lsd_image(), ref["lsd"]), (c, i)
        lines = vision.find_marker_lines(G.MAX_GAP)
        assert lines.shape == ref["lines"].shape and np.array_equal(lines, ref["lines"]), (c, i, len(lines), ref["n_lines"])
        assert vision.lsd_stats(G.MAX_GAP, exact=True) == (ref["rounds"], ref["steps"]), (c, i)
        assert np.array_equal(vision.ocr_preprocess(), ref["ocr"]), (c, i)
        y0 = info["scales_start_y"]
        assert np.array_equal(vision.find_scales_preprocess(y0)[y0:], ref["scales"][y0:]), (c, i)
        if info["anchors"]:
            got, bars = vision.calc_meters_to_px_ratio(info["anchors"], want_bars=True)
            assert got == ref["mpx"] is not None, (c, i, got, ref["mpx"])
            for (m, x, y), bar in zip(info["anchors"], bars):
                one = o.find_scale_width(m, x, y, ref["scales"])
                assert tuple(int(v) for v in bar) == (one[1][0], one[1][1], one[1][2], 1), (c, i, bar, one)
        colour = vision.crop_to_map(False)
        assert np.array_equal(colour[0], ref["ui_colour"]), (c, i)


def test_batch_with_bands_of_eight_rows(vision, world):
    """Three frames: bands of 8 rows.  The fused pass (all stages, with and without the minimap walk, grey and colour) and the plain
    pass (markers only), both line searches."""
    import squad_mortar_helper_amd as smh
    n = world["n"]
    for stages, gray in ((smh.STAGE_ALL, True), (smh.STAGE_MARKERS, True), (smh.STAGE_ALL | MINIMAP, True), (smh.STAGE_ALL, False)):
        for classic in (0, 1):
            _run_and_check(vision, world, world["d"], n, stages, gray, classic, 8, range(n) if classic == 0 else (), ("8 rows", stages, gray, classic))


@pytest.mark.parametrize("forced", [8, 24, 56, 0])
def test_batch_with_full_height_bands(vision, world, forced):
    """The case's frames repeated on the device until the launch takes full-height bands: forced to 8, 24 and 56 rows, and the
    library's own rule (24 rows up to rh = 900, 56 / 58 / 62 beyond).  Every record; the images and the tile-major mask of the
    first and the last repetition."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    c, k = world["c"], world["n"]
    _lib.check(_lib.load().smhv_debug_map_band_rows(forced))
    try:
        for stages in (smh.STAGE_ALL, smh.STAGE_MARKERS):
            n, rows = _frames_for_full_bands(c, 1 if stages & 0xE else 0, k)
            assert rows == (forced or rows) and (forced or rows in ((24,) if c.rh <= 900 else (56, 58, 62)))
            d = world["d"].repeat(n // k, 1, 1, 1)
            for classic in (0, 1):
                _run_and_check(vision, world, d, n, stages, True, classic, rows, (0, k - 1, n - k, n - 1) if classic == 0 else (), ("full", forced, rows, n, stages, classic))
            del d
    finally:
        _lib.check(_lib.load().smhv_debug_map_band_rows(0))


PIPE_CASES = {(c.W, c.H) for c in G.WIDTH_GROUP + G.HEIGHT_EDGE}


def test_pipeline_schedules(vision, world):
    """smhv_pipeline with the batch-granular search, the frame-granular search service, and the service building its tile store by
    the walk over the bit rows: every slot's records are the plain batch's and the oracle's, its images the oracle's."""
    import torch
    import squad_mortar_helper_amd as smh
    c, n = world["c"], world["n"]
    if (c.W, c.H) not in PIPE_CASES:
        return                                                       # (the width and the rh 899..902 groups)
    stages = smh.STAGE_ALL
    plain = _run_and_check(vision, world, world["d"], n, stages, True, 0, 8, (), ("plain", c))
    keys = ("map_open", "n_lines", "mpx", "n_mask_px", "red_pixels", "rounds", "minimap", "status")
    for search, flags in (("batch", 0), ("frame", 0), ("frame", smh._lib.PIPE_WALK_BIT_ROWS)):
        pipe = smh.Pipeline(vision, c.W, c.H, n, 4, search=search, flags=flags)
        try:
            slots = [pipe.submit(world["d"].data_ptr(), n, stages=stages, max_gap=G.MAX_GAP, anchors=world["anchors"]) for _ in range(5)]
            pipe.wait()
            assert slots == [0, 1, 2, 3, 0]
            for s_ in range(4):
                recs = smh.results_to_dicts(pipe.slots[s_].read_results(0, n))
                for i in range(n):
                    _check_record(recs[i], world["refs"][i], world["infos"][i], stages, (search, flags, s_, i))
                    assert all(recs[i][k_] == plain[i][k_] for k_ in keys) and np.array_equal(recs[i]["lines"], plain[i]["lines"]), (search, flags, s_, i)
                    if world["refs"][i]["map_open"] and s_ in (0, 3):
                        _check_images(pipe.slots[s_], i, world["refs"][i], world["infos"][i], stages, True, (search, flags, s_, i))
        finally:
            pipe.close()
    torch.cuda.synchronize()


def test_base_pointer_off_a_16_byte_boundary(vision, world):
    """include/smh_vision_hip.h: d_frames needs the alignment of a pixel and no more.  A frame width that is a multiple of 4 (every row
    16-byte aligned relative to the base), the frames copied into a larger allocation at byte offsets 4, 8 and 12 with a frame of
    random bytes on both sides: the oracle's outputs, from a plain batch and from both pipeline schedules.  Offsets 1, 2, 3: refused with
    SMHV_E_INVALID before anything is enqueued or counted."""
    import torch
    import squad_mortar_helper_amd as smh
    c, n = world["c"], world["n"]
    if c != G.ALIGNED_CASE:
        return
    assert c.W % 4 == 0
    fbytes = c.W * c.H * 4
    g = torch.Generator(device="cpu").manual_seed(5)
    buf = torch.randint(0, 256, ((n + 2) * fbytes + 16,), dtype=torch.uint8, generator=g).cuda()
    assert buf.data_ptr() % 16 == 0
    stages = smh.STAGE_ALL | MINIMAP

    class At:                                                                   # (what _run_and_check needs of a tensor)
        def __init__(self, off):
            self.off = off

        def data_ptr(self):
            return buf.data_ptr() + fbytes + self.off
    for off in (4, 8, 12):
        buf[fbytes + off:fbytes + off + n * fbytes] = world["d"].reshape(-1)
        torch.cuda.synchronize()
        for st in (stages, smh.STAGE_MARKERS):
            _run_and_check(vision, world, At(off), n, st, True, 0, 8, range(n), ("offset", off, st))
        for search in ("batch", "frame"):
            pipe = smh.Pipeline(vision, c.W, c.H, n, 4, search=search)
            try:
                for bad in (1, 2, 3):
                    with pytest.raises(smh.VisionError) as e:
                        pipe.submit(At(off).data_ptr() + bad, n, stages=stages, anchors=world["anchors"])
                    assert e.value.code == smh._lib.E_INVALID
                slot = pipe.submit(At(off).data_ptr(), n, stages=stages, max_gap=G.MAX_GAP, anchors=world["anchors"])
                assert slot == 0                                                # (the refused submissions took no slot)
                pipe.wait()
                recs = smh.results_to_dicts(pipe.slots[slot].read_results(0, n))
                for i in range(n):
                    _check_record(recs[i], world["refs"][i], world["infos"][i], stages, ("offset", off, search, i))
                    if world["refs"][i]["map_open"]:
                        _check_images(pipe.slots[slot], i, world["refs"][i], world["infos"][i], stages, True, ("offset", off, search, i))
            finally:
                pipe.close()
    fb = smh.FrameBatch(vision, c.W, c.H, n)
    try:
        for bad in (1, 2, 3):
            with pytest.raises(smh.VisionError) as e:
                fb.run(At(0).data_ptr() + bad, n, stages=stages, anchors=world["anchors"])
            assert e.value.code == smh._lib.E_INVALID
    finally:
        fb.close()


@pytest.mark.parametrize("W,H,why", G.REFUSED, ids=["%dx%d" % (W, H) for W, H, _ in G.REFUSED])
def test_sizes_beyond_the_limits_are_refused_at_creation(vision, o, W, H, why):
    """rw + m_xoff = 4097 (the library's own limit: the oracle takes the size) and rw = 7 (the reference's): SMHV_E_GEOMETRY from
    smhv_batch_create and smhv_pipeline_create_ex, so nothing is ever launched on such a size.  The sizes ON the limits are in the
    case table and run through every test above."""
    import squad_mortar_helper_amd as smh
    assert (o.map_bounds(W, H) is None) == ("rw = 7" in why)
    for make in (lambda: smh.FrameBatch(vision, W, H, 2), lambda: smh.Pipeline(vision, W, H, 2, 3, search="frame"), lambda: smh.Pipeline(vision, W, H, 2, 2, search="batch")):
        with pytest.raises(smh.VisionError) as e:
            make()
        assert e.value.code == smh._lib.E_GEOMETRY, (W, H, why)
    assert {(c.rw + c.m_xoff) for c in G.CASES} >= {4096} and {c.rw for c in G.CASES} >= {8}
