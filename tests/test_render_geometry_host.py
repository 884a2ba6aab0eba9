"""The inputs of the geometry tests without a GPU: the scenes' designed minimap rectangles against the oracle, and the restatements
(tests/render_ref.py, tests/overlay_ref.py, tests/firing_ref.py) on the new shapes against values derived by hand, so that the
reference is known right where tests/test_render_geometry_gpu.py leans on it."""
import ctypes as C

import numpy as np
import pytest

import firing_ref as FR
import minimap_scenes as S
import overlay_ref as O
import render_geometry_cases as G
import render_ref as RR

f32 = np.float32


@pytest.fixture(scope="module")
def scenes(built):
    return S.make_scenes()


def test_the_oracle_finds_the_designed_rectangle_of_every_scene(scenes):
    from oracle import oracle as o
    frames, anchors, rects, names = scenes
    _, _, rw, rh = S.roi()
    assert (rw, rh) == (360, 585) and len(frames) == S.N_SCENES <= 12
    proper = 0
    for i, name in enumerate(names[:-1]):
        assert o.find_minimap(frames[i]) == rects[i], (i, name)
        l, r, t, b = rects[i]
        assert l < rw // 2 < r and t < rh // 2 < b, (i, name)      # the rectangle holds the ROI's centre
        proper += (l, r, t, b) != (0, rw - 1, 0, rh - 1)
        res = o.process_frame(frames[i], True, 15, 0xF, anchors[i][1], anchors[i][0])
        assert res["map_open"] == 1 and res["n_lines"] >= 1, (i, name)   # the line search still returns lines
        assert (res["mpx"] is None) == (i == S.NO_ANCHORS), (i, name)
    assert proper == S.N_SCENES - 2                                 # all but the unstriped scene: a proper part of the ROI
    assert o.crop_to_map(frames[-1]) is None and rects[-1] is None  # the last frame is closed
    # the shapes the scenes are there for
    widths = [r[1] - r[0] for r in rects[:-1]]
    heights = [r[3] - r[2] for r in rects[:-1]]
    assert min(widths) < 20 and min(heights) < 20
    assert any(0 < rw // 2 - r[0] <= 4 for r in rects[:-1]) and any(0 < r[3] - rh // 2 <= 4 for r in rects[:-1])
    assert any(r[1] == rw - 1 and r[3] == rh - 1 and r[0] > 0 and r[2] > 0 for r in rects[:-1])


def _blend(c, u):
    """Step 5 of the overlay by hand: c * (64 / 255) + u * (1 - 64 / 255), + 0.5, truncated; every operation one f32 operation."""
    A = f32(64.0) / f32(255.0)
    B = f32(1.0) - A
    return int(np.uint8(min(f32(f32(f32(c) * A) + f32(f32(u) * B)) + f32(0.5), f32(255.0))))


def test_a_flat_map_is_green_and_a_1x1_map_blends_one_colour_over_the_rectangle():
    for data in (np.full((48, 64), 4242, np.uint16), np.array([[30000]], np.uint16), np.full((1, 9), 65535, np.uint16)):
        assert np.all(FR.color_map(data) == np.array([0, 255, 0, 255], np.uint8))
    U = np.empty((80, 80, 4), np.uint8)
    U[...] = (100, 100, 100, 255)
    quad, scale, tl = RR.identity(80, 80)
    cm = FR.color_map(np.array([[30000]], np.uint16))
    # 0 * A + 100 * B = 74.90 -> 75; 255 * A + 74.90 = 138.90 -> 139
    assert (_blend(0, 100), _blend(255, 100)) == (75, 139)
    for fit, x0, y0 in ((True, 10, 20), (False, 30, 40)):            # offset: 1 * (40 / (1 + 1)) = 20 on both axes
        out = RR.render(U, True, (10, 50, 20, 60), None, 80, 80, quad, scale, tl, RR.HEIGHTMAP | (0 if fit else RR.BOUNDS_OFFSET), cm, 1, 1)
        inside = np.zeros((80, 80), bool)
        inside[y0:60, x0:50] = True
        assert np.all(out[inside] == np.array([75, 139, 75, 255], np.uint8)) and np.all(out[~inside] == U[0, 0]), fit
        assert np.array_equal(out, O.overlay(U, (10, 50, 20, 60), cm, 1, 1, fit)), fit


def test_a_2048x3_map_taps_the_rows_computed_by_hand():
    # rows of one value each: 0 (blue), 32768 (green, just past the middle: 254), 65535 (red)
    data = np.empty((3, 2048), np.uint16)
    data[0], data[1], data[2] = 0, 32768, 65535
    cm = FR.color_map(data)
    rows = [(0, 0, 255), (0, 254, 0), (255, 0, 0)]
    for j in range(3):
        assert np.all(cm[j, :, :3] == np.array(rows[j], np.uint8)), j
    # the rectangle (0, 30, 10, 16): 6 pixel rows over 3 texel rows; t = ((cy - 10) / 6) * 3 - 0.5 for cy = 10.5 ... 15.5 is
    # -0.25, 0.25, 0.75, 1.25, 1.75, 2.25: rows (ja, jb) and weights fy
    hand = [(0, 0, 0.75), (0, 1, 0.25), (0, 1, 0.75), (1, 2, 0.25), (1, 2, 0.75), (2, 2, 0.25)]
    ja, jb, fy, gy = O.taps(np.arange(10, 16), f32(10), f32(6), 3)
    assert [(int(a), int(b), float(f)) for a, b, f in zip(ja, jb, fy)] == hand and np.array_equal(gy, f32(1.0) - fy)
    # 30 pixel columns over 2048 texel columns: column x taps floor((x + 0.5) / 30 * 2048 - 0.5) and the next
    ia, ib, _, _ = O.taps(np.arange(0, 30), f32(0), f32(30), 2048)
    assert [int(v) for v in ia[:3]] == [33, 101, 170] and int(ib[-1]) == 2014 and np.array_equal(ib, ia + 1)
    U = np.zeros((20, 30, 4), np.uint8)
    U[..., 3] = 255
    quad, scale, tl = RR.identity(30, 20)
    out = RR.render(U, True, (0, 30, 10, 16), None, 30, 20, quad, scale, tl, RR.HEIGHTMAP, cm)
    assert np.all(out[:10, :, :3] == 0) and np.all(out[16:, :, :3] == 0)
    for k, (a, b, fyk) in enumerate(hand):
        gyk = f32(1.0) - f32(fyk)
        c = [f32(f32(f32(rows[a][ch]) * gyk) + f32(f32(rows[b][ch]) * f32(fyk))) for ch in range(3)]   # the columns' two taps are equal
        want = [int(np.uint8(min(f32(f32(v * O.A) + f32(f32(0.0) * O.B)) + f32(0.5), f32(255.0)))) for v in c]
        assert np.all(out[10 + k, :, :3] == np.array(want, np.uint8)), (k, want, out[10 + k, 0].tolist())
    # the same map with width and height exchanged taps other rows: the restatement tells the two apart
    assert not np.array_equal(out, RR.render(U, True, (0, 30, 10, 16), None, 30, 20, quad, scale, tl, RR.HEIGHTMAP, FR.color_map(data.T.copy())))


def test_the_colour_tables_invariant_holds_over_every_value_of_every_range_in_use():
    """What k_hm_lut16 and rnd_tab_color rest on: no colour has both red and blue, and red is monotone in the value -- so one
    threshold value says which of the two the shared byte is."""
    used = set()
    for name, (data, _, _) in G.heightmaps().items():
        used.add((int(data.min()), int(data.max())))
    assert len(used) >= 10 and {(1000, 1001), (1000, 1003), (0, 2999), (60000, 65535), (4242, 4242)} <= used
    for lo, hi in sorted(used | set(G.VALUE_RANGES)):
        v = np.arange(lo, hi + 1, dtype=np.int64).astype(np.uint16).reshape(1, -1)
        cm = FR.color_map(v)[0].astype(np.int64)
        r, g, b = cm[:, 0], cm[:, 1], cm[:, 2]
        assert not np.any((r > 0) & (b > 0)), (lo, hi)
        assert np.all(np.diff(r) >= 0) and np.all(np.diff(b) <= 0), (lo, hi)
        red = np.nonzero(r)[0]
        vr = int(red[0]) if len(red) else len(r)                  # the first value with red (none: past the end)
        assert np.all(b[vr:] == 0) and np.all(r[:vr] == 0), (lo, hi)
        if lo == hi:
            assert (int(r[0]), int(g[0]), int(b[0])) == (0, 255, 0)
        else:
            assert (int(r[-1]), int(b[0])) == (255, 255) and (int(r[0]), int(b[-1])) == (0, 0), (lo, hi)


def test_the_line_families_paint_what_the_comparison_needs():
    _, _, rw, rh = S.roi()
    ow, oh = G.WINDOW
    U = np.zeros((rh, rw, 4), np.uint8)
    U[..., 3] = 255
    for name, view in G.line_views(rw, rh).items():
        lines, fam = G.line_list(view)
        assert lines.shape == (256, 4) and len(fam) == len(G.border_family()) == 120
        masks = G.check_line_family(lines, fam, view, ow, oh)
        assert not any(masks[i].any() for i in G.ZERO_LENGTH)
        want = RR.render(U, True, None, lines, ow, oh, view.quad, view.scale, view.top_left, RR.MARKERS)
        G.check_pairs(want, masks, 256)
        big = float(np.max(np.abs(lines)))
        assert (big > 1.5e4) == (name == "zoom 10, far pan"), (name, big)
    # lines with an end point that is not finite: what the restatement paints of each (identity viewport)
    view = G.line_views(rw, rh)["identity"]
    for ln, count in G.NON_FINITE:
        assert int(RR.line_mask(ow, oh, np.array(ln, np.float32), view.scale, view.top_left).sum()) == count, ln


def test_the_thin_view_overflows_the_staged_forms_lds_in_some_bands_only(built):
    """The 1024 x 640 map through the "thin" view: the launch gets the most LDS there is (12,288 texels).  The generic scene's
    rectangle is 11 px wide: the 8 px of it in tile 0 tap ~760 texel columns, and a band with two or more covered rows spans at
    least 15 texel rows -- it gathers; the 3 px in tile 1 tap ~280 columns, and every band fits."""
    from squad_mortar_helper_amd import _lib
    _, _, rw, rh = S.roi()
    view = G.matrix_views(rw, rh)["thin"]
    ow, oh = G.WINDOW
    tx, fm = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.load().smhv_debug_render_rule(rw, rh, float(view.scale[0]), float(view.scale[1]), 1024, 640, None, None, C.byref(tx), C.byref(fm)))
    assert tx.value == 12288 and fm.value == _lib.RENDER_FORM_TABLE
    x0, y0, r, b = RR.hm_rect((42, 321, 58, 532), 1024, 640, 0, 0, True, view.scale, view.top_left)
    sx, sy = f32(r - x0), f32(b - y0)
    staged, gathered = G.staged_bands(ow, oh, (x0, y0, f32(x0 + sx), f32(y0 + sy), sx, sy), 1024, 640, tx.value)
    assert staged >= 8 and gathered >= 8, (staged, gathered)
