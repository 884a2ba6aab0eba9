"""The map view's layers without a GPU: the restatement (tests/render_layers_ref.py) against pixel sets derived by hand from the
header's rules, the paint order, the three Python builders against values written out by hand, and the public ABI of the two
calls through a compiled C program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import render_geometry_cases as G
import render_layers_cases as LC
import render_layers_ref as LR
import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smh_vision_hip.h")
f32 = np.float32
ID = (RR.identity(20, 12)[1], RR.identity(20, 12)[2])
RED, BLUE = (200, 10, 20, 255), (5, 6, 250, 255)


def _set(mask):
    return set(map(tuple, np.argwhere(mask)))


def _rect(x0, y0, x1, y1, kind=LR.RECT, rgba=RED):
    return (x0, y0, x1, y1, rgba, kind)


def test_a_rectangle_is_the_outer_box_without_the_inner_one():
    m = LR.prim_mask(20, 12, _rect(2, 1, 7, 5), *ID)
    outer = {(y, x) for y in range(1, 5) for x in range(2, 7)}
    inner = {(y, x) for y in (2, 3) for x in (3, 4, 5)}
    assert _set(m) == outer - inner and m.sum() == 14
    # inverted corners paint the same
    for c in ((7, 5, 2, 1), (7, 1, 2, 5), (2, 5, 7, 1)):
        assert np.array_equal(LR.prim_mask(20, 12, _rect(*c), *ID), m), c
    # narrower than 2: filled -- the columns with centres 2.5 and 3.5, no inner column (3.25 <= cx < 2.75 holds for none)
    m = LR.prim_mask(20, 12, _rect(2.25, 1, 3.75, 5), *ID)
    assert _set(m) == {(y, x) for y in range(1, 5) for x in (2, 3)}
    # flatter than 2 likewise; 1 px wide is one column
    assert _set(LR.prim_mask(20, 12, _rect(2, 3, 7, 4.5), *ID)) == {(y, x) for y in (3,) for x in range(2, 7)}
    assert _set(LR.prim_mask(20, 12, _rect(4, 1, 5, 5), *ID)) == {(y, 4) for y in range(1, 5)}
    # exactly 2 wide: both columns are the frame (3 <= cx < 3 holds for none)
    assert _set(LR.prim_mask(20, 12, _rect(2, 1, 4, 5), *ID)) == {(y, x) for y in range(1, 5) for x in (2, 3)}
    # 3 wide: centre 3.5 is inside in the rows 2 and 3
    assert _set(LR.prim_mask(20, 12, _rect(2, 1, 5, 5), *ID)) == {(y, x) for y in range(1, 5) for x in (2, 3, 4)} - {(2, 3), (3, 3)}
    # a NaN corner yields the other one: a = b in x, nothing is painted; all NaN and a degenerate one paint nothing either
    nan = float("nan")
    assert not LR.prim_mask(20, 12, _rect(nan, 1, 7, 5), *ID).any()
    assert not LR.prim_mask(20, 12, _rect(nan, nan, nan, nan), *ID).any()
    assert not LR.prim_mask(20, 12, _rect(3, 3, 3, 9), *ID).any()
    # an infinite corner: the frame's left column and its top and bottom rows run to the window's edge
    m = LR.prim_mask(20, 12, _rect(10, 2, float("inf"), 6), *ID)
    assert _set(m) == {(y, 10) for y in range(2, 6)} | {(y, x) for y in (2, 5) for x in range(10, 20)}
    # half-open at a pixel centre: an edge at 2.5 takes the centre 2.5 in on the left and out on the right
    assert _set(LR.prim_mask(20, 12, _rect(2.5, 1, 3.5, 2), *ID)) == {(1, 2)}


def test_shift1_moves_the_frame_by_one_and_applies_after_the_viewport():
    m = LR.prim_mask(20, 12, _rect(2, 1, 7, 5, LR.RECT | LR.SHIFT1), *ID)
    assert np.array_equal(m[1:, 1:], LR.prim_mask(20, 12, _rect(2, 1, 7, 5), *ID)[:-1, :-1]) and not m[0].any() and not m[:, 0].any()
    # scale 2, top left (1, 0): corners (5, 2), (15, 10), then + 1 -- not (2 + 1) * 2
    e = LR.ends((2, 1, 7, 5), (f32(2), f32(2)), (f32(1), f32(0)), True)
    assert e == (f32(6), f32(3), f32(16), f32(11))
    m = LR.prim_mask(20, 12, _rect(2, 1, 7, 5, LR.RECT | LR.SHIFT1), (f32(2), f32(2)), (f32(1), f32(0)))
    assert _set(m) == {(y, x) for y in range(3, 11) for x in range(6, 16)} - {(y, x) for y in range(4, 10) for x in range(7, 15)}
    # a line is shifted too: rows 10 and 11 instead of 9 and 10
    m = LR.prim_mask(20, 20, (3, 10, 8, 10, RED, LR.LINE | LR.SHIFT1), *ID)
    assert _set(m) == {(y, x) for y in (10, 11) for x in range(4, 9)}
    # the minimap bounds: (left, top), (right, bottom) of a record's (left, right, top, bottom), shifted, green
    p = LR.bounds_prim((3, 9, 2, 7))
    assert p[:4] == (3, 2, 9, 7) and p[4] == (0, 255, 0, 255) and p[5] == LR.RECT | LR.FOREGROUND | LR.SHIFT1
    assert _set(LR.prim_mask(20, 12, p, *ID)) == {(y, x) for y in range(3, 8) for x in range(4, 10)} - {(y, x) for y in range(4, 7) for x in range(5, 9)}


def test_paint_order_below_prims_detected_lines_foreground_prims_bounds():
    U = np.zeros((20, 20, 4), np.uint8)
    U[..., 3] = 255
    quad, scale, tl = RR.identity(20, 20)
    below = (5, 4, 5, 16, BLUE, LR.LINE)                            # vertical: columns 4 and 5
    lines = [(3, 10, 17, 10)]                                       # the detected one: rows 9 and 10
    fg = (4, 8, 7, 12, RED, LR.RECT | LR.FOREGROUND)                # its frame holds (9, 4) ... and crosses both
    green = RR.line_color(0, 1)
    out = LR.render(U, True, (12, 16, 8, 12), lines, 20, 20, quad, scale, tl, RR.MARKERS, [fg, below], True)
    assert list(green) == [0, 255, 0, 255]
    assert tuple(out[9, 4]) == RED and tuple(out[10, 4]) == RED      # all three cross: the foreground prim's
    assert tuple(out[9, 5]) == tuple(green)                          # (9, 5) is inside the frame: below-prim and line cross, the line's
    assert tuple(out[5, 4]) == BLUE and tuple(out[9, 10]) == tuple(green) and tuple(out[8, 6]) == RED
    # the bounds lie above everything: its left column (x = 13) crosses the detected line in the rows 9 and 10
    assert tuple(out[9, 13]) == LR.BOUNDS_COLOR and tuple(out[10, 13]) == LR.BOUNDS_COLOR and tuple(out[10, 14]) == tuple(green) and tuple(out[12, 15]) == LR.BOUNDS_COLOR
    # the detected line keeps the colour it has without prims; prims in list order inside their class
    assert np.array_equal(LR.render(U, True, None, lines, 20, 20, quad, scale, tl, RR.MARKERS), RR.render(U, True, None, lines, 20, 20, quad, scale, tl, RR.MARKERS))
    two = [(2, 2, 9, 9, RED, LR.RECT), (2, 2, 9, 9, BLUE, LR.RECT)]
    assert tuple(LR.render(U, True, None, None, 20, 20, quad, scale, tl, 0, two)[2, 2]) == BLUE
    assert tuple(LR.render(U, True, None, None, 20, 20, quad, scale, tl, 0, two[::-1])[2, 2]) == RED
    # nothing to draw is render_ref's image; a closed frame is background; no rectangle, no bounds
    assert np.array_equal(LR.render(U, True, (1, 5, 1, 5), lines, 20, 20, quad, scale, tl, RR.MARKERS), RR.render(U, True, (1, 5, 1, 5), lines, 20, 20, quad, scale, tl, RR.MARKERS))
    assert np.all(LR.render(U, False, (1, 5, 1, 5), lines, 20, 20, quad, scale, tl, RR.MARKERS, [fg, below], True, background=(9, 8, 7, 255)) == np.array((9, 8, 7, 255), np.uint8))
    assert np.array_equal(LR.render(U, True, None, None, 20, 20, quad, scale, tl, 0, (), True), U)
    # a debug view enters as `ui`: at the identity viewport of its own size the image is the view
    V = np.random.default_rng(1).integers(0, 256, size=(7, 9, 4), dtype=np.uint8)
    V[..., 3] = 255
    assert np.array_equal(LR.render(V, True, None, None, 9, 7, *RR.identity(9, 7)), V)


def test_the_prim_list_of_the_gpu_tests_does_what_it_is_for():
    for name, view in LC.views(986, 822).items():
        prims = LC.prim_list(view)
        assert len(prims) == 256 and sum(1 for p in prims if p[5] & LR.FOREGROUND) == 256 - LC.N_BELOW
        assert {p[5] & 0xFF for p in prims} == {LR.LINE, LR.RECT} and any(p[5] & LR.SHIFT1 for p in prims)
        masks = LC.check_prim_list(prims, view)
        U = np.zeros((822, 986, 4), np.uint8)
        U[..., 3] = 255
        base = LR.render(U, True, None, None, *LC.WINDOW, view.quad, view.scale, view.top_left, 0, (), False, background=G.BG)
        want = LR.render(U, True, None, None, *LC.WINDOW, view.quad, view.scale, view.top_left, 0, prims, False, background=G.BG)
        assert LC.changed(want, base) >= LC.PRIMS_MIN[name] > 0, (name, LC.changed(want, base))
        # the crossing of a pair is the second prim's, the first the next wave compacts
        for (i, j), (cx, cy) in zip(G.PAIRS, G.PAIR_CENTRES):
            assert not any(m[cy, cx] for m in masks[j + 1:]) and tuple(want[cy, cx]) == prims[j][4], (name, i, j)


def test_builders_restate_the_callers_side(built):
    import squad_mortar_helper_amd as smh
    M, R_ = (255, 0, 255, 255), (255, 0, 0, 255)
    # custom markers in magenta, below; drag and measure only from the threshold on (draw.rs:34-36: sum((a - b)^2) >= t^2)
    got = smh.ctl_marker_prims([((1.5, 2.0), (30.0, 40.25))], drag=((0.0, 0.0), (6.0, 0.0)), measure=((10.0, 10.0), (13.0, 15.25)), drag_threshold=6.0)
    assert got == [(1.5, 2.0, 30.0, 40.25, M, 0), (0.0, 0.0, 6.0, 0.0, M, 0), (10.0, 10.0, 13.0, 15.25, R_, 0)]      # 36 >= 36; 9 + 27.5625 >= 36
    got = smh.ctl_marker_prims([], drag=((0.0, 0.0), (5.99, 0.0)), measure=((10.0, 10.0), (13.0, 15.0)), drag_threshold=6.0)
    assert got == []                                                # 35.88 and 34 < 36
    assert smh.ctl_marker_prims([((1, 2), (3, 4))]) == [(1.0, 2.0, 3.0, 4.0, M, 0)]
    assert smh.ctl_marker_prims([], drag=((0, 0), (3, 4)), drag_threshold=5.0) == [(0.0, 0.0, 3.0, 4.0, M, 0)]
    # OCR boxes: offset by the quadrant's size, foreground rectangles, [1 - c/100, c/100, 0] as (uint8)(clamp01(v) * 255 + 0.5)
    K = smh.PRIM_RECT | smh.PRIM_FOREGROUND
    got = smh.ocr_box_prims([(3, 4, 50, 20, 0.0), (3, 4, 50, 20, 50.0), (3, 4, 50, 20, 100.0), (0, 0, 1, 1, 137.0), (3, 4, 50, 20, 25.0)], 493, 411)
    assert got[0] == (496.0, 415.0, 543.0, 431.0, (255, 0, 0, 255), K)
    assert got[1] == (496.0, 415.0, 543.0, 431.0, (128, 128, 0, 255), K)          # 0.5 * 255 + 0.5 = 128.0
    assert got[2] == (496.0, 415.0, 543.0, 431.0, (0, 255, 0, 255), K)
    assert got[3] == (493.0, 411.0, 494.0, 412.0, (0, 255, 0, 255), K)            # 1.37 clamps to 1, -0.37 to 0
    assert got[4][4] == (191, 64, 0, 255)                                         # 191.75 and 64.25, truncated
    # scale bars: (left, y, right, found) -> a magenta foreground line at y, bars that were not found skipped
    got = smh.scale_bar_prims([(10, 30, 90, 1), (0, 0, 0, 0), (12, 44, 200, 1)], 493, 411)
    assert got == [(503.0, 441.0, 583.0, 441.0, M, smh.PRIM_LINE | smh.PRIM_FOREGROUND), (505.0, 455.0, 693.0, 455.0, M, smh.PRIM_LINE | smh.PRIM_FOREGROUND)]
    # RenderLayers lays the prims out as the C struct wants them
    ly, arr = smh.RenderLayers(got, minimap_bounds=True, map_source=smh._lib.VIEW_LSD_INPUT).struct()
    assert (ly.size, ly.flags, ly.map_source, ly.n_prims) == (C.sizeof(smh._lib.RenderLayersStruct), 1, 4, 2)
    assert (ly.prims[1].x0, ly.prims[1].y1, tuple(ly.prims[1].rgba), ly.prims[1].kind) == (505.0, 455.0, M, 0x100)
    ly, _ = smh.RenderLayers().struct()
    assert (ly.flags, ly.map_source, ly.n_prims) == (0, 0, 0) and not ly.prims


def test_struct_sizes_offsets_and_constants_against_a_c_program(built, tmp_path):
    from squad_mortar_helper_amd import _lib
    src = str(tmp_path / "layers_abi.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\nint main(void) {\n'
                ' printf("%u %u %u %u %u %u\\n", SMHV_PRIM_LINE, SMHV_PRIM_RECT, SMHV_PRIM_FOREGROUND, SMHV_PRIM_SHIFT1, SMHV_RENDER_MAX_PRIMS, SMHV_LAYER_MINIMAP_BOUNDS);\n'
                ' printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(smhv_render_prim), offsetof(smhv_render_prim, x0), offsetof(smhv_render_prim, y0),\n'
                '        offsetof(smhv_render_prim, x1), offsetof(smhv_render_prim, y1), offsetof(smhv_render_prim, rgba), offsetof(smhv_render_prim, kind));\n'
                ' printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(smhv_render_layers), offsetof(smhv_render_layers, size), offsetof(smhv_render_layers, flags),\n'
                '        offsetof(smhv_render_layers, map_source), offsetof(smhv_render_layers, n_prims), offsetof(smhv_render_layers, prims));\n'
                ' printf("%zu %zu\\n", sizeof(smhv_render_options), sizeof(smhv_frame_result));\n'
                ' return 0; }\n')
    exe = src[:-2]
    # the header stays plain C
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror=implicit-function-declaration", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]
    assert rows[0] == [0, 1, 0x100, 0x200, 256, 1] == [_lib.PRIM_LINE, _lib.PRIM_RECT, _lib.PRIM_FOREGROUND, _lib.PRIM_SHIFT1, _lib.RENDER_MAX_PRIMS, _lib.LAYER_MINIMAP_BOUNDS]
    P, Y = _lib.RenderPrim, _lib.RenderLayersStruct
    assert rows[1] == [24, 0, 4, 8, 12, 16, 20] == [C.sizeof(P), P.x0.offset, P.y0.offset, P.x1.offset, P.y1.offset, P.rgba.offset, P.kind.offset]
    assert rows[2] == [24, 0, 4, 8, 12, 16] == [C.sizeof(Y), Y.size.offset, Y.flags.offset, Y.map_source.offset, Y.n_prims.offset, Y.prims.offset]
    assert rows[3] == [52, 1216]                                    # smhv_render_options and the record stay what they were


def test_header_and_binding_declare_the_two_calls(built):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    with open(HEADER) as f:
        h = f.read()
    assert re.search(r"SMHV_API\s+int\s+smhv_batch_render_layers\s*\(\s*smhv_batch\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+smhv_heightmap\s*\*\s*\w+\s*,"
                     r"\s*const\s+smhv_render_options\s*\*\s*\w+\s*,\s*const\s+smhv_render_layers\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"SMHV_API\s+int\s+smhv_render_map_layers\s*\(\s*smhv_ctx\s*\*\s*\w+\s*,\s*const\s+smhv_heightmap\s*\*\s*\w+\s*,\s*const\s+smhv_render_options\s*\*\s*\w+\s*,"
                     r"\s*const\s+smhv_render_layers\s*\*\s*\w+\s*,\s*const\s+smhv_line\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;", h)
    # the header pins the rules, and the map view's sentence stays true
    assert "fminf(P0.x, P1.x)" in h and "a.x + 1.0f <= cx && cx < b.x - 1.0f" in h and "Text labels are not drawn" in h and "The reference's text is not drawn" in h
    for name in ("smhv_batch_render_layers", "smhv_render_map_layers"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    for fn in (smh.RenderLayers, smh.ctl_marker_prims, smh.ocr_box_prims, smh.scale_bar_prims, smh.prim):
        assert callable(fn)
    import inspect
    assert "layers" in inspect.signature(smh.FrameBatch.render).parameters and "layers" in inspect.signature(smh.HipVision.render_map).parameters
