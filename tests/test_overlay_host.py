"""The heightmap overlay without a GPU: the public ABI of the new stage, image id and entry points, and the restatement
(tests/overlay_ref.py) against cases computed by hand from the header's f32 steps."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import overlay_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smh_vision_hip.h")
f32 = np.float32


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_stage_the_image_and_both_entry_points():
    h = _header()
    assert re.search(r"#define\s+SMHV_STAGE_HEIGHTMAP_OVERLAY\s+0x100u\b", h)
    assert re.search(r"#define\s+SMHV_IMAGE_HEIGHTMAP_OVERLAY\s+101\b", h)
    assert re.search(r"SMHV_API\s+int\s+smhv_heightmap_overlay\s*\(\s*smhv_ctx\s*\*\s*\w*\s*,\s*const\s+smhv_heightmap\s*\*\s*\w*\s*,"
                     r"\s*const\s+smhv_firing_options\s*\*\s*\w*\s*,\s*uint8_t\s*\*\s*\w*\s*\)\s*;", h)
    assert re.search(r"SMHV_API\s+int\s+smhv_batch_overlay_ptr\s*\(\s*smhv_batch\s*\*\s*\w*\s*,\s*void\s*\*\*\s*\w*\s*\)\s*;", h)


def test_stage_values_and_struct_sizes_against_a_c_program(built, tmp_path):
    from squad_mortar_helper_amd import _lib
    src = str(tmp_path / "overlay_abi.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "smh_vision_hip.h"\nint main(void) {\n'
                ' printf("%u %u %d\\n", SMHV_STAGE_HEIGHTMAP_OVERLAY, SMHV_STAGE_ALL & SMHV_STAGE_HEIGHTMAP_OVERLAY, SMHV_IMAGE_HEIGHTMAP_OVERLAY);\n'
                ' printf("%zu %zu\\n", sizeof(smhv_frame_result), sizeof(smhv_batch_layout));\n'
                ' return 0; }\n')
    exe = src[:-2]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]
    assert rows[0] == [0x100, 0, 101]
    # the record and the layout do not grow: the overlay slab has the ui slab's layout
    assert rows[1] == [1216, 168] == [C.sizeof(_lib.FrameResult), C.sizeof(_lib.BatchLayout)]


def test_binding_exposes_the_stage(built):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    assert _lib.STAGE_HEIGHTMAP_OVERLAY == smh.STAGE_HEIGHTMAP_OVERLAY == 0x100
    assert not (smh.STAGE_ALL & smh.STAGE_HEIGHTMAP_OVERLAY)
    assert _lib.IMAGE_HEIGHTMAP_OVERLAY == 101
    for name in ("smhv_heightmap_overlay", "smhv_batch_overlay_ptr"):
        assert name in _lib.SIGNATURES
    assert callable(smh.FrameBatch.read_overlay) and callable(smh.FrameBatch.overlay_ptr) and callable(smh.HipVision.heightmap_overlay)


def _ui(h, w, seed=3):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    u[..., 3] = 255
    return u


def _blend(c, u):
    """Step 5 by hand for one channel: c, u as f32."""
    o = f32(c) * (f32(64.0) / f32(255.0)) + f32(u) * (f32(1.0) - f32(64.0) / f32(255.0))
    return int(np.uint8(min(o + f32(0.5), f32(255.0))))


def test_coverage_is_half_open_at_pixel_centres():
    # [2.5, 6.5): the centre 2.5 is in, the centre 6.5 is out
    assert list(O.covered(10, f32(2.5), f32(6.5))) == [2, 3, 4, 5]
    assert list(O.covered(10, f32(2.4), f32(6.6))) == [2, 3, 4, 5, 6]
    assert list(O.covered(10, f32(2.6), f32(6.5))) == [3, 4, 5]
    # the left edge on a pixel centre through the offset: W = 3, b00 = 1, right - left = 2 -> off.x = 1 * (2 / 4) = 0.5
    U = _ui(8, 12)
    Cm = np.full((3, 3, 4), 255, np.uint8)
    out = O.overlay(U, (4, 6, 1, 5), Cm, 1, 0, fit_to_minimap=False)
    x0, y0, x1, y1, _, _ = O.quad((4, 6, 1, 5), 3, 3, 1, 0, False)
    assert (x0, y0, x1, y1) == (f32(4.5), f32(1.0), f32(6.0), f32(5.0))
    changed = np.argwhere(np.any(out != U, axis=2))
    assert set(map(tuple, changed)) <= {(y, x) for y in range(1, 5) for x in (4, 5)}
    assert np.all(out[1:5, 4:6, 3] == 255) and np.array_equal(out[:, :4], U[:, :4]) and np.array_equal(out[:, 6:], U[:, 6:])
    assert np.array_equal(out[0], U[0]) and np.array_equal(out[5:], U[5:])


def test_a_pixel_on_a_texel_centre_reproduces_the_texel():
    # one texel per pixel (W = H = 4 over a 4 x 4 quad at (2, 3)): pixel (x, y) samples texel (x - 2, y - 3) with fx = fy = 0
    rng = np.random.default_rng(8)
    Cm = rng.integers(0, 256, size=(4, 4, 4), dtype=np.uint8)
    Cm[..., 3] = 255
    U = _ui(10, 10)
    U[3:7, 2:6, :3] = Cm[..., :3]                                  # u == c: the blend gives the texel back
    out = O.overlay(U, (2, 6, 3, 7), Cm)
    assert np.array_equal(out[3:7, 2:6, :3], Cm[..., :3]) and np.all(out[3:7, 2:6, 3] == 255)
    # and with another ui_map, every channel is the blend of the texel alone
    U2 = _ui(10, 10, seed=9)
    out2 = O.overlay(U2, (2, 6, 3, 7), Cm)
    for y, x, k in [(3, 2, 0), (4, 3, 1), (6, 5, 2), (5, 2, 1)]:
        assert out2[y, x, k] == _blend(Cm[y - 3, x - 2, k], U2[y, x, k]), (y, x, k)


def test_a_pixel_midway_between_two_texels_gives_their_exact_mix():
    # W = 2 x the quad's width: pixel x samples s = 2 x + 0.5 (fx = 0.5) between texels 2x and 2x+1; rows are uniform in y
    Cm = np.zeros((8, 8, 4), np.uint8)
    Cm[..., 3] = 255
    Cm[:, :, 0] = np.array([10, 31, 200, 7, 0, 255, 128, 129], np.uint8)[None, :]
    Cm[:, :, 1] = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.uint8)[None, :]
    U = _ui(6, 6)
    out = O.overlay(U, (0, 4, 0, 4), Cm)
    for y in range(4):
        for x in range(4):
            for k in (0, 1):
                a, b = f32(Cm[0, 2 * x, k]), f32(Cm[0, 2 * x + 1, k])
                top = a * f32(0.5) + b * f32(0.5)                    # fy: t = 2 y + 0.5 as well, both rows equal
                c = top * f32(0.5) + top * f32(0.5)
                assert out[y, x, k] == _blend(c, U[y, x, k]), (y, x, k)


def test_a_uniform_map_gives_the_blend_of_its_colour():
    Cm = np.empty((37, 53, 4), np.uint8)
    Cm[...] = (200, 100, 30, 255)
    U = np.empty((40, 50, 4), np.uint8)
    U[...] = (10, 250, 128, 255)
    out = O.overlay(U, (3, 45, 2, 33), Cm)
    want = [_blend(200, 10), _blend(100, 250), _blend(30, 128), 255]
    assert want == [58, 212, 103, 255]                               # (uint8)(c*A + u*B + 0.5), by hand: 58.19, 212.85, 103.90
    assert np.all(out[2:33, 3:45] == np.array(want, np.uint8))
    assert np.array_equal(out[:2], U[:2]) and np.array_equal(out[33:], U[33:]) and np.array_equal(out[:, :3], U[:, :3]) and np.array_equal(out[:, 45:], U[:, 45:])


def test_the_offset_mode_moves_the_top_left_by_the_formula():
    mm, W, H, b00, b01 = (100, 700, 50, 650), 1000, 700, 37, -21
    fit = O.quad(mm, W, H, b00, b01, True)
    off = O.quad(mm, W, H, b00, b01, False)
    ox = f32(37) * (f32(600) / (f32(1000) + f32(37)))
    oy = f32(-21) * (f32(600) / (f32(700) + f32(-21)))
    assert fit[:4] == (f32(100), f32(50), f32(700), f32(650))
    assert off[0] == f32(100) + ox and off[1] == f32(50) + oy
    assert off[4] == f32(700) - off[0] and off[2] == off[0] + off[4] and off[5] == f32(650) - off[1]
    assert 21.0 < float(ox) < 21.5 and -18.6 < float(oy) < -18.5
    # the covered columns start where the shifted edge does
    rng = np.random.default_rng(2)
    Cm = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    Cm[..., 3] = 255
    U = _ui(700, 760)
    out = O.overlay(U, mm, Cm, b00, b01, fit_to_minimap=False)
    cols = np.nonzero(np.any(out != U, axis=(0, 2)))[0]
    rows = np.nonzero(np.any(out != U, axis=(1, 2)))[0]
    assert cols.min() >= 121 and cols.max() == 699 and rows.min() >= 31 and rows.max() == 649


def test_a_rectangle_outside_the_ui_map_or_none_changes_nothing():
    U = _ui(20, 20)
    Cm = np.full((5, 5, 4), 77, np.uint8)
    assert np.array_equal(O.overlay(U, (500, 600, 500, 600), Cm), U)
    assert np.array_equal(O.overlay(U, (2, 18, 25, 40), Cm), U)
    assert np.array_equal(O.overlay(U, None, Cm), U)
    # degenerate quads: zero width, right < left (u32 wraps)
    assert np.array_equal(O.overlay(U, (5, 5, 2, 10), Cm), U)
    assert np.array_equal(O.overlay(U, (9, 4, 2, 10), Cm), U)


def test_w_plus_b00_zero_covers_nothing():
    U = _ui(20, 20)
    Cm = np.full((4, 6, 4), 90, np.uint8)
    assert np.array_equal(O.overlay(U, (2, 15, 3, 17), Cm, -6, 0, fit_to_minimap=False), U)   # W + b00 == 0
    assert np.array_equal(O.overlay(U, (2, 15, 3, 17), Cm, 0, -4, fit_to_minimap=False), U)   # H + b01 == 0
    assert np.array_equal(O.overlay(U, (2, 2, 3, 17), Cm, -6, 0, fit_to_minimap=False), U)    # 0 / 0
    assert not np.array_equal(O.overlay(U, (2, 15, 3, 17), Cm, -6, 0, fit_to_minimap=True), U)
