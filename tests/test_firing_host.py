"""Firing solutions without a GPU: the ABI of the new structs against the header, the SMHHM file format, and the restatement
(tests/firing_ref.py) against the reference's anchor values."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import firing_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_firing_structs_match_a_c_program_compiled_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib
    src = str(tmp_path / "firing_layout.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\nint main(void) {\n'
                ' printf("%zu %zu %zu\\n", sizeof(smhv_firing), sizeof(smhv_firing_result), sizeof(smhv_firing_options));\n'
                ' printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(smhv_firing, meters), offsetof(smhv_firing, alt_delta), offsetof(smhv_firing, mils),'
                ' offsetof(smhv_firing, bearing), offsetof(smhv_firing, source), offsetof(smhv_firing, reserved));\n'
                ' printf("%zu %zu\\n", offsetof(smhv_firing_result, n_lines), offsetof(smhv_firing_result, line));\n'
                ' printf("%zu %zu %zu %zu\\n", offsetof(smhv_firing_options, size), offsetof(smhv_firing_options, flags),'
                ' offsetof(smhv_firing_options, viewport_scale), offsetof(smhv_firing_options, viewport_top_left));\n'
                ' printf("%u %u %u %u %u\\n", SMHV_STAGE_FIRING, SMHV_FIRING_BOUNDS_OFFSET, SMHV_FIRING_NONE, SMHV_FIRING_SCALES, SMHV_FIRING_HEIGHTMAP);\n'
                ' return 0; }\n')
    exe = src[:-2]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]
    assert rows[0] == [48, 1544, 24] == [C.sizeof(_lib.Firing), C.sizeof(_lib.FiringResult), C.sizeof(_lib.FiringOptions)]
    F = _lib.Firing
    assert rows[1] == [F.meters.offset, F.alt_delta.offset, F.mils.offset, F.bearing.offset, F.source.offset, F.reserved.offset]
    assert rows[2] == [_lib.FiringResult.n_lines.offset, _lib.FiringResult.line.offset]
    O = _lib.FiringOptions
    assert rows[3] == [O.size.offset, O.flags.offset, O.viewport_scale.offset, O.viewport_top_left.offset]
    assert rows[4] == [_lib.STAGE_FIRING, _lib.FIRING_BOUNDS_OFFSET, _lib.FIRING_NONE, _lib.FIRING_SCALES, _lib.FIRING_HEIGHTMAP] == [0x80, 1, 0, 1, 2]
    dt = _lib.firing_dtype()
    assert dt.itemsize == 48 and [dt.fields[k][1] for k in ("meters", "alt_delta", "mils", "bearing", "source")] == rows[1][:5]
    # STAGE_FIRING is not part of STAGE_ALL, and the binding exports it
    import squad_mortar_helper_amd as smh
    assert smh.STAGE_FIRING == 0x80 and smh.STAGE_ALL & smh.STAGE_FIRING == 0
    hdr = open(os.path.join(ROOT, "include", "smh_vision_hip.h")).read()
    assert re.search(r"#define SMHV_STAGE_ALL 0xFu", hdr)


def test_smhhm_round_trip_and_rejected_headers(built, tmp_path):
    from squad_mortar_helper_amd import heightmap as H
    rng = np.random.default_rng(3)
    data = rng.integers(0, 65536, size=(37, 53), dtype=np.uint16)
    bounds, scale = ((-1200, 340), (51000, 49000)), (100.0, 100.0, 12.5)
    p = str(tmp_path / "map.smhhm")
    H.write_smhhm(p, data, bounds, scale)
    raw = open(p, "rb").read()
    assert raw[:4] == bytes.fromhex("0BADFEEF") and raw[4:6] == b"\0\0" and raw[6:10] == bytes.fromhex("0BADFEEF")
    assert raw[10:18] == (53).to_bytes(4, "little") + (37).to_bytes(4, "little") and raw[46:52] == b"\xfd7zXZ\0"
    d2, b2, s2 = H.read_smhhm(p)
    assert np.array_equal(d2, data) and b2 == bounds and s2 == scale
    bad_magic = bytearray(raw); bad_magic[0] ^= 1
    bad_ver = bytearray(raw); bad_ver[4] = 1
    bad_magic2 = bytearray(raw); bad_magic2[9] ^= 0x10
    for i, b in enumerate((bad_magic, bad_ver, bad_magic2)):
        q = str(tmp_path / ("bad%d.smhhm" % i))
        open(q, "wb").write(bytes(b))
        assert H.read_smhhm(q) is None


def test_mils_anchor_values():
    assert R.calc(1000, 0) == 1117.8198030882309
    assert R.calc(1232, 0) == 810.1925178125936
    assert math.isnan(R.calc(1233, 0))
    assert R.calc(800, 25.5) == 1234.874808451302
    # V^2 and V^4 are pow's values (what the Rust build folds), and the device header embeds exactly those
    src = open(os.path.join(ROOT, "squad-mortar-helper_amd", "csrc", "smh_firing.h")).read()
    assert "#define SMH_MORTAR_V2 %s" % R.V2.hex() in src and "#define SMH_MORTAR_V4 %s" % R.V4.hex() in src


def test_bearings_of_the_eight_compass_directions():
    # screen y grows downwards: p1 straight above p0 is north
    want = {(0, -1): 0, (1, -1): 45, (1, 0): 90, (1, 1): 135, (0, 1): 180, (-1, 1): 225, (-1, 0): 270, (-1, -1): 315}
    for (dx, dy), fwd in want.items():
        b = R.firing_line((10.0, 10.0, 10.0 + 7 * dx, 10.0 + 7 * dy))["bearing"]
        assert (float(b[0]), float(b[1])) == (fwd, (fwd + 180) % 360), (dx, dy, b)


def test_roundf_is_half_away_from_zero_and_fmod_wraps():
    f = np.float32
    assert [float(R.roundf(f(v))) for v in (0.5, 1.5, 2.5, -0.5, -2.5)] == [1.0, 2.0, 3.0, -1.0, -3.0]
    assert float(R.roundf(f(0.49999997))) == 0.0 and float(np.floor(f(0.49999997) + f(0.5))) == 1.0
    # 359.6 degrees rounds to 360 and wraps to 0; its opposite is 180
    fwd, bck = R.bearings_from_degrees(f(359.6) + f(90.0))
    assert (float(fwd), float(bck)) == (0.0, 180.0)


def test_restated_heightmap_branch_by_hand():
    data = np.zeros((100, 200), np.uint16)
    data[10, 20] = 65535
    hm = (data, ((0, 0), (0, 0)), (1.0, 1.0, 0.1953125))     # height(v) = v / 65535 m
    # minimap {left 0, right 400, top 0, bottom 200}: 2 map px per heightmap texel
    r = R.firing_line((40.0, 20.0, 0.0, 0.0), minimap=(0, 400, 0, 200), hm=hm)
    assert r["source"] == R.HEIGHTMAP and r["meters"] == math.hypot(20.0, 10.0) and r["alt_delta"] == -1.0
    assert r["mils"] == (R.calc(r["meters"], -1.0), R.calc(r["meters"], 1.0))
    # an end point outside: the record's meters, or nothing
    assert R.firing_line((400.0, 20.0, 0.0, 0.0), minimap=(0, 400, 0, 200), meters=5.0, hm=hm)["source"] == R.SCALES
    assert R.firing_line((400.0, 20.0, 0.0, 0.0), minimap=(0, 400, 0, 200), hm=hm)["source"] == R.NONE


def test_product_package_does_not_import_the_restatement(built):
    pkg = os.path.join(ROOT, "squad-mortar-helper_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "firing_ref" not in src, f


def test_color_map_restatement_quirks():
    const = np.full((3, 4), 777, np.uint16)
    assert (R.color_map(const).reshape(-1, 4) == [0, 255, 0, 255]).all()     # NaN drops out of f64::max
    ramp = np.array([[0, 65535, 32767, 32768]], np.uint16)
    cm = R.color_map(ramp)[0]
    assert cm[0].tolist() == [0, 0, 255, 255] and cm[1].tolist() == [255, 0, 0, 255] and cm[2, 3] == 255 and cm[3, 3] == 255
