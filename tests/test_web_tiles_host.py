"""CPU half of the map-tile tests of the remote-viewer feed (tests/web_tiles_cases.py): the sizes' self-checks, the literal bytes of
one hand-typed MapTiles message, every case's own assertion on the restatement (tests/web_tiles_ref.py), the mutant check, the
library's client half (MapTexture, decode_map_tiles) replaying every case's stream to the exact map of every open frame, what the
entry points refuse before a device is asked, and csrc/smh_maptiles.h compiled into a stand-alone program
(tests/map_tiles_check.cpp, with -fsanitize=address,undefined where the host compiler links it) whose numbers equal the
restatement's.  No device."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import web_ref as W
import web_tiles_cases as TC
import web_tiles_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "squad-mortar-helper_amd", "csrc")


def test_sizes_and_tables_hold_what_they_are_there_for(built):
    TC.check_sizes()
    assert len(TC.CASE_NAMES) == len(set(TC.CASE_NAMES)) and set(TC.MUTANTS.values()) <= set(TC.CASE_NAMES) and len(TC.MUTANTS) >= 6
    assert {n.split("/")[0] for n in TC.CASE_NAMES} == set(TC.SIZE_NAMES) | {"seq", "cont", "long"}
    assert TC.FRAME_CASES == ["cont/batch then frame"]
    tx, ty = T.grid(TC.MAIN.rw, TC.MAIN.rh)
    assert (tx, ty) == (2, 17) and T.tile_rect(TC.MAIN.rw, TC.MAIN.rh, tx * ty - 1) == (64, 256, 37, 15)
    assert TC.corner_tiles(TC.MAIN) == [2, 3, 32, 33] and TC.corner_tiles(TC.SIZES["8x274"]) == [1, 17]
    assert [TC.k_star(c) for c in (TC.SIZES["8x274"], TC.MAIN)] == [17, 34]                # (worked out by hand: 26 + 144 + 16 x 4096 + 3840 + 16 x 2368 + 2224 = 109658 > 109494 only with all 34)


def test_one_message_typed_out_by_hand(built):
    """A 65 x 17 map of zeros whose last pixel becomes (1, 2, 3, 4): tile 3 of the 2 x 2 grid, one pixel wide and high."""
    import squad_mortar_helper_amd as smh
    base = bytearray(65 * 17 * 4)
    new = bytearray(base)
    new[-4:] = bytes([1, 2, 3, 4])
    want = bytes.fromhex("0600" "41000000" "11000000" "4000" "1000" "01000000" "d19177cd" "00b50f5a"
                         "03000000" "000000000000000000000000"
                         "01020304" "000000000000000000000000")
    assert T.map_tiles(65, 17, base, new) == want and len(want) == 58 == T.tiles_len(65, 17, [3])
    assert (zlib.crc32(bytes(base)), zlib.crc32(bytes(new))) == (0xCD7791D1, 0x5A0FB500)
    w, h, base_crc, crc, tiles = smh.decode_map_tiles(want)
    assert (w, h, base_crc, crc) == (65, 17, 0xCD7791D1, 0x5A0FB500) and [(t, a.tolist()) for t, a in tiles] == [(3, [[[1, 2, 3, 4]]])]
    assert smh.WEB_MAP_TILES == T.MAP_TILES == 6
    for bad in (want[:-1], want + b"\x00", b"\x01" + want[1:], want[:10] + b"\x20" + want[11:]):
        with pytest.raises(ValueError):
            smh.decode_map_tiles(bad)


@pytest.mark.parametrize("gray", [False, True], ids=["colour", "grey"])
@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_every_case_is_there_for_what_it_says_and_replays(built, name, gray):
    """The case's own assertion and the restatement's client; then MapTexture over the same stream: after every open frame's
    messages the texture is that frame's map, byte for byte."""
    import squad_mortar_helper_amd as smh
    case = TC.BY_NAME[name]
    fr = TC.ref_frames(case, gray)
    res = TC.run_reference(case, fr)
    case.check(res, fr)
    TC.replay(case, res, fr)
    tex = smh.MapTexture()
    for st, r in zip(case.steps, res):
        for f, kind, crc, data in (r["messages"] if r else []):
            if kind in (W.MAP, T.MAP_TILES):
                tex.apply(data)
            if kind == W.MARKERS:
                want = fr[st[1]][st[2] if st[0] == "frame" else f][2][2]
                assert tex.map.tobytes() == want and tex.crc() == crc == zlib.crc32(want), (name, st, f)


def test_map_texture_refuses_tiles_against_another_map(built):
    import squad_mortar_helper_amd as smh
    case = TC.BY_NAME["seq/X Y X"]
    fr = TC.ref_frames(case, False)
    (r,) = TC.run_reference(case, fr)
    maps = [d for _, k, _, d in r["messages"] if k == W.MAP]
    tiles = [d for _, k, _, d in r["messages"] if k == T.MAP_TILES]
    tex = smh.MapTexture()
    assert tex.crc() is None
    with pytest.raises(ValueError):
        tex.apply(tiles[0])                                     # no texture yet
    tex.apply(maps[0])
    with pytest.raises(ValueError):
        tex.apply(tiles[1])                                     # made against the map AFTER tiles[0]
    before = tex.map.copy()
    tex.apply(tiles[0])
    tex.apply(tiles[1])
    assert np.array_equal(tex.map, before) and tex.crc() == zlib.crc32(fr[0][0][2][2])


@pytest.mark.parametrize("rule", sorted(TC.MUTANTS))
def test_every_mutant_is_told_apart(built, rule):
    assert TC.mutant_is_told_apart(rule, False) and TC.mutant_is_told_apart(rule, True), rule


def test_mutants_change_one_rule_only(built):
    """On a plain X P1 X every mutant is feed_tiles."""
    case = TC.BY_NAME["seq/X Y X"]
    fr = TC.ref_frames(case, True)
    want = TC.run_reference(case, fr)
    for rule in TC.MUTANTS:
        if rule != "unpadded_tiles":                            # (one full tile: only the index list's padding is missing)
            assert TC.run_reference(case, fr, rule) == want, rule


def test_null_handles_are_refused_before_a_device_is_asked(built):
    from squad_mortar_helper_amd import _lib as L
    lib = L.load()
    assert lib.smhv_batch_feed_tiles(None, None, 0, 1, 0, None) == L.E_INVALID
    assert lib.smhv_feed_frame_tiles(None, None, None, 0, None, None, 0) == L.E_INVALID


def test_the_header_as_a_stand_alone_program(built, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "map_tiles_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "map_tiles_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    jobs = []
    for c in list(TC.SIZES.values()) + [(65, 17), (64, 16), (1, 1), (4096, 274)]:
        w, h = (c.rw, c.rh) if hasattr(c, "rw") else c
        n = T.grid(w, h)[0] * T.grid(w, h)[1]
        for tiles in ([], [n - 1], list(range(0, n, 3)), list(range(n)), list(range(min(TC.k_star(TC.MAIN), n)))):
            jobs.append((w, h, tiles))
    jobs.append((TC.EQUAL.rw, TC.EQUAL.rh, TC.equal_tiles(TC.EQUAL)))
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(jobs)) + b"".join(struct.pack("<3I%dI" % len(t), w, h, len(t), *t) for w, h, t in jobs))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok: %d jobs" % len(jobs)), (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    got, at = (tmp_path / "out.bin").read_bytes(), 0
    for w, h, tiles in jobs:
        tx, ty = T.grid(w, h)
        assert struct.unpack_from("<2I", got, at) == (tx, ty), (w, h)
        at += 8
        for t in range(tx * ty):
            _, _, cw, ch = T.tile_rect(w, h, t)
            assert struct.unpack_from("<3I", got, at) == (cw, ch, T.tile_bytes(w, h, t)), (w, h, t)
            at += 12
        L_, m, chosen = struct.unpack_from("<QQI", got, at)
        at += 20
        assert (L_, m, chosen) == (T.tiles_len(w, h, tiles), T.map_len(w, h), int(T.tiles_len(w, h, tiles) < T.map_len(w, h))), (w, h, len(tiles))
    assert at == len(got)
    w, h, tiles = jobs[-1]
    assert T.tiles_len(w, h, tiles) == T.map_len(w, h)          # (the one job where `<` and `<=` part)
