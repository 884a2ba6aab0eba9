"""The remote-viewer feed's protocol on the host (no GPU): the restatement (tests/web_ref.py) against messages written out by hand,
the library's host-only encoders and the interaction parser against the restatement, the feed's structs against the header, and
the sequence rule on a hand-made sequence."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np

import web_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _h(s):
    return bytes.fromhex(s.replace(" ", ""))


def test_restatement_against_hand_written_messages():
    # UpdateState: 03 00, f64, flag (+ left, right, top, bottom as u32)
    assert W.update_state(1.5, (1, 2, 3, 0x01020304)) == _h("0300 000000000000f83f 01 01000000 02000000 03000000 04030201")
    assert W.update_state(0.25, None) == _h("0300 000000000000d03f 00")
    assert W.update_state(None, None) == _h("0300 0000000000000000 00")
    assert W.update_state(None, (7, 8, 9, 10)) == _h("0300 0000000000000000 01 07000000 08000000 09000000 0a000000")
    assert len(W.update_state(1.0, (0, 0, 0, 0))) == 27 and len(W.update_state(1.0, None)) == 11
    # Markers: 02 00, custom, n as u32, n x (p0.x, p0.y, p1.x, p1.y) as f32
    assert W.markers(np.zeros((0, 4), np.float32)) == _h("0200 00 00000000")
    assert W.markers([[1.0, 2.0, -3.0, 0.5]]) == _h("0200 00 01000000 0000803f 00000040 000040c0 0000003f")
    assert W.markers([[1.0, 2.0, -3.0, 0.5]], custom=True)[:3] == _h("0200 01")
    many = np.arange(128, dtype=np.float32).reshape(32, 4)
    m = W.markers(many)
    assert len(m) == 7 + 16 * 32 and m[:7] == _h("0200 00 20000000") and m[7:11] == _h("00000000") and m[-4:] == struct.pack("<f", 127.0)
    assert m[7 + 16 * 5 + 8:7 + 16 * 5 + 12] == struct.pack("<f", 22.0)          # marker 5's p1.x
    # Map: 01 00, w, h, then the RGBA bytes
    assert W.map_event(2, 1, bytes([1, 2, 3, 255, 4, 5, 6, 255])) == _h("0100 02000000 01000000 010203ff 040506ff")
    # Heightmap: 04 00 01 00 (flag, pad), w, h, bounds[0][0], bounds[0][1] as i32, scale[2], texels; None: 04 00 00
    hm = W.heightmap(np.array([[1, 2, 3], [0xFFFE, 5, 6]], np.uint16), ((-2, 3), (9, 9)), (7.0, 8.0, 0.5))
    assert hm == _h("0400 01 00 03000000 02000000 feffffff 03000000 0000003f 0100 0200 0300 feff 0500 0600")
    assert hm[3] == 0 and len(hm) == 24 + 12 and (len(hm) - 12) % 2 == 0         # the pad byte at offset 3; the texels start at 24, an even offset
    assert W.heightmap(None) == _h("0400 00")
    assert W.fit(True) == _h("0500 01") and W.fit(False) == _h("0500 00")
    # the ids are the macro's numbering
    assert (W.MAP, W.MARKERS, W.UPDATE_STATE, W.HEIGHTMAP, W.FIT_TO_MINIMAP) == (1, 2, 3, 4, 5)


def test_host_encoders_equal_the_restatement_on_random_inputs(built):
    import squad_mortar_helper_amd as smh
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 31, 32, 33, 200):
        lines = rng.uniform(-5000.0, 5000.0, size=(n, 4)).astype(np.float32)
        if n > 1:
            lines.view(np.uint32)[1, 2] = 0x7FC01234                              # a NaN payload travels bit for bit
            lines[0, 0] = -0.0
        for custom in (False, True):
            assert smh.encode_markers(lines, custom) == W.markers(lines, custom), (n, custom)
    for (w, h) in ((1, 1), (3, 2), (17, 5), (64, 64), (129, 3)):
        data = rng.integers(0, 65536, size=(h, w), dtype=np.uint16)
        bounds = ((int(rng.integers(-2**31, 2**31)), int(rng.integers(-2**31, 2**31))), (int(rng.integers(-100, 100)), 5))
        scale = tuple(float(np.float32(v)) for v in rng.uniform(-100.0, 100.0, 3))
        assert smh.encode_heightmap(data, bounds, scale) == W.heightmap(data, bounds, scale), (w, h)
    assert smh.encode_heightmap(None) == W.heightmap(None)
    for flag in (False, True):
        assert smh.encode_fit(flag) == W.fit(flag)
    # a buffer that is too small is refused and says what is needed
    lib, need = smh._lib.load(), C.c_uint64()
    buf = np.zeros(64, np.uint8)
    lines = np.ones((4, 4), np.float32)
    assert lib.smhv_web_event_markers(lines.ctypes.data, 4, 0, buf.ctypes.data, 70, C.byref(need)) == smh._lib.E_INVALID and need.value == 71
    assert lib.smhv_web_event_fit(1, buf.ctypes.data, 2, C.byref(need)) == smh._lib.E_INVALID and need.value == 3 and not buf.any()


def test_parse_interaction(built):
    import squad_mortar_helper_amd as smh
    rng = np.random.default_rng(12)
    f = rng.uniform(-1e4, 1e4, 4).astype(np.float32)
    f.view(np.uint32)[1] = 0x7FA00001                                             # a signalling NaN's bits pass through
    f.view(np.uint32)[3] = 0xFFC00000
    add = struct.pack("<H", 1) + f.tobytes()
    kind, line = smh.parse_interaction(add)
    assert kind == "add" and line.tobytes() == f.tobytes() and W.parse_interaction(add) == ("add", f.tobytes())
    dele = struct.pack("<HI", 2, 0xFEDCBA98)
    assert smh.parse_interaction(dele) == ("delete", 0xFEDCBA98) == W.parse_interaction(dele)
    # every wrong length from 0 to 20 (the whole message: 2 bytes of kind and the rest), both kinds
    for kind_id, good in ((1, 18), (2, 6)):
        for n in range(0, 21):
            msg = (struct.pack("<H", kind_id) + bytes(range(40)))[:n]
            got, want = smh.parse_interaction(msg), W.parse_interaction(msg)
            assert (got is None) == (want is None) == (n != good), (kind_id, n)
    for kind_id in (0, 3, 0x0101, 0xFFFF):                                        # unknown kinds, at the lengths the known ones take
        for n in (2, 6, 18):
            msg = (struct.pack("<H", kind_id) + bytes(16))[:n]
            assert smh.parse_interaction(msg) is None and W.parse_interaction(msg) is None


def test_feed_structs_match_the_header(built, tmp_path):
    import re
    from squad_mortar_helper_amd import _lib
    E, H = _lib.FeedEntry, _lib.FeedHeader
    assert C.sizeof(E) == 24 and [(n, getattr(E, n).offset) for n, _ in E._fields_] == [("offset", 0), ("length", 8), ("frame", 12), ("kind", 16), ("crc", 20)]
    assert C.sizeof(H) == 32 and [(n, getattr(H, n).offset) for n, _ in H._fields_] == \
        [("n_entries", 0), ("frames_done", 4), ("n_maps", 8), ("has_last_crc", 12), ("last_crc", 16), ("reserved", 20), ("bytes_used", 24)]
    hdr = open(os.path.join(ROOT, "include", "smh_vision_hip.h")).read()
    defs = dict(re.findall(r"#define (SMHV_(?:WEB|FEED)_\w+) (\d+)u", hdr))
    assert [int(defs[k]) for k in ("SMHV_WEB_MAP", "SMHV_WEB_MARKERS", "SMHV_WEB_UPDATE_STATE", "SMHV_WEB_HEIGHTMAP", "SMHV_WEB_FIT_TO_MINIMAP", "SMHV_FEED_SNAPSHOT")] == \
        [_lib.WEB_MAP, _lib.WEB_MARKERS, _lib.WEB_UPDATE_STATE, _lib.WEB_HEIGHTMAP, _lib.WEB_FIT_TO_MINIMAP, _lib.FEED_SNAPSHOT] == [W.MAP, W.MARKERS, W.UPDATE_STATE, W.HEIGHTMAP, W.FIT_TO_MINIMAP, 1]
    # a C program compiled against the header agrees on sizes and offsets
    src = str(tmp_path / "smhv_feed_layout.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                "sizeof(smhv_feed_entry), offsetof(smhv_feed_entry, length), offsetof(smhv_feed_entry, frame), offsetof(smhv_feed_entry, kind), offsetof(smhv_feed_entry, crc), "
                "sizeof(smhv_feed_header), offsetof(smhv_feed_header, frames_done), offsetof(smhv_feed_header, has_last_crc), offsetof(smhv_feed_header, last_crc), "
                "offsetof(smhv_feed_header, bytes_used)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", src[:-2]])
    assert subprocess.check_output([src[:-2]]).decode().split() == ["24", "8", "12", "16", "20", "32", "4", "12", "16", "24"]


def _frame(px, lines=(), mpx=None, minimap=None, map_open=True, status=0, w=2, h=2):
    ui = (w, h, bytes([px]) * (w * h * 4))
    return (map_open, status, ui, np.asarray(lines, np.float32).reshape(-1, 4), mpx is not None, mpx if mpx is not None else 0.0, minimap is not None,
            minimap if minimap is not None else (0, 0, 0, 0))


def test_sequence_rule_on_a_hand_made_sequence():
    A, B = 10, 20
    crc = {p: zlib.crc32(bytes([p]) * 16) for p in (A, B)}
    line = [[1.0, 2.0, 3.0, 4.0]]
    seq = [_frame(A, line, mpx=0.5), _frame(A), _frame(A, map_open=False), _frame(A, minimap=(1, 2, 3, 4)), _frame(B), _frame(B, status=1), _frame(A, line)]
    r = W.feed(seq)
    kinds = [(f, k) for f, k, _, _ in r["messages"]]
    U, M, K = W.UPDATE_STATE, W.MAP, W.MARKERS
    # frame 0 sends its map (no texture yet); 1 and 3 do not (equal, also across the closed frame 2); 4 does (B); 5 is dropped on
    # its status and leaves the stored CRC alone; 6 sends A again (the texture is B's)
    assert kinds == [(0, U), (0, M), (0, K), (1, U), (1, K), (3, U), (3, K), (4, U), (4, M), (4, K), (6, U), (6, M), (6, K)]
    assert r["frames_done"] == 7 and r["n_maps"] == 3 and r["stored"] == crc[A]
    assert [c for f, k, c, _ in r["messages"] if k == M] == [crc[A], crc[B], crc[A]]
    by = {(f, k): d for f, k, _, d in r["messages"]}
    assert by[(0, U)] == W.update_state(0.5, None) and by[(3, U)] == W.update_state(None, (1, 2, 3, 4)) and by[(1, U)] == W.update_state(None, None)
    assert by[(0, K)] == W.markers(line) and by[(1, K)] == W.markers([]) and by[(4, M)] == W.map_event(2, 2, bytes([B]) * 16)
    # offsets: the first message at 6, every one at 6 (mod 16), none overlapping, bytes_used the end of the last
    offs = [(o, n) for _, _, n, _, o in r["entries"]]
    assert offs[0][0] == 6 and all(o % 16 == 6 for o, _ in offs) and all(offs[i][0] + offs[i][1] <= offs[i + 1][0] for i in range(len(offs) - 1))
    assert r["bytes_used"] == offs[-1][0] + offs[-1][1]
    # a stored CRC from an earlier call: frame 0 sends no map when it equals A's, and does when it is B's
    assert [k for f, k, _, _ in W.feed(seq[:1], stored=crc[A])["messages"]] == [U, K]
    assert [k for f, k, _, _ in W.feed(seq[:1], stored=crc[B])["messages"]] == [U, M, K]
    assert W.feed([seq[2], seq[5]], stored=crc[B]) == dict(messages=[], entries=[], frames_done=2, n_maps=0, stored=crc[B], bytes_used=0)
    # a capacity cut: whole frames only; the stored CRC reflects the consumed frames; continuing yields the same messages
    cap = r["entries"][7][4] - 1                                                   # frame 4's first message would end beyond it ... but frame 3 fits
    cut = W.feed(seq, capacity=cap)
    assert cut["frames_done"] == 4 and cut["messages"] == r["messages"][:7] and cut["stored"] == crc[A] and cut["bytes_used"] <= cap
    rest = W.feed(seq[4:], stored=cut["stored"], first=4)
    assert cut["messages"] + rest["messages"] == r["messages"] and rest["stored"] == r["stored"]
    exact = W.feed(seq, capacity=r["entries"][9][4] + r["entries"][9][2])          # frame 4's Markers ends exactly at the capacity: it fits
    assert exact["frames_done"] == 6 and exact["stored"] == crc[B]                 # (frame 5 has nothing to write: consumed too)
    assert W.feed(seq, capacity=r["entries"][9][4] + r["entries"][9][2] - 1)["frames_done"] == 4
    # the snapshot of ws.rs:35-55: Map always, UpdateState / Markers only when they carry something; the stored CRC untouched
    snap = W.feed(seq, stored=crc[A], snapshot=True)
    assert [(f, k) for f, k, _, _ in snap["messages"]] == [(0, M), (0, U), (0, K), (1, M), (3, M), (3, U), (4, M), (6, M), (6, K)] and snap["stored"] == crc[A]
    assert W.worst_case(2, 2) == 6 + 32 + 32 + 519
