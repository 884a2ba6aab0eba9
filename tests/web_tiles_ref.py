"""The feed's map tiles (include/smh_vision_hip.h, "remote-viewer feed: map tiles"), restated with struct.pack, zlib.crc32 and
numpy on top of tests/web_ref.py: the tile grid, the MapTiles message, the choice between MapTiles and Map, the base of every frame
and the kept map across calls -- what smhv_batch_feed_tiles / smhv_feed_frame_tiles are compared with, byte for byte.  Pure Python;
needs neither the library nor a device."""
import struct
import zlib

import numpy as np

import web_ref as W

MAP_TILES = 6
TW, TH = 64, 16


def pad16(n):
    return (n + 15) & ~15


def grid(w, h):
    """(tiles_x, tiles_y)"""
    return -(-w // TW), -(-h // TH)


def tile_rect(w, h, t):
    """Tile t = ty * tiles_x + tx -> (x0, y0, cw, ch), clipped at the map's right and bottom edge."""
    tiles_x, _ = grid(w, h)
    ty, tx = divmod(t, tiles_x)
    return TW * tx, TH * ty, min(TW, w - TW * tx), min(TH, h - TH * ty)


def tile_bytes(w, h, t):
    _, _, cw, ch = tile_rect(w, h, t)
    return pad16(4 * cw * ch)


def tiles_len(w, h, tiles):
    """L = 26 + pad16(4 n) + the sum of the tiles' padded bytes."""
    return 26 + pad16(4 * len(tiles)) + sum(tile_bytes(w, h, t) for t in tiles)


def map_len(w, h):
    return 10 + 4 * w * h


def _image(w, h, rgba):
    return np.frombuffer(bytes(rgba), np.uint8).reshape(h, w, 4)


def changed_tiles(w, h, base, new, alpha=True):
    """The tiles any byte of which differs between the two maps, ascending (alpha=False: a mutant's rule)."""
    d = _image(w, h, base) != _image(w, h, new)
    d = d.any(axis=2) if alpha else d[..., :3].any(axis=2)
    tiles_x, tiles_y = grid(w, h)
    return [t for t in range(tiles_x * tiles_y) if (lambda x0, y0, cw, ch: d[y0:y0 + ch, x0:x0 + cw].any())(*tile_rect(w, h, t))]


def map_tiles(w, h, base, new, alpha=True, padded=True):
    """The MapTiles message that turns the map `base` into the map `new` (both w * h * 4 bytes of RGBA)."""
    base, new = bytes(base), bytes(new)
    tiles = changed_tiles(w, h, base, new, alpha)
    img = _image(w, h, new)
    out = struct.pack("<HIIHHIII", MAP_TILES, w, h, TW, TH, len(tiles), zlib.crc32(base) & 0xFFFFFFFF, zlib.crc32(new) & 0xFFFFFFFF)
    lst = struct.pack("<%dI" % len(tiles), *tiles)
    out += lst + (b"\x00" * (pad16(len(lst)) - len(lst)) if padded else b"")
    for t in tiles:
        x0, y0, cw, ch = tile_rect(w, h, t)
        px = img[y0:y0 + ch, x0:x0 + cw].tobytes()
        out += px + (b"\x00" * (pad16(len(px)) - len(px)) if padded else b"")
    assert not padded or not alpha or len(out) == tiles_len(w, h, tiles)
    return out


def kept_usable(kept, stored, w, h):
    """kept = (w, h, rgba) or None: usable iff there is a stored CRC, it is the kept map's, and the kept map has this call's size."""
    return kept is not None and stored is not None and stored == (zlib.crc32(bytes(kept[2])) & 0xFFFFFFFF) and (kept[0], kept[1]) == (w, h)


def feed_tiles(frames, stored=None, kept=None, capacity=None, first=0, rule=None):
    """web_ref.feed with map tiles.  frames as web_ref.frame_events takes them; stored: the feed's stored CRC or None; kept: the
    feed's kept map (w, h, rgba) or None.  rule: None, or the one rule a mutant changes (tests/web_tiles_cases.py).
    -> dict(messages, entries, frames_done, n_maps, stored, bytes_used, kept): web_ref.feed's result and the kept map afterwards."""
    off, used, done, n_maps = 6, 0, 0, 0
    messages, entries = [], []
    base = None                                                # the map of the nearest earlier open OK frame of this call
    first_open = True
    last_open = None                                           # (a mutant's: the batch's last open frame, consumed or not)
    for fr in frames:
        if fr[0] and fr[1] == W.FRAME_OK:
            last_open = fr[2]
    for i, fr in enumerate(frames):
        ev, crc, after = W.frame_events(fr, stored)
        if not ev and rule == "base_is_previous_frame" and not first_open:
            base = None                                        # the mutant: a closed frame in between loses the base
        if ev:
            w, h, rgba = fr[2]
            if first_open:
                usable = kept_usable(kept, stored, w, h) if rule != "kept_trusted_after_foreign_map" else (kept is not None and stored is not None and (kept[0], kept[1]) == (w, h))
                base = kept[2] if usable else None
            if len(ev) == 3 and base is not None:              # a Map would go out: tiles instead when they are shorter
                msg = map_tiles(w, h, base, rgba, alpha=rule != "alpha_ignored", padded=rule != "unpadded_tiles")
                if (len(msg) <= map_len(w, h)) if rule == "le_for_lt" else (len(msg) < map_len(w, h)):
                    ev = [ev[0], (MAP_TILES, msg), ev[2]]
            o, placed = off, []
            for kind, data in ev:
                placed.append((o, kind, data))
                o += W.slot(len(data))
            end = placed[-1][0] + len(placed[-1][2])
            if capacity is not None and end > capacity:
                break
            for po, kind, data in placed:
                messages.append((first + i, kind, crc, data))
                entries.append((first + i, kind, len(data), crc, po))
                n_maps += kind == W.MAP
            off, used = o, end
            base, first_open = rgba, False
            kept = (w, h, bytes(rgba))
        stored = after
        done = i + 1
    if rule == "kept_from_batch_end" and last_open is not None and kept is not None:
        kept = (last_open[0], last_open[1], bytes(last_open[2]))
    return dict(messages=messages, entries=entries, frames_done=done, n_maps=n_maps, stored=stored, bytes_used=used, kept=kept)


def apply_message(texture, data):
    """The viewer's texture (w, h, bytearray) or None after one Map or MapTiles message, by the rule alone (the library's client
    half, squad_mortar_helper_amd.web.MapTexture, is held against this)."""
    (kind,) = struct.unpack_from("<H", data, 0)
    if kind == W.MAP:
        w, h = struct.unpack_from("<II", data, 2)
        return (w, h, bytearray(data[10:]))
    assert kind == MAP_TILES
    _, w, h, tw, th, n, base_crc, crc = struct.unpack_from("<HIIHHIII", data, 0)
    assert (tw, th) == (TW, TH) and texture is not None and (texture[0], texture[1]) == (w, h) and zlib.crc32(bytes(texture[2])) == base_crc
    img = np.frombuffer(bytes(texture[2]), np.uint8).reshape(h, w, 4).copy()
    at = 26 + pad16(4 * n)
    for t in struct.unpack_from("<%dI" % n, data, 26):
        x0, y0, cw, ch = tile_rect(w, h, t)
        img[y0:y0 + ch, x0:x0 + cw] = np.frombuffer(data, np.uint8, 4 * cw * ch, at).reshape(ch, cw, 4)
        at += pad16(4 * cw * ch)
    assert at == len(data) and zlib.crc32(img.tobytes()) == crc
    return (w, h, bytearray(img.tobytes()))
