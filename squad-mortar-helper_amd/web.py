"""The remote-viewer feed (smhv_feed_* / smhv_batch_feed / smhv_feed_frame): the reference web server's events of every processed
frame (web/src/lib.rs:127-214), written on the device, and the host-only rest of its protocol.  FrameBatch.feed and
HipVision.feed_frame take map_source = a VIEW_* of _lib: that debug view is hashed and sent as the Map in the ui_map's place
(smhv_batch_feed_view / smhv_feed_frame_view; src/ui/map.rs:210).  Transport is the caller's: a
message from WebFeed.read() or an encoder is what the reference hands its websocket as one binary frame."""
import ctypes as C
import struct
import zlib

import numpy as np

from . import _lib as L


class WebFeed:
    """A feed: a message buffer of `capacity_bytes` on the device, room for `max_frames` frames per call, and the CRC-32 of the
    map the viewers hold.  FrameBatch.feed / HipVision.feed_frame fill it; read() hands the messages out."""

    def __init__(self, vision, capacity_bytes, max_frames):
        self._lib = L.load()
        self._vision = vision            # keeps the context alive
        f = C.c_void_p()
        L.check(self._lib.smhv_feed_create(vision._ctx, int(capacity_bytes), int(max_frames), C.byref(f)))
        self._f = f
        self.capacity_bytes, self.max_frames = int(capacity_bytes), int(max_frames)

    def close(self):
        if self._f:
            self._lib.smhv_feed_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Forget the CRC of the map last sent: the next open frame sends its map."""
        L.check(self._lib.smhv_feed_reset(self._f))

    def header(self):
        """Synchronising copy of the header alone -> FeedHeader."""
        h = L.FeedHeader()
        L.check(self._lib.smhv_feed_read(self._f, C.byref(h), None, 0, None, 0))
        return h

    def read(self):
        """Waits for the feed's last call -> (FeedHeader, [(frame, kind, crc, bytes)]) in the order the messages are to be
        sent; only the header, the entries and bytes_used bytes cross to the host."""
        h = self.header()
        entries = (L.FeedEntry * max(int(h.n_entries), 1))()
        raw = np.empty(max(int(h.bytes_used), 1), np.uint8)
        L.check(self._lib.smhv_feed_read(self._f, C.byref(h), entries, len(entries), raw.ctypes.data, raw.size))
        self.entries = entries[:h.n_entries]
        return h, [(int(e.frame), int(e.kind), int(e.crc), raw[e.offset:e.offset + e.length].tobytes()) for e in self.entries]

    def ptrs(self):
        """Device addresses (header, entries, bytes) for a consumer on the device."""
        p = [C.c_void_p() for _ in range(3)]
        L.check(self._lib.smhv_feed_ptrs(self._f, *[C.byref(x) for x in p]))
        return tuple(x.value or 0 for x in p)


TILE_W, TILE_H = 64, 16                      # the MapTiles grid (include/smh_vision_hip.h, "remote-viewer feed: map tiles")


def _pad16(n):
    return (n + 15) & ~15


def decode_map_tiles(message):
    """A MapTiles message (FrameBatch.feed_tiles / HipVision.feed_frame_tiles) -> (w, h, base_crc, crc, [(index, tile uint8
    [ch, cw, 4])]): the tiles of the map that differ from the map whose CRC-32 is base_crc, clipped at the map's right and bottom
    edge; applied to that map they give the map whose CRC-32 is crc.  ValueError for anything that is not a whole, well-formed
    MapTiles message."""
    m = bytes(message)
    if len(m) < 26:
        raise ValueError("MapTiles: %d bytes" % len(m))
    kind, w, h, tw, th, n, base_crc, crc = struct.unpack_from("<HIIHHIII", m, 0)
    if kind != L.WEB_MAP_TILES or (tw, th) != (TILE_W, TILE_H):
        raise ValueError("MapTiles: id %d, tiles of %d x %d" % (kind, tw, th))
    tiles_x, tiles_y = -(-w // TILE_W), -(-h // TILE_H)
    at = 26 + _pad16(4 * n)
    if len(m) < at:
        raise ValueError("MapTiles: %d bytes, %d indices" % (len(m), n))
    idx = struct.unpack_from("<%dI" % n, m, 26)
    if any(b <= a for a, b in zip(idx, idx[1:])) or (n and idx[-1] >= tiles_x * tiles_y):
        raise ValueError("MapTiles: the indices are not strictly ascending tiles of a %d x %d map" % (w, h))
    out = []
    for t in idx:
        ty, tx = divmod(t, tiles_x)
        cw, ch = min(TILE_W, w - TILE_W * tx), min(TILE_H, h - TILE_H * ty)
        nb = 4 * cw * ch
        if len(m) < at + _pad16(nb):
            raise ValueError("MapTiles: the message ends inside tile %d" % t)
        out.append((t, np.frombuffer(m, np.uint8, nb, at).reshape(ch, cw, 4)))
        at += _pad16(nb)
    if at != len(m):
        raise ValueError("MapTiles: %d bytes behind the last tile" % (len(m) - at))
    return w, h, base_crc, crc, out


class MapTexture:
    """The client half of the tile feed: the map a viewer holds.  apply(message) takes a Map or a MapTiles message as
    WebFeed.read() hands them out; a MapTiles whose base_crc is not the texture's CRC-32 is refused (ValueError) and changes
    nothing.  map: uint8 [h, w, 4] or None."""

    def __init__(self):
        self.map = None

    def crc(self):
        """CRC-32 of the texture's bytes, or None before the first Map."""
        return None if self.map is None else zlib.crc32(self.map.tobytes()) & 0xFFFFFFFF

    def apply(self, message):
        m = bytes(message)
        (kind,) = struct.unpack_from("<H", m, 0)
        if kind == L.WEB_MAP:
            w, h = struct.unpack_from("<II", m, 2)
            if len(m) != 10 + 4 * w * h:
                raise ValueError("Map: %d bytes for %d x %d" % (len(m), w, h))
            self.map = np.frombuffer(m, np.uint8, 4 * w * h, 10).reshape(h, w, 4).copy()
            return
        w, h, base_crc, crc, tiles = decode_map_tiles(m)
        if self.map is None or self.map.shape != (h, w, 4) or self.crc() != base_crc:
            raise ValueError("MapTiles against a map with CRC %08x: the texture's is %s" % (base_crc, "none" if self.map is None else "%08x" % self.crc()))
        tiles_x = -(-w // TILE_W)
        for t, px in tiles:
            ty, tx = divmod(t, tiles_x)
            self.map[TILE_H * ty:TILE_H * ty + px.shape[0], TILE_W * tx:TILE_W * tx + px.shape[1]] = px
        if self.crc() != crc:
            raise ValueError("MapTiles: the map after the tiles has CRC %08x, the message says %08x" % (self.crc(), crc))


def _encode(call):
    n = C.c_uint64()
    L.check(call(None, 0, C.byref(n)))
    out = np.empty(int(n.value), np.uint8)
    L.check(call(out.ctypes.data, out.size, C.byref(n)))
    return out.tobytes()


def encode_markers(lines, custom=False):
    """Event::Markers (web/src/lib.rs:142-152): lines float32 [n, 4] = (p0.x, p0.y, p1.x, p1.y) -> bytes."""
    ln = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
    lib = L.load()
    return _encode(lambda out, cap, n: lib.smhv_web_event_markers(ln.ctypes.data if len(ln) else None, len(ln), int(bool(custom)), out, cap, n))


def encode_heightmap(data=None, bounds=((0, 0), (0, 0)), scale=(1.0, 1.0, 1.0)):
    """Event::Heightmap (lib.rs:178-206): data uint16 [h, w] or None -> bytes."""
    lib = L.load()
    if data is None:
        return _encode(lambda out, cap, n: lib.smhv_web_event_heightmap(None, 0, 0, None, None, out, cap, n))
    d = np.ascontiguousarray(data, np.uint16)
    b = (C.c_int32 * 4)(*[int(v) for pair in bounds for v in pair])
    sc = (C.c_float * 3)(*[float(v) for v in scale])
    return _encode(lambda out, cap, n: lib.smhv_web_event_heightmap(d.ctypes.data, d.shape[1], d.shape[0], b, sc, out, cap, n))


def encode_fit(fit_to_minimap):
    """Event::HeightmapFitToMinimap (lib.rs:208-213) -> bytes."""
    lib = L.load()
    return _encode(lambda out, cap, n: lib.smhv_web_event_fit(int(bool(fit_to_minimap)), out, cap, n))


def parse_interaction(data):
    """Interaction::deserialize (lib.rs:37-71): a client's reply -> ("add", float32[4] = p0.x, p0.y, p1.x, p1.y), ("delete", index)
    or None."""
    buf = np.frombuffer(bytes(data), np.uint8)
    kind, index = C.c_uint32(), C.c_uint32()
    line = np.zeros(4, np.float32)
    L.check(L.load().smhv_web_interaction_parse(buf.ctypes.data if buf.size else None, buf.size, C.byref(kind), line.ctypes.data_as(C.POINTER(C.c_float)), C.byref(index)))
    if kind.value == 1:
        return "add", line
    if kind.value == 2:
        return "delete", int(index.value)
    return None
