"""The remote-viewer feed (smhv_feed_* / smhv_batch_feed / smhv_feed_frame): the reference web server's events of every processed
frame (web/src/lib.rs:127-214), written on the device, and the host-only rest of its protocol.  FrameBatch.feed and
HipVision.feed_frame take map_source = a VIEW_* of _lib: that debug view is hashed and sent as the Map in the ui_map's place
(smhv_batch_feed_view / smhv_feed_frame_view; src/ui/map.rs:210).  Transport is the caller's: a
message from WebFeed.read() or an encoder is what the reference hands its websocket as one binary frame."""
import ctypes as C

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
