"""The reference web server's protocol, restated with struct.pack and zlib.crc32 from web/src/lib.rs:37-214, web/src/ws.rs:35-55,
src/ui/state.rs:81-88 and src/ui/map.rs:213-233: what the remote-viewer feed (include/smh_vision_hip.h) is compared with, byte
for byte.  Pure Python; needs neither the library nor a device."""
import struct
import zlib

import numpy as np

MAP, MARKERS, UPDATE_STATE, HEIGHTMAP, FIT_TO_MINIMAP = 1, 2, 3, 4, 5   # the macro at lib.rs:74-126 numbers the variants from 1
FRAME_OK = 0
MAX_LINES = 32


# ---- Event::serialize (lib.rs:127-214): the u16 id, then the variant's fields, all little endian ----
def update_state(mpx, minimap):
    """mpx: float or None (unwrap_or(0.0)); minimap: (left, right, top, bottom) or None."""
    out = struct.pack("<Hd", UPDATE_STATE, 0.0 if mpx is None else mpx)
    return out + (b"\x00" if minimap is None else b"\x01" + struct.pack("<4I", *[int(v) for v in minimap]))


def map_event(w, h, rgba):
    rgba = bytes(rgba)
    assert len(rgba) == w * h * 4
    return struct.pack("<HII", MAP, w, h) + rgba


def markers(lines, custom=False):
    ln = np.ascontiguousarray(lines, "<f4").reshape(-1, 4)     # p0.x, p0.y, p1.x, p1.y per marker, bit for bit
    return struct.pack("<HBI", MARKERS, 1 if custom else 0, len(ln)) + ln.tobytes()


def heightmap(data=None, bounds=((0, 0), (0, 0)), scale=(1.0, 1.0, 1.0)):
    if data is None:
        return struct.pack("<HB", HEIGHTMAP, 0)
    d = np.ascontiguousarray(data, "<u2")
    h, w = d.shape
    # the flag, then the pad byte that keeps the u16 texels on an even offset (lib.rs:192-194)
    return struct.pack("<HBBIIiif", HEIGHTMAP, 1, 0, w, h, int(bounds[0][0]), int(bounds[0][1]), scale[2]) + d.tobytes()


def fit(flag):
    return struct.pack("<HB", FIT_TO_MINIMAP, 1 if flag else 0)


def parse_interaction(data):
    """Interaction::deserialize (lib.rs:37-71) -> ("add", 16 raw bytes of f32 x 4), ("delete", index) or None."""
    data = bytes(data)
    if len(data) < 2:
        return None
    (kind,), rest = struct.unpack("<H", data[:2]), data[2:]
    if kind == 1:
        return ("add", rest) if len(rest) == 16 else None
    if kind == 2:
        return ("delete", struct.unpack("<I", rest)[0]) if len(rest) == 4 else None
    return None


# ---- what one processed frame sends (state.rs:81-88, map.rs:213-233) and what a new client gets (ws.rs:35-55) ----
def frame_events(frame, stored, snapshot=False):
    """frame = (map_open, status, (w, h, ui_map bytes), lines, has_mpx, mpx, has_minimap, minimap); stored: the CRC-32 the
    current texture was made from, or None.  -> ([(kind, bytes)], crc of the map or None, the stored CRC afterwards)."""
    map_open, status, ui, lines, has_mpx, mpx, has_minimap, minimap = frame
    if not map_open or status != FRAME_OK:                     # sleeping / dropped on Err: nothing, and the texture stays
        return [], None, stored
    w, h, rgba = ui
    crc = zlib.crc32(bytes(rgba)) & 0xFFFFFFFF
    u = (UPDATE_STATE, update_state(mpx if has_mpx else None, minimap if has_minimap else None))
    m = (MAP, map_event(w, h, rgba))
    k = (MARKERS, markers(lines, False))
    if snapshot:
        out = [m] + ([u] if has_mpx or has_minimap else []) + ([k] if len(lines) else [])
        return out, crc, stored
    if stored is None or crc != stored:
        return [u, m, k], crc, crc
    return [u, k], crc, stored


def slot(n):
    """Messages start at offsets = 6 (mod 16): what a message of n bytes takes of the buffer."""
    return (n + 15) & ~15


def feed(frames, stored=None, capacity=None, snapshot=False, first=0):
    """The feed over `frames` in order.  A frame's events are written whole or not at all: a frame fits when its last message
    ends at or before `capacity` (None: no limit); the first frame that does not fit ends the call.
    -> dict(messages=[(frame, kind, crc, bytes)], entries=[(frame, kind, length, crc, offset)], frames_done, n_maps, stored,
    bytes_used)."""
    off, used, done, n_maps = 6, 0, 0, 0
    messages, entries = [], []
    for i, fr in enumerate(frames):
        ev, crc, after = frame_events(fr, stored, snapshot)
        if ev:
            o, placed = off, []
            for kind, data in ev:
                placed.append((o, kind, data))
                o += slot(len(data))
            end = placed[-1][0] + len(placed[-1][2])
            if capacity is not None and end > capacity:
                break
            for po, kind, data in placed:
                messages.append((first + i, kind, crc, data))
                entries.append((first + i, kind, len(data), crc, po))
                n_maps += kind == MAP
            off, used = o, end
        stored = after
        done = i + 1
    return dict(messages=messages, entries=entries, frames_done=done, n_maps=n_maps, stored=stored, bytes_used=used)


def worst_case(w, h):
    """One frame's worst case in the buffer: UpdateState with bounds, a Map, 32 marker lines."""
    return 6 + slot(27) + slot(10 + w * h * 4) + 7 + 16 * MAX_LINES
