"""Heightmaps on the device (smhv_heightmap_*): the range / altitude-difference source of the firing solutions
(src/ui/markers.rs:37-91) and the overlay colours (color_map_heightmap, src/ui/heightmaps.rs:169-207), plus the app's own
saved files ("SMHHM", src/squadex/heightmaps/serde.rs)."""
import ctypes as C
import lzma
import struct

import numpy as np

from . import _lib as L

SMHHM_MAGIC = 0xBADFEEF
SMHHM_VERSION = 0


def read_smhhm(path):
    """-> (data u16 [h, w], bounds ((b00, b01), (b10, b11)), scale (x, y, z)), or None for a wrong magic or version (as the
    reference's deserialize returns Ok(None))."""
    with open(path, "rb") as f:
        head = f.read(10)
        if len(head) < 10:
            raise EOFError("%s: truncated SMHHM header" % path)
        m0, ver, m1 = struct.unpack(">I", head[:4])[0], struct.unpack("<H", head[4:6])[0], struct.unpack(">I", head[6:10])[0]
        if m0 != SMHHM_MAGIC or ver != SMHHM_VERSION or m1 != SMHHM_MAGIC:
            return None
        rest = f.read(8 + 16 + 12)
        if len(rest) < 36:
            raise EOFError("%s: truncated SMHHM header" % path)
        w, h = struct.unpack("<II", rest[:8])
        b = struct.unpack("<4i", rest[8:24])
        scale = struct.unpack("<3f", rest[24:36])
        raw = lzma.LZMADecompressor(format=lzma.FORMAT_XZ).decompress(f.read(), max_length=w * h * 2)
    if len(raw) < w * h * 2:
        raise EOFError("%s: the texel stream holds %d of %d bytes" % (path, len(raw), w * h * 2))
    data = np.frombuffer(raw[:w * h * 2], "<u2").reshape(h, w).copy()
    return data, ((b[0], b[1]), (b[2], b[3])), scale


def write_smhhm(path, data, bounds, scale):
    """serialize (serde.rs:18-39): BE magic, LE u16 version, BE magic, LE w, h, four i32 bounds, three f32 scale values, then
    an xz stream of the w*h LE u16 texels."""
    data = np.ascontiguousarray(data, "<u2")
    h, w = data.shape
    b = np.asarray(bounds, np.int32).reshape(4)
    head = struct.pack(">I", SMHHM_MAGIC) + struct.pack("<H", SMHHM_VERSION) + struct.pack(">I", SMHHM_MAGIC)
    head += struct.pack("<II", w, h) + struct.pack("<4i", *[int(v) for v in b]) + struct.pack("<3f", *[float(v) for v in scale])
    with open(path, "wb") as f:
        f.write(head)
        f.write(lzma.compress(data.tobytes(), format=lzma.FORMAT_XZ, preset=9))


class Heightmap:
    """A device copy of a heightmap (heightmap-ripper's Heightmap: w x h u16 texels, bounds [[i32; 2]; 2], scale [f32; 3]).
    Bind it with FrameBatch.set_firing / Pipeline.set_firing or pass it to HipVision.firing_solutions."""

    def __init__(self, vision, data_u16, bounds, scale):
        self._lib = L.load()
        self._vision = vision                      # keeps the context alive
        data = np.ascontiguousarray(data_u16, np.uint16)
        if data.ndim != 2:
            raise ValueError("data_u16 must be a 2-D array [h, w]")
        self.data = data
        self.height_px, self.width = data.shape
        self.bounds = tuple(tuple(int(v) for v in row) for row in np.asarray(bounds, np.int64).reshape(2, 2))
        self.scale = tuple(float(np.float32(v)) for v in scale)
        b = (C.c_int32 * 4)(*[v for row in self.bounds for v in row])
        s = (C.c_float * 3)(*self.scale)
        hm = C.c_void_p()
        L.check(self._lib.smhv_heightmap_create(vision._ctx, data.ctypes.data, self.width, self.height_px, b, s, C.byref(hm)))
        self._hm = hm

    @classmethod
    def load(cls, vision, path):
        """A heightmap file the app saved (SMHHM); None for a wrong magic or version."""
        r = read_smhhm(path)
        if r is None:
            return None
        data, bounds, scale = r
        return cls(vision, data, bounds, scale)

    def save(self, path):
        write_smhhm(path, self.data, self.bounds, self.scale)

    def height(self, x, y):
        """Heightmap::height (heightmap-ripper/src/lib.rs:22-25) in f64."""
        v = int(self.data[y, x])
        return (v / 65535.0) * (float(np.float32(self.scale[2])) / 0.1953125)

    def color_map(self):
        """color_map_heightmap (src/ui/heightmaps.rs:169-207) on the device -> uint8 [h, w, 4] RGBA."""
        out = np.empty((self.height_px, self.width, 4), np.uint8)
        L.check(self._lib.smhv_heightmap_color_map(self._hm, out.ctypes.data))
        return out

    def color_map_device_ms(self, d_rgba):
        """Calibration: both colour-map passes into w*h*4 bytes of device memory at d_rgba -> their device time in ms."""
        ms = C.c_float(0.0)
        L.check(self._lib.smhv_debug_heightmap_color_map_device(self._hm, C.c_void_p(d_rgba), C.byref(ms)))
        return float(ms.value)

    def close(self):
        if getattr(self, "_hm", None):
            self._lib.smhv_heightmap_destroy(self._hm)
            self._hm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
