"""8-bit 4:2:0 video frames (NV12 / I420) -> BGRA on the device (include/smh_vision_hip.h, SMHV_PIXELS_NV12 / _I420).

A video decoder, on the host or the GPU's own, leaves planes of 1.5 bytes per pixel.  yuv_to_bgra turns decoded surfaces that
already sit in device memory into the BGRA frames FrameBatch.run, Pipeline.submit and HipVision.load_frame_device take;
IngestQueue.push_pixels / commit take the same layouts from the host.  The arithmetic is the header's, to the bit.

The other way, for a hardware encoder: bgra_to_yuv turns RGBA / BGRA images in device memory into NV12 / I420 frames
(FrameBatch.video does it for a batch's render slab and ui_map), again by the header's integer arithmetic.
"""
import ctypes as C

from . import _lib
from ._lib import check

LAYOUTS = {"nv12": _lib.PIXELS_NV12, "i420": _lib.PIXELS_I420}
MATRICES = {"709": 0, "601": 1}
CHROMA = {"nearest": 0, "bilinear": 1}


def pixels(layout, matrix="709", full_range=False, chroma="nearest"):
    """SMHV_PIXELS_YUV(layout, matrix, range, chroma): layout "nv12" / "i420", matrix "709" / "601", chroma "nearest" / "bilinear"."""
    return LAYOUTS[layout] | (MATRICES[str(matrix)] << 8) | ((1 if full_range else 0) << 9) | (CHROMA[chroma] << 10)


def staging_bytes(w, h, layout):
    """Bytes of a tight frame of w x h in `layout` (any layout name of the ingest queue): what a staging buffer holds of it."""
    from .ingest import PIXEL_LAYOUTS
    code = LAYOUTS[layout] if layout in LAYOUTS else PIXEL_LAYOUTS[layout][0]
    n = int(_lib.load().smhv_ingest_staging_bytes(int(w), int(h), code))
    if n == 0:
        check(_lib.E_INVALID)
    return n


def yuv_layout(y_pitch=0, uv_pitch=0, u_offset=0, v_offset=0, frame_stride=0):
    """smhv_yuv_layout in bytes; a zero member means tight."""
    return _lib.YuvLayout(int(y_pitch), int(uv_pitch), int(u_offset), int(v_offset), int(frame_stride))


def yuv_to_bgra(vision, src_ptr, n, w, h, pixels, layout=None, out_ptr=None, out_stride=0, roi_only=False, stream=None):
    """smhv_yuv_to_bgra_device: n decoded surfaces at device address src_ptr -> n BGRA frames at out_ptr, out_stride bytes apart
    (0: w * h * 4).  pixels: yuv.pixels(...); layout: None (tight), a yuv_layout(...) or a dict of its members.  roi_only: the map
    ROI's and the button's rectangles alone are written.  Asynchronous on `stream` (a HIP stream handle; None: the context's).
    out_ptr None: a zeroed torch uint8 tensor [n, h, w, 4] on the current device is allocated and returned after the device has
    finished; otherwise returns None at once."""
    if isinstance(layout, dict):
        layout = yuv_layout(**layout)
    out = None
    if out_ptr is None:
        import torch
        out = torch.zeros((int(n), int(h), int(w), 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        out_ptr, out_stride = out.data_ptr(), 0
    check(_lib.load().smhv_yuv_to_bgra_device(vision._ctx, C.c_void_p(int(src_ptr)), C.byref(layout) if layout is not None else None, int(n), int(w), int(h),
                                              int(pixels), C.c_void_p(int(out_ptr)), int(out_stride), _lib.YUV_ROI_ONLY if roi_only else 0,
                                              C.c_void_p(int(stream)) if stream else None))
    if out is not None:
        torch.cuda.synchronize()
    return out


# ---- video frames OUT: RGBA / BGRA images -> NV12 / I420 (include/smh_vision_hip.h, "video frames OUT") -------------------------

def video_bytes(w, h, pixels):
    """smhv_video_bytes: bytes of a tight frame of w x h in the output word `pixels` (yuv.pixels(...) with nearest chroma)."""
    n = int(_lib.load().smhv_video_bytes(int(w), int(h), int(pixels)))
    if n == 0:
        check(_lib.E_INVALID)
    return n


def _video_out(n, w, h, pixels):
    """A zeroed torch uint8 tensor [n, video_bytes(w, h, pixels)] on the current device, already there."""
    import torch
    out = torch.zeros((int(n), video_bytes(w, h, pixels)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return out


def bgra_to_yuv(vision, src_ptr, n, w, h, pixels, rgba=False, src_pitch=0, src_stride=0, layout=None, out_ptr=None, stream=None):
    """smhv_bgra_to_yuv_device: n BGRA8 images (rgba: RGBA8) at device address src_ptr, rows src_pitch and images src_stride bytes
    apart (0: tight) -> n video frames at out_ptr.  pixels: yuv.pixels(...) with nearest chroma (the output's chroma is always the
    2 x 2 box; a word with the bilinear bit is refused by the library); layout: None (tight), a yuv_layout(...) or a dict of its
    members.  Asynchronous on `stream` (a HIP stream handle; None: the context's).  out_ptr None: a torch uint8 tensor
    [n, video_bytes(w, h, pixels)] of tight frames is allocated and returned after the device has finished; otherwise returns None
    at once."""
    if isinstance(layout, dict):
        layout = yuv_layout(**layout)
    out = None
    if out_ptr is None:
        import torch
        out = _video_out(n, w, h, pixels)
        out_ptr, layout = out.data_ptr(), None
    check(_lib.load().smhv_bgra_to_yuv_device(vision._ctx, C.c_void_p(int(src_ptr)), int(src_pitch), int(src_stride), int(n), int(w), int(h),
                                              _lib.VIDEO_SRC_RGBA if rgba else 0, int(pixels), C.c_void_p(int(out_ptr)),
                                              C.byref(layout) if layout is not None else None, C.c_void_p(int(stream)) if stream else None))
    if out is not None:
        torch.cuda.synchronize()
    return out
