"""Resident-batch pipeline (BASELINE configs 2-5): N frames stay in HBM, one result record per frame.

torch is used only as plumbing (device memory for the frame batch, the current HIP stream and
torch.distributed); every kernel is in libsmh_vision_hip.so.
"""
import ctypes as C
from collections.abc import Mapping

import numpy as np

from . import _lib as L

STAGE_NAMES = ("button", "map_pass", "brq_pass", "lsd", "scale_ratio")


def make_anchors(per_frame):
    """per_frame: list (len n) of (scales_start_y, [(meters, x, y), ...]) -> ctypes array of smhv_anchors."""
    arr = (L.Anchors * len(per_frame))()
    for i, (start_y, scales) in enumerate(per_frame):
        arr[i].n = min(len(scales), L.MAX_SCALES)
        arr[i].scales_start_y = start_y
        for j, (m, x, y) in enumerate(scales[:L.MAX_SCALES]):
            arr[i].scales[j][0], arr[i].scales[j][1], arr[i].scales[j][2] = m, x, y
    return arr


def results_to_dicts(recs):
    out = []
    for r in recs:
        n = r.n_lines
        out.append(dict(
            map_open=int(r.map_open), n_lines=int(n),
            lines=np.array([[r.lines[i].x0, r.lines[i].y0, r.lines[i].x1, r.lines[i].y1] for i in range(n)], np.float32).reshape(-1, 4),
            mpx=(r.mpx if r.has_mpx else None), n_mask_px=int(r.n_mask_px), red_pixels=int(r.red_pixels),
            rounds=int(r.rounds), ray_steps=int(r.ray_steps),
            length_px=np.array(r.length_px[:n], np.float64), meters=np.array(r.meters[:n], np.float64),
            angle=np.array(r.angle[:n], np.float32),
            minimap=(tuple(r.minimap) if r.has_minimap else None),
            status=int(r.status), error=(None if r.status == L.FRAME_OK else "line search gave the frame up (SMHV_FRAME_LSD_STUCK)" if r.status == L.FRAME_LSD_STUCK
                                         else "status %d" % r.status)))
    return out


_PTR_KEYS = ("results", "ui", "mask", "ocr", "scales", "bits")


def _ptr(address):
    return C.c_void_p(int(address)) if address else None


class _DevicePtrs(Mapping):
    """FrameBatch.device_ptrs(): read-only; the "mask" and "ui" entries ask the library for d_mask / d_ui the first time they are read."""

    def __init__(self, batch, ptrs):
        self._batch, self._ptrs = batch, ptrs

    def __getitem__(self, key):
        if key == "mask" and self._ptrs["mask"] is None:
            self._ptrs["mask"] = self._batch._mask_ptr()
        if key == "ui" and self._ptrs["ui"] is None:
            self._ptrs["ui"] = self._batch._ui_ptr()
        return self._ptrs[key]

    def __iter__(self):
        return iter(_PTR_KEYS)

    def __len__(self):
        return len(_PTR_KEYS)


class FrameBatch:
    """Owns the output buffers for up to `max_frames` frames of one size on one device."""

    def __init__(self, vision, frame_w, frame_h, max_frames, _handle=None):
        self._lib = L.load()
        self._vision = vision            # keeps the context alive
        self._owned = _handle is None    # a pipeline slot's batch belongs to the pipeline
        if _handle is None:
            b = C.c_void_p()
            L.check(self._lib.smhv_batch_create(vision._ctx, frame_w, frame_h, max_frames, C.byref(b)))
        else:
            b = _handle
        self._b = b
        self.max_frames = max_frames
        self.frame_w, self.frame_h = frame_w, frame_h
        self.layout = L.BatchLayout()
        L.check(self._lib.smhv_batch_layout_get(self._b, C.byref(self.layout)))

    def close(self):
        if self._b:
            if self._owned:
                self._lib.smhv_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def roi(self):
        return tuple(self.layout.roi)

    def enable_timing(self, on=True):
        L.check(self._lib.smhv_batch_enable_timing(self._b, int(on)))

    def run(self, frames_ptr, n, stages=L.STAGE_ALL, grayscale=True, max_gap=15, anchors=None, stream=0):
        """frames_ptr: device address of n tightly packed BGRA8 frames.  Asynchronous on `stream`."""
        if anchors is not None and len(anchors) < n:
            raise ValueError("anchors holds %d entries, the run covers %d frames" % (len(anchors), n))
        a = C.cast(anchors, C.c_void_p) if anchors is not None else None
        L.check(self._lib.smhv_batch_run(self._b, C.c_void_p(frames_ptr), n, stages, int(bool(grayscale)), max_gap, a, C.c_void_p(stream)))

    def set_scales_stream(self, stream=0):
        """Scales branch on a caller-provided HIP stream (0: the batch's own); see smhv_batch_set_scales_stream."""
        L.check(self._lib.smhv_batch_set_scales_stream(self._b, C.c_void_p(stream)))

    def wait_map_pass(self, stream=0):
        """`stream` waits for the streaming pass of this batch's most recent run (see smhv_batch_wait_map_pass)."""
        L.check(self._lib.smhv_batch_wait_map_pass(self._b, C.c_void_p(stream)))

    def stage_ms(self):
        ms = (C.c_float * 5)()
        L.check(self._lib.smhv_batch_stage_ms(self._b, ms))
        return dict(zip(STAGE_NAMES, [float(v) for v in ms]))

    def lsd_coop_stats(self, first=0, n=None):
        """Diagnostic: uint32[n, 4] = (helped groups, cache hits, helper casts, requests posted) per frame of the last LSD launch."""
        n = self.max_frames - first if n is None else n
        out = np.zeros((n, 4), np.uint32)
        L.check(self._lib.smhv_batch_lsd_coop_stats(self._b, first, n, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def device_ptrs(self):
        """Mapping of the output slabs' device addresses ("results", "ui", "mask", "ocr", "scales", "bits").  "mask" and "ui" are fetched
        when they are first read: asking the library for d_mask makes the batch write the byte mask behind every run from then on, and
        asking it for d_ui makes grey runs write the RGBA slab themselves instead of the luma plane (smhv_batch_device_ptrs) -- which a
        caller that reads the other slabs only never pays."""
        p = [C.c_void_p() for _ in range(6)]
        args = [C.byref(x) for x in p]
        args[1] = args[2] = None
        L.check(self._lib.smhv_batch_device_ptrs(self._b, *args))
        return _DevicePtrs(self, dict(zip(_PTR_KEYS, [x.value for x in p])))

    def _mask_ptr(self):
        m = C.c_void_p()
        L.check(self._lib.smhv_batch_device_ptrs(self._b, None, None, C.byref(m), None, None, None))
        return m.value

    def _ui_ptr(self):
        u = C.c_void_p()
        L.check(self._lib.smhv_batch_device_ptrs(self._b, None, C.byref(u), None, None, None, None))
        return u.value

    def ui_state(self):
        """(frames whose RGBA ui slab may be owed, whether grey runs write it themselves): smhv_debug_batch_ui_state."""
        stale, eager = C.c_uint32(0), C.c_int(0)
        L.check(self._lib.smhv_debug_batch_ui_state(self._b, C.byref(stale), C.byref(eager)))
        return int(stale.value), bool(eager.value)

    def materialize_ui(self, stream=0):
        """Diagnostic: what the grey runs so far owe the RGBA ui slab is made on `stream` now (what every reader of the slab does first)."""
        L.check(self._lib.smhv_debug_batch_materialize_ui(self._b, C.c_void_p(stream)))

    def mask_state(self):
        """(frames whose byte mask is owed, whether every run writes it): smhv_debug_batch_mask_state."""
        stale, eager = C.c_uint32(0), C.c_int(0)
        L.check(self._lib.smhv_debug_batch_mask_state(self._b, C.byref(stale), C.byref(eager)))
        return int(stale.value), bool(eager.value)

    def tile_mask(self, frame=0):
        """The marker mask of one frame as the streaming passes leave it for the line search: (tiled uint32[tile_rows, word_columns, 8],
        occ uint8[tile_rows, occ_pitch], bits uint32[rows, word_columns], bits_xoff) -- include/smh_vision_hip.h, smhv_batch_tile_mask.
        tiled and occ are None when the last run wrote the bit rows only (bands that are not whole tile rows)."""
        geo = (C.c_uint32 * 4)()
        L.check(self._lib.smhv_batch_tile_mask(self._b, None, None, geo))
        trows, wcols, opitch, xoff = [int(v) for v in geo]
        tiled = np.zeros((trows, wcols, 8), np.uint32)
        occ = np.zeros((trows, opitch), np.uint8)
        bits = np.zeros((self.roi[3], wcols), np.uint32)
        written = C.c_int(0)
        L.check(self._lib.smhv_batch_read_tile_mask(self._b, frame, tiled.ctypes.data, occ.ctypes.data, bits.ctypes.data, C.byref(written)))
        return (tiled if written.value else None), (occ if written.value else None), bits, xoff

    def _read_slab(self, fn, ctype, first, n, per_frame=1):
        """Synchronising host copy of rows [first, first + n) of a result slab (a smhv_batch_read_*) -> a ctypes array of n * per_frame ctype."""
        n = self.max_frames - first if n is None else n
        out = (ctype * (n * per_frame))()
        L.check(fn(self._b, first, n, out))
        return out

    def _slab_ptr(self, fn, k=1):
        """The device address(es) a smhv_batch_*_ptr hands out: one int, or a tuple of k."""
        d = [C.c_void_p() for _ in range(k)]
        L.check(fn(self._b, *[C.byref(x) for x in d]))
        return d[0].value or 0 if k == 1 else tuple(x.value or 0 for x in d)

    @staticmethod
    def _plane(made, name, ptr, asked, shape, dtype="uint8"):
        """The device address of an output plane: `ptr`, or, when the plane is asked for and ptr is None, that of a zeroed torch tensor of
        `shape` allocated here and kept in made[name]."""
        if asked and ptr is None:
            import torch
            made[name] = torch.zeros(shape, dtype=getattr(torch, dtype), device="cuda")
            ptr = made[name].data_ptr()
        return ptr

    @staticmethod
    def _call(made, fn, *args):
        """fn(*args), checked; when planes were allocated here (`made`), after their zeros are in place, and the device has finished on return."""
        if made:
            import torch
            torch.cuda.synchronize()
        L.check(fn(*args))
        if made:
            torch.cuda.synchronize()

    def read_results(self, first=0, n=None, check=True):
        """Synchronising host copy of the records.  A frame the library gave up (status != 0 in its record) makes the call
        raise VisionError(E_STATE) -- the reference drops a frame on any Err (src/vision/mod.rs:272-276); check=False returns
        the records regardless, for a caller that drops exactly those frames."""
        n = self.max_frames - first if n is None else n
        recs = (L.FrameResult * n)()
        rc = self._lib.smhv_batch_read_results(self._b, first, n, recs)
        if rc != 0 and not (rc == L.E_STATE and not check):
            try:
                L.check(rc)
            except L.VisionError as e:
                # the library reports the condition ONCE and has copied the records out: they travel with the exception
                # (frames whose status is set are to be dropped; the others are valid), a retry would not see the error again
                e.records = recs if rc == L.E_STATE else None
                raise
        return recs

    def set_firing(self, heightmap=None, fit_to_minimap=True, viewport=None):
        """Bind a Heightmap (None = none) and the options for STAGE_FIRING runs of this batch (smhv_batch_set_firing; the
        library keeps its own reference of the heightmap).  Without a call the runs use no heightmap and the default options."""
        opt = L.firing_options(fit_to_minimap, viewport)
        L.check(self._lib.smhv_batch_set_firing(self._b, L._hm(heightmap), C.byref(opt)))

    def read_firing(self, first=0, n=None):
        """Synchronising host copy of the firing slab -> (n_lines uint32 [n], numpy structured array [n, MAX_LINES] of smhv_firing)."""
        out = self._read_slab(self._lib.smhv_batch_read_firing, L.FiringResult, first, n)
        raw = np.frombuffer(out, np.uint8).reshape(len(out), C.sizeof(L.FiringResult))
        n_lines = raw[:, :4].copy().view(np.uint32).reshape(len(out))
        lines = raw[:, 8:].copy().view(L.firing_dtype()).reshape(len(out), L.MAX_LINES)
        return n_lines, lines

    def firing_ptr(self):
        return self._slab_ptr(self._lib.smhv_batch_firing_ptr)

    def read_overlay(self, frame):
        """Synchronising host copy of a frame's heightmap overlay (STAGE_HEIGHTMAP_OVERLAY) -> uint8 [h, w, 4] RGBA."""
        return self.read_image(L.IMAGE_HEIGHTMAP_OVERLAY, frame)

    def overlay_ptr(self):
        """Device address of the overlay slab (the ui slab's layout: layout.ui_pitch / ui_stride / ui_offset)."""
        return self._slab_ptr(self._lib.smhv_batch_overlay_ptr)

    def render(self, viewport, out_w, out_h, first=0, n=None, heightmap=None, markers=False, fit_to_minimap=True, background=(0, 0, 0, 255),
               stream=None, options=None, layers=None):
        """Draw the map view of frames [first, first + n) into the render slab on `stream` (smhv_batch_render): the ui_map through
        `viewport` (a MapViewport) into a window of out_w x out_h, the heightmap's overlay when `heightmap` is given, the records'
        marker lines when `markers`.  Asynchronous.  options: a ready RenderOptions instead of the keyword arguments.  layers: a
        RenderLayers (smhv_batch_render_layers): prims, the minimap bounds, a debug view as the map."""
        from .render import render_options
        n = self.max_frames - first if n is None else n
        opt = options if options is not None else render_options(viewport, out_w, out_h, heightmap is not None, markers, fit_to_minimap, background)
        if layers is not None:
            ly, keep = layers.struct()
            L.check(self._lib.smhv_batch_render_layers(self._b, first, n, L._hm(heightmap), C.byref(opt), C.byref(ly), stream))
            del keep
            return
        L.check(self._lib.smhv_batch_render(self._b, first, n, L._hm(heightmap), C.byref(opt), stream))

    def render_size(self):
        """(out_w, out_h) of the most recent render, from the library."""
        w, h = C.c_uint32(), C.c_uint32()
        L.check(self._lib.smhv_batch_render_size(self._b, C.byref(w), C.byref(h)))
        return int(w.value), int(h.value)

    def read_render(self, frame):
        """Synchronising host copy of a frame's image of the most recent render -> uint8 [out_h, out_w, 4] RGBA."""
        w, h = self.render_size()
        out = np.empty((h, w, 4), np.uint8)
        L.check(self._lib.smhv_batch_read_render(self._b, frame, out.ctypes.data))
        return out

    def render_ptr(self):
        """(device address of the render slab, bytes per frame) of the most recent render."""
        d, st = C.c_void_p(), C.c_uint64()
        L.check(self._lib.smhv_batch_render_ptr(self._b, C.byref(d), C.byref(st)))
        return d.value or 0, int(st.value)

    def render_labels(self, options, labels, first=0, n=None, heightmap=None, stream=None):
        """Draw the marker labels onto the images of the most recent render over frames [first, first + n) on `stream`
        (smhv_batch_render_labels) and write the label slab.  options: the RenderOptions of that render (the window and the
        viewport); labels: a LabelOptions; heightmap: what the numbers take their range and altitude from.  Asynchronous."""
        n = self.max_frames - first if n is None else n
        lo, keep = labels.struct()
        L.check(self._lib.smhv_batch_render_labels(self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(lo), stream))
        del keep

    def read_labels(self, first=0, n=None):
        """Synchronising host copy of the label slab -> a ctypes array of n LabelResult."""
        return self._read_slab(self._lib.smhv_batch_read_labels, L.LabelResult, first, n)

    def labels_ptr(self):
        """Device address of the label slab (one smhv_label_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_labels_ptr)

    def reach(self, options, reach, first=0, n=None, heightmap=None, classes_ptr=None, stream=None):
        """The reach map of frames [first, first + n) on `stream` (smhv_batch_reach): options = a RenderOptions (the window and the
        viewport; with paint the most recent render's), reach = a ReachOptions, heightmap = what range and altitude come from.
        With reach.classes and classes_ptr None a torch uint8 tensor [n, out_h, out_w] is allocated, filled and returned (the call
        then returns after the device has finished); with classes_ptr (device memory, n * out_h * out_w bytes) the call is
        asynchronous and returns None, as it does without classes."""
        n = self.max_frames - first if n is None else n
        ro = reach.struct()
        made = {}
        classes_ptr = self._plane(made, "classes", classes_ptr, reach.classes, (n, int(options.out_h), int(options.out_w)))
        self._call(made, self._lib.smhv_batch_reach, self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(ro), _ptr(classes_ptr), _ptr(stream))
        return made.get("classes")

    def read_reach(self, first=0, n=None):
        """Synchronising host copy of the reach slab -> a ctypes array of n ReachResult."""
        return self._read_slab(self._lib.smhv_batch_read_reach, L.ReachResult, first, n)

    def reach_ptr(self):
        """Device address of the reach slab (one smhv_reach_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_reach_ptr)

    def relief(self, options, relief, first=0, n=None, heightmap=None, bytes_ptr=None, shades_ptr=None, heights_ptr=None, stream=None):
        """The terrain relief of frames [first, first + n) on `stream` (smhv_batch_relief): options = a RenderOptions (the window and
        the viewport; with paint the most recent render's), relief = a ReliefOptions, heightmap = the terrain.  A plane that relief
        asks for and that has no pointer (device memory, n * out_h * out_w elements) is allocated as a torch tensor [n, out_h,
        out_w] (uint8, uint8, float32), and the call then returns after the device has finished; with every plane's pointer given,
        or no plane, it is asynchronous.  -> dict(bytes=, shades=, heights=) of the tensors allocated here."""
        n = self.max_frames - first if n is None else n
        ro = relief.struct()
        out = {}
        shape = (n, int(options.out_h), int(options.out_w))
        ptrs = [self._plane(out, name, ptr, getattr(relief, name), shape, "float32" if name == "heights" else "uint8")
                for name, ptr in (("bytes", bytes_ptr), ("shades", shades_ptr), ("heights", heights_ptr))]
        planes = L.ReliefPlanes(*[int(p) if p else None for p in ptrs])
        self._call(out, self._lib.smhv_batch_relief, self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(ro), C.byref(planes), _ptr(stream))
        return out

    def read_relief(self, first=0, n=None):
        """Synchronising host copy of the relief slab -> a ctypes array of n ReliefResult."""
        return self._read_slab(self._lib.smhv_batch_read_relief, L.ReliefResult, first, n)

    def relief_ptr(self):
        """Device address of the relief slab (one smhv_relief_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_relief_ptr)

    def grid(self, options, grid, first=0, n=None, heightmap=None, bytes_ptr=None, cells_ptr=None, stream=None):
        """The map grid of frames [first, first + n) on `stream` (smhv_batch_grid): options = a RenderOptions (the window and the
        viewport; with paint the most recent render's), grid = a GridOptions, heightmap = the map's size in metres (None: the
        records' metres per pixel).  A plane that grid asks for and that has no pointer (device memory, n * out_h * out_w elements)
        is allocated as a torch tensor [n, out_h, out_w] (uint8; the cells int32, the u32 words' bits), and the call then returns
        after the device has finished; with every plane's pointer given, or no plane, it is asynchronous.
        -> dict(bytes=, cells=) of the tensors allocated here."""
        n = self.max_frames - first if n is None else n
        go = grid.struct()
        out = {}
        shape = (n, int(options.out_h), int(options.out_w))
        ptrs = [self._plane(out, name, ptr, getattr(grid, name), shape, "int32" if name == "cells" else "uint8")
                for name, ptr in (("bytes", bytes_ptr), ("cells", cells_ptr))]
        planes = L.GridPlanes(*[int(p) if p else None for p in ptrs])
        self._call(out, self._lib.smhv_batch_grid, self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(go), C.byref(planes), _ptr(stream))
        return out

    def read_grid(self, first=0, n=None):
        """Synchronising host copy of the grid slab -> a ctypes array of n GridResult."""
        return self._read_slab(self._lib.smhv_batch_read_grid, L.GridResult, first, n)

    def grid_ptr(self):
        """Device address of the grid slab (one smhv_grid_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_grid_ptr)

    def grid_refs(self, options, grid, first=0, n=None, heightmap=None, stream=None):
        """The grid references of the ends of the detected lines of frames [first, first + n) on `stream` (smhv_batch_grid_refs);
        options, grid, heightmap as grid() takes them.  Asynchronous; read_grid_refs() waits for the records."""
        n = self.max_frames - first if n is None else n
        go = grid.struct()
        L.check(self._lib.smhv_batch_grid_refs(self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(go), _ptr(stream)))

    def read_grid_refs(self, first=0, n=None):
        """Synchronising host copy of the references slab -> a ctypes array of n GridRefsResult."""
        return self._read_slab(self._lib.smhv_batch_read_grid_refs, L.GridRefsResult, first, n)

    def grid_refs_ptr(self):
        """Device address of the references slab (one smhv_grid_refs_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_grid_refs_ptr)

    def clearance(self, clearance, first=0, n=None, heightmap=None, fit_to_minimap=True, viewport=None, profiles_ptr=None, profiles=False, stream=None):
        """The terrain clearance of the detected lines of frames [first, first + n) on `stream` (smhv_batch_clearance): clearance = a
        ClearanceOptions (samples, margin_m); heightmap, fit_to_minimap, viewport as the firing solutions take them.  With
        profiles and profiles_ptr None a torch float32 tensor [n, MAX_LINES, CLEAR_PROFILE] is allocated, filled and returned (the
        call then returns after the device has finished); with profiles_ptr (device memory of that size) the call is asynchronous
        and returns None, as it does without profiles.  read_clearance() waits for the records."""
        n = self.max_frames - first if n is None else n
        co = clearance.struct()
        fo = L.firing_options(fit_to_minimap, viewport)
        made = {}
        profiles_ptr = self._plane(made, "profiles", profiles_ptr, profiles, (n, L.MAX_LINES, L.CLEAR_PROFILE), "float32")
        self._call(made, self._lib.smhv_batch_clearance, self._b, first, n, L._hm(heightmap), C.byref(fo), C.byref(co), _ptr(profiles_ptr), _ptr(stream))
        return made.get("profiles")

    def read_clearance(self, first=0, n=None):
        """Synchronising host copy of the clearance slab -> a ctypes array of n ClearanceResult."""
        return self._read_slab(self._lib.smhv_batch_read_clearance, L.ClearanceResult, first, n)

    def clearance_ptr(self):
        """Device address of the clearance slab (one smhv_clearance_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_clearance_ptr)

    def clearance_map(self, options, clearance, first=0, n=None, heightmap=None, bytes_ptr=None, stream=None):
        """The clearance map of frames [first, first + n) on `stream` (smhv_batch_clearance_map): options = a RenderOptions (the
        window and the viewport; with paint the most recent render's), clearance = a ClearanceOptions.  With clearance.bytes and
        bytes_ptr None a torch uint8 tensor [n, out_h, out_w] is allocated, filled and returned (the call then returns after the
        device has finished); with bytes_ptr (device memory, n * out_h * out_w bytes) the call is asynchronous and returns None,
        as it does without bytes."""
        n = self.max_frames - first if n is None else n
        co = clearance.struct()
        made = {}
        bytes_ptr = self._plane(made, "bytes", bytes_ptr, clearance.bytes, (n, int(options.out_h), int(options.out_w)))
        self._call(made, self._lib.smhv_batch_clearance_map, self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(co), _ptr(bytes_ptr), _ptr(stream))
        return made.get("bytes")

    def read_clearance_map(self, first=0, n=None):
        """Synchronising host copy of the clearance-map slab -> a ctypes array of n ClearanceMapResult."""
        return self._read_slab(self._lib.smhv_batch_read_clearance_map, L.ClearanceMapResult, first, n)

    def clearance_map_ptr(self):
        """Device address of the clearance-map slab (one smhv_clearance_map_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_clearance_map_ptr)

    def ballistics(self, weapon, first=0, n=None, heightmap=None, fit_to_minimap=True, viewport=None, stream=None):
        """The weapon's solutions of the detected lines of frames [first, first + n) on `stream` (smhv_batch_ballistics): weapon = a
        ballistics.Weapon; heightmap, fit_to_minimap, viewport as the firing solutions take them.  Asynchronous; read_ballistics()
        waits for the records."""
        n = self.max_frames - first if n is None else n
        w = weapon.struct()
        fo = L.firing_options(fit_to_minimap, viewport)
        L.check(self._lib.smhv_batch_ballistics(self._b, first, n, L._hm(heightmap), C.byref(fo), C.byref(w), _ptr(stream)))

    def read_ballistics(self, first=0, n=None):
        """Synchronising host copy of the ballistics slab -> a ctypes array of n BallisticResult."""
        return self._read_slab(self._lib.smhv_batch_read_ballistics, L.BallisticResult, first, n)

    def ballistics_ptr(self):
        """Device address of the ballistics slab (one smhv_ballistic_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_ballistics_ptr)

    def ballistic_map(self, options, weapon, ballistic, first=0, n=None, heightmap=None, classes_ptr=None, tof_ptr=None, stream=None):
        """The weapon's reach map of frames [first, first + n) on `stream` (smhv_batch_ballistic_map): options = a RenderOptions (the
        window and the viewport; with paint the most recent render's), weapon = a ballistics.Weapon, ballistic = a BallisticOptions.
        A plane that ballistic asks for and that has no pointer (device memory, n * out_h * out_w elements) is allocated as a torch
        tensor [n, out_h, out_w] (uint8, float32), and the call then returns after the device has finished; with every plane's
        pointer given, or no plane, it is asynchronous.  -> dict(classes=, tof=) of the tensors allocated here."""
        n = self.max_frames - first if n is None else n
        w, bo = weapon.struct(), ballistic.struct()
        out = {}
        shape = (n, int(options.out_h), int(options.out_w))
        ptrs = [self._plane(out, name, ptr, getattr(ballistic, name), shape, "float32" if name == "tof" else "uint8")
                for name, ptr in (("classes", classes_ptr), ("tof", tof_ptr))]
        planes = L.BallisticPlanes(*[int(p) if p else None for p in ptrs])
        self._call(out, self._lib.smhv_batch_ballistic_map, self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(w), C.byref(bo), C.byref(planes),
                   _ptr(stream))
        return out

    def read_ballistic_map(self, first=0, n=None):
        """Synchronising host copy of the ballistic-map slab -> a ctypes array of n BallisticMapResult."""
        return self._read_slab(self._lib.smhv_batch_read_ballistic_map, L.BallisticMapResult, first, n)

    def ballistic_map_ptr(self):
        """Device address of the ballistic-map slab (one smhv_ballistic_map_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_ballistic_map_ptr)

    def ballistic_clearance(self, weapon, clearance, first=0, n=None, heightmap=None, fit_to_minimap=True, viewport=None, stream=None):
        """Both arcs of the weapon against the terrain, for the detected lines of frames [first, first + n) on `stream`
        (smhv_batch_ballistic_clearance): weapon = a ballistics.Weapon, clearance = a BallisticClearanceOptions (samples, margin_m);
        heightmap, fit_to_minimap, viewport as the firing solutions take them.  Asynchronous; read_ballistic_clearance() waits."""
        n = self.max_frames - first if n is None else n
        w, co = weapon.struct(), clearance.struct()
        fo = L.firing_options(fit_to_minimap, viewport)
        L.check(self._lib.smhv_batch_ballistic_clearance(self._b, first, n, L._hm(heightmap), C.byref(fo), C.byref(w), C.byref(co), _ptr(stream)))

    def read_ballistic_clearance(self, first=0, n=None):
        """Synchronising host copy of the ballistic-clearance slab -> a ctypes array of n BallisticClearanceResult."""
        return self._read_slab(self._lib.smhv_batch_read_ballistic_clearance, L.BallisticClearanceResult, first, n)

    def ballistic_clearance_ptr(self):
        """Device address of the ballistic-clearance slab (one smhv_ballistic_clearance_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_ballistic_clearance_ptr)

    def ballistic_clearance_map(self, options, weapon, clearance, first=0, n=None, heightmap=None, bytes_ptr=None, margin_ptr=None, stream=None):
        """The ballistic clearance map of frames [first, first + n) on `stream` (smhv_batch_ballistic_clearance_map): options = a
        RenderOptions (the window and the viewport; with paint the most recent render's), weapon = a ballistics.Weapon, clearance = a
        BallisticClearanceOptions.  A plane that clearance asks for and that has no pointer (device memory, n * out_h * out_w
        elements) is allocated as a torch tensor [n, out_h, out_w] (uint8, float32), and the call then returns after the device has
        finished; with every plane's pointer given, or no plane, it is asynchronous.  -> dict(bytes=, margin=) of the tensors
        allocated here."""
        n = self.max_frames - first if n is None else n
        w, co = weapon.struct(), clearance.struct()
        out = {}
        shape = (n, int(options.out_h), int(options.out_w))
        ptrs = [self._plane(out, name, ptr, getattr(clearance, name), shape, "float32" if name == "margin" else "uint8")
                for name, ptr in (("bytes", bytes_ptr), ("margin", margin_ptr))]
        planes = L.BallisticClearancePlanes(*[int(p) if p else None for p in ptrs])
        self._call(out, self._lib.smhv_batch_ballistic_clearance_map, self._b, first, n, L._hm(heightmap), C.byref(options), C.byref(w), C.byref(co),
                   C.byref(planes), _ptr(stream))
        return out

    def read_ballistic_clearance_map(self, first=0, n=None):
        """Synchronising host copy of the ballistic-clearance-map slab -> a ctypes array of n BallisticClearanceMapResult."""
        return self._read_slab(self._lib.smhv_batch_read_ballistic_clearance_map, L.BallisticClearanceMapResult, first, n)

    def ballistic_clearance_map_ptr(self):
        """Device address of the ballistic-clearance-map slab (one smhv_ballistic_clearance_map_result per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_ballistic_clearance_map_ptr)

    def scale_labels(self, frames_ptr, n, stream=0):
        """The scale labels of frames [0, n) (smhv_batch_scale_labels), on `stream` behind this batch's run over the same frames
        (frames_ptr: what that run was given; its stages must include STAGE_OCR).  Asynchronous; read_scale_labels() waits for it."""
        L.check(self._lib.smhv_batch_scale_labels(self._b, C.c_void_p(frames_ptr), n, C.c_void_p(stream)))

    def read_scale_labels(self, first=0, n=None, crops=True):
        """Synchronising host copy of the label and crop slabs -> (a ctypes array of n ScaleLabelFrame, uint8 [n, MAX_SCALE_LABELS,
        LABEL_CROP_H, LABEL_CROP_W] or None); of a frame's cells only the first ScaleLabelFrame.n are its own."""
        n = self.max_frames - first if n is None else n
        out = (L.ScaleLabelFrame * n)()
        cells = np.empty((n, L.MAX_SCALE_LABELS, L.LABEL_CROP_H, L.LABEL_CROP_W), np.uint8) if crops else None
        L.check(self._lib.smhv_batch_read_scale_labels(self._b, first, n, out, cells.ctypes.data if cells is not None else None))
        return out, cells

    def scale_labels_ptr(self):
        """Device addresses of the label slab (one smhv_scale_label_frame per frame) and the crop slab."""
        return self._slab_ptr(self._lib.smhv_batch_scale_labels_ptr, 2)

    def label_text(self, atlas, n, stream=0):
        """The texts of the scale labels of frames [0, n) read against `atlas` (a GlyphAtlas; smhv_batch_label_text), on `stream`
        behind scale_labels() over at least n frames.  Asynchronous; read_label_text() waits for it."""
        L.check(self._lib.smhv_batch_label_text(self._b, atlas._a, n, C.c_void_p(stream)))

    def read_label_text(self, first=0, n=None):
        """Synchronising host copy of the text slab -> a ctypes array of n LabelTextFrame."""
        return self._read_slab(self._lib.smhv_batch_read_label_text, L.LabelTextFrame, first, n)

    def label_text_ptr(self):
        """Device addresses of the text slab (one smhv_label_text_frame per frame) and of the frames' smhv_anchors, tightly packed."""
        return self._slab_ptr(self._lib.smhv_batch_label_text_ptr, 2)

    def run_label_anchors(self, frames_ptr, n, stages=L.STAGE_ALL, grayscale=True, max_gap=15, stream=0):
        """run() with the anchors the last label_text() left on the device (smhv_batch_run_label_anchors): the meters never visit the host."""
        L.check(self._lib.smhv_batch_run_label_anchors(self._b, C.c_void_p(frames_ptr), n, stages, int(bool(grayscale)), max_gap, C.c_void_p(stream)))

    def probe(self, options, points, first=0, n=None, stream=None):
        """The vision debugger's numbers of frames [first, first + n) at `points` = [(mx, my)] window positions (at most
        MAX_PROBES) through the viewport of `options` (a RenderOptions), on `stream` (smhv_batch_probe): no pixels.  Asynchronous;
        read_probes() waits for it."""
        from .render import probe_points
        n = self.max_frames - first if n is None else n
        pts = probe_points([(float(x), float(y)) for x, y in points])
        L.check(self._lib.smhv_batch_probe(self._b, first, n, C.byref(options), pts if len(points) else None, len(points), stream))

    def read_probes(self, first=0, n=None):
        """Synchronising host copy of the probe slab -> a ctypes array of n * MAX_PROBES Probe (frame f's at [f * MAX_PROBES])."""
        return self._read_slab(self._lib.smhv_batch_read_probes, L.Probe, first, n, L.MAX_PROBES)

    def probes_ptr(self):
        """Device address of the probe slab (MAX_PROBES smhv_probe per frame)."""
        return self._slab_ptr(self._lib.smhv_batch_probes_ptr)

    def render_debug(self, options, debug, first=0, n=None, stream=None):
        """Draw the debug text and the vision debugger onto the images of the most recent render over frames [first, first + n) on
        `stream` (smhv_batch_render_debug), behind the render and the labels, and write the probe slab.  options: the
        RenderOptions of that render; debug: a DebugOptions.  Asynchronous."""
        n = self.max_frames - first if n is None else n
        do, keep = debug.struct()
        L.check(self._lib.smhv_batch_render_debug(self._b, first, n, C.byref(options), C.byref(do), stream))
        del keep

    def feed(self, feed, first=0, n=None, snapshot=False, stream=0, map_source=L.VIEW_NONE):
        """The web server's events of frames [first, first + n) into `feed` (a WebFeed) on `stream` (smhv_batch_feed):
        UpdateState, Map when the ui_map's CRC-32 differs from the one the feed last sent, Markers -- or, with snapshot, what a
        client that has just connected gets.  map_source: a VIEW_* of _lib -- that debug view is hashed and sent as the Map in
        the ui_map's place (smhv_batch_feed_view).  Asynchronous; feed.read() waits for it."""
        n = self.max_frames - first if n is None else n
        flags = L.FEED_SNAPSHOT if snapshot else 0
        if map_source == L.VIEW_NONE:
            L.check(self._lib.smhv_batch_feed(self._b, feed._f, first, n, flags, C.c_void_p(stream)))
        else:
            L.check(self._lib.smhv_batch_feed_view(self._b, feed._f, first, n, flags, int(map_source), C.c_void_p(stream)))

    def feed_tiles(self, feed, first=0, n=None, stream=0):
        """feed() with map tiles (smhv_batch_feed_tiles): a frame whose ui_map differs from the map before it in a few 64 x 16
        tiles sends a MapTiles message (web.decode_map_tiles, web.MapTexture) in the Map's place.  The ui_map only, no snapshot.
        Asynchronous; feed.read() waits for it."""
        n = self.max_frames - first if n is None else n
        L.check(self._lib.smhv_batch_feed_tiles(self._b, feed._f, first, n, 0, C.c_void_p(stream)))

    def video(self, source, pixels, first=0, n=None, out_ptr=None, layout=None, stream=None):
        """Frames [first, first + n) of what the batch shows a viewer as NV12 / I420 video frames on `stream` (smhv_batch_video).
        source: "render" (the render slab at the most recent render's window size) or "ui_map" (the ui_map at the ROI's size; a grey
        one is read from its luma plane, no RGBA is made).  pixels: yuv.pixels(...) with nearest chroma; layout: None (tight), a
        yuv.yuv_layout(...) or a dict of its members.  out_ptr None: a torch uint8 tensor [n, yuv.video_bytes(w, h, pixels)] of tight
        frames is allocated and returned after the device has finished; otherwise asynchronous, returns None."""
        from . import yuv
        n = self.max_frames - first if n is None else n
        src = {"render": L.VIDEO_RENDER, "ui_map": L.VIDEO_UI_MAP}[source]
        if isinstance(layout, dict):
            layout = yuv.yuv_layout(**layout)
        out = None
        if out_ptr is None:
            import torch
            w, h = self.render_size() if source == "render" else self.roi[2:]
            out = yuv._video_out(n, w, h, pixels)
            out_ptr, layout = out.data_ptr(), None
        L.check(self._lib.smhv_batch_video(self._b, src, first, n, int(pixels), C.c_void_p(int(out_ptr)), C.byref(layout) if layout is not None else None,
                                           C.c_void_p(int(stream)) if stream else None))
        if out is not None:
            torch.cuda.synchronize()
        return out

    def read_image(self, which, frame):
        x, y, w, h = self.roi
        if which in (L.IMAGE_UI_MAP, L.IMAGE_HEIGHTMAP_OVERLAY):
            out = np.empty((h, w, 4), np.uint8)
        elif which == L.VIEW_LSD_INPUT:
            out = np.empty((h, w), np.uint8)
        else:
            out = np.empty((h // 2, w // 2), np.uint8)
        L.check(self._lib.smhv_batch_read_image(self._b, which, frame, out.ctypes.data))
        return out


class Pipeline:
    """`depth` batches in flight on library-owned streams (smhv_pipeline_*): submit() is asynchronous and returns the slot;
    the library owns every stream of the schedule and picks the line-search schedule: batch-granular below depth 6; from
    depth 6 on it holds both and measures which one the workload runs faster on (SMHV_SEARCH_AUTO)."""

    def __init__(self, vision, frame_w, frame_h, max_frames, depth=4, search=None, **options):
        """search: None / "auto" (batch-granular below depth 6, measured from there on), "batch", "frame";
        options: the other fields of smhv_pipeline_options (streams, idle_close_us, occupancy_policy, late_helpers,
        service_workgroups, flags, remote_after, remote_tickets, remote_last, room_for_others)."""
        self._lib = L.load()
        self._vision = vision
        p = C.c_void_p()
        opt = L.PipelineOptions()
        opt.size = C.sizeof(L.PipelineOptions)
        opt.search = {None: L.SEARCH_AUTO, "auto": L.SEARCH_AUTO, "batch": L.SEARCH_BATCH, "frame": L.SEARCH_FRAME}[search]
        for k, v in options.items():
            if k not in ("streams", "idle_close_us", "occupancy_policy", "late_helpers", "service_workgroups", "flags", "remote_after", "remote_tickets", "remote_last", "room_for_others"):
                raise TypeError("Pipeline: unknown option %r" % k)
            setattr(opt, k, int(v))
        L.check(self._lib.smhv_pipeline_create_ex(vision._ctx, frame_w, frame_h, max_frames, depth, C.byref(opt), C.byref(p)))
        self._p = p
        self.depth = depth
        self.slots = []
        for i in range(depth):
            b = C.c_void_p()
            L.check(self._lib.smhv_pipeline_slot(self._p, i, C.byref(b), None))
            self.slots.append(FrameBatch(vision, frame_w, frame_h, max_frames, _handle=b))

    def stream_of(self, slot):
        """A HIP stream to order a consumer of the slot's outputs on (batch-granular search: the stream its record kernel ran
        on; frame-granular search: the call waits for the slot's submission on the host first)."""
        st = C.c_void_p()
        L.check(self._lib.smhv_pipeline_slot(self._p, slot, None, C.byref(st)))
        return st.value or 0

    def hold(self, slot, stream):
        """The slot's outputs are read by work already enqueued on `stream`: its next submission waits for that."""
        L.check(self._lib.smhv_pipeline_hold(self._p, slot, C.c_void_p(stream)))

    def submit(self, frames_ptr, n, stages=L.STAGE_ALL, grayscale=True, max_gap=15, anchors=None, after_stream=0):
        if anchors is not None and len(anchors) < n:
            raise ValueError("anchors holds %d entries, the submission covers %d frames" % (len(anchors), n))
        a = C.cast(anchors, C.c_void_p) if anchors is not None else None
        slot = C.c_uint32(0)
        L.check(self._lib.smhv_pipeline_submit(self._p, C.c_void_p(frames_ptr), n, stages, int(bool(grayscale)), max_gap, a, C.c_void_p(after_stream), C.byref(slot)))
        return int(slot.value)

    def set_firing(self, heightmap=None, fit_to_minimap=True, viewport=None):
        """Bind a Heightmap (None = none) and the options for STAGE_FIRING submissions made after this call
        (smhv_pipeline_set_firing); submissions in flight keep what they were submitted with."""
        opt = L.firing_options(fit_to_minimap, viewport)
        L.check(self._lib.smhv_pipeline_set_firing(self._p, L._hm(heightmap), C.byref(opt)))

    def search_stats(self):
        """Diagnostic (synchronises): the frame-granular line search of a pipeline of depth >= 3 -> dict, or None."""
        out = (C.c_uint64 * 32)()
        L.check(self._lib.smhv_debug_pipeline_stats(self._p, out))
        if not out[0]:
            return None
        keys = ("launches", "frames", "waves", "busy_cycles", "resident_cycles", "waves_per_launch", "submissions")
        d = dict(zip(keys, [int(v) for v in out[1:8]]))
        d["cycles_per_frame_by_phase"] = dict(zip(("acquire", "search", "record", "release"), [int(v) / max(d["frames"], 1) for v in out[8:12]]))
        d["help_cycles_per_frame"] = int(out[12]) / max(d["frames"], 1)
        d["remote_help"] = {"requests": int(out[16]), "helpers_attached": int(out[17]), "candidates_cast": int(out[18]), "tickets_left": int(out[19]) - (1 << 64) if int(out[19]) >= (1 << 63) else int(out[19])}
        d["cycles_per_frame"] = d["busy_cycles"] / max(d["frames"], 1)
        d["busy_fraction"] = d["busy_cycles"] / max(d["resident_cycles"], 1)
        # where a submission's time goes (100 MHz ticks -> ms): publication -> a wave takes the frame (mean over frames); publication ->
        # last frame counted off (mean over submissions); how long that last frame was at work
        d["remote_help"].update({"polls": int(out[23]), "polls_empty": int(out[24]), "claims_lost": int(out[25]), "exits_idle": int(out[26]), "exits_closed": int(out[27]),
                                 "cycles_attached_per_helper": int(out[28]) / max(int(out[17]), 1), "cast_fraction_of_attached": int(out[29]) / max(int(out[28]), 1)})
        d["timeline_ms"] = {"frame_wait": int(out[20]) / max(d["frames"], 1) / 1e5, "submission_search": int(out[21]) / max(d["submissions"], 1) / 1e5,
                            "last_frame_at_work": int(out[22]) / max(d["submissions"], 1) / 1e5}
        # SMHV_SEARCH_AUTO at depth >= 6: the pipeline times both searches on the workload it is given and keeps the faster
        d["adaptive"] = bool(int(out[13]) & 2)
        d["settled"] = bool(int(out[13]) & 4) or not d["adaptive"]
        d["mode"] = "frame-granular" if int(out[13]) & 1 else "batch-granular"
        d["measured_frames_per_s"] = {"frame-granular": int(out[14]), "batch-granular": int(out[15])}
        return d

    def peek(self):
        """Diagnostic, no device-wide synchronisation: the search service's life-cycle words and ring counters."""
        out = (C.c_uint64 * 16)()
        L.check(self._lib.smhv_debug_pipeline_peek(self._p, out))
        keys = ("submissions", "alive_epoch", "launches", "last_seq", "avail", "head", "reserved", "closing_epoch", "completed", "busy")
        d = dict(zip(keys, [int(v) for v in out[:10]]))
        d["avail"] = d["avail"] - (1 << 64) if d["avail"] >= (1 << 63) else d["avail"]
        d["slots"] = [(int(v) >> 32, int(v) & 0xFFFFFFFF) for v in out[10:14]]
        d["service_workgroups"], d["waves_per_workgroup"] = int(out[14]) >> 32, int(out[14]) & 0xFFFFFFFF
        d["lds_words_per_wave"], d["lds_bytes_dynamic"] = int(out[15]) >> 32, int(out[15]) & 0xFFFFFFFF
        return d

    def wait(self, slot=None):
        if slot is None:
            L.check(self._lib.smhv_pipeline_wait_all(self._p))
        else:
            L.check(self._lib.smhv_pipeline_wait(self._p, slot))

    def close(self):
        if self._p:
            for b in self.slots:
                b.close()
            self._lib.smhv_pipeline_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
