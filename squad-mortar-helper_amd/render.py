"""The map view (smhv_batch_render / smhv_render_map): the viewport the app's window shows the map through, and the options of a
render call.  MapViewport is the app's own (src/ui/map.rs:14-126): calc letter-boxes the map into the window, zooms and pans;
the same object feeds the firing solutions (firing_viewport), so the numbers and the picture use one viewport."""
import ctypes as C
import math

import numpy as np

from . import _lib as L


class MapViewport:
    """MapViewport (src/ui/map.rs:14-18) and the quad MapViewport::calc returns with it; every field a C float's value."""

    def __init__(self, quad=(0.0, 0.0, 0.0, 0.0), scale=(1.0, 1.0), top_left=(0.0, 0.0)):
        self.quad = tuple(float(v) for v in quad)                 # (left, top, right, bottom)
        self.scale_factor_w, self.scale_factor_h = (float(v) for v in scale)
        self.top_left = tuple(float(v) for v in top_left)

    @classmethod
    def calc(cls, region_w, region_h, map_w, map_h, zoom=0, zoom_pos=(0.0, 0.0), pan_pos=(0.0, 0.0)):
        """MapViewport::calc (map.rs:21-77) by the library's f32 restatement (smhv_map_viewport_calc; needs no device)."""
        opt = L.RenderOptions()
        zp, pp = (C.c_float * 2)(*zoom_pos), (C.c_float * 2)(*pan_pos)
        L.check(L.load().smhv_map_viewport_calc(region_w, region_h, map_w, map_h, int(zoom), zp, pp, C.byref(opt)))
        return cls(tuple(opt.quad), tuple(opt.viewport_scale), tuple(opt.viewport_top_left))

    @classmethod
    def identity(cls, map_w, map_h):
        """The window that is exactly the map: the render is the ui_map (with the heightmap: the overlay stage's image)."""
        return cls((0.0, 0.0, float(map_w), float(map_h)), (1.0, 1.0), (0.0, 0.0))

    def translate_xy(self, xy):
        """Map-ROI coordinates -> window coordinates (map.rs:79-101), f32."""
        f = C.c_float
        return (f(f(f(xy[0]).value * f(self.scale_factor_w).value).value + f(self.top_left[0]).value).value,
                f(f(f(xy[1]).value * f(self.scale_factor_h).value).value + f(self.top_left[1]).value).value)

    def inverse_xy(self, xy):
        """Window coordinates -> map-ROI coordinates (map.rs:103-125), f32."""
        f = C.c_float
        return (f(f(f(xy[0]).value - f(self.top_left[0]).value).value / f(self.scale_factor_w).value).value,
                f(f(f(xy[1]).value - f(self.top_left[1]).value).value / f(self.scale_factor_h).value).value)

    def firing_viewport(self):
        """What FrameBatch.set_firing / Pipeline.set_firing / HipVision.firing_solutions take as `viewport`."""
        return (self.scale_factor_w, self.scale_factor_h, self.top_left[0], self.top_left[1])


def render_options(viewport, out_w, out_h, heightmap=False, markers=False, fit_to_minimap=True, background=(0, 0, 0, 255)):
    """smhv_render_options for a window of out_w x out_h seen through `viewport` (a MapViewport)."""
    o = L.RenderOptions()
    o.size = C.sizeof(L.RenderOptions)
    o.flags = (L.RENDER_HEIGHTMAP if heightmap else 0) | (L.RENDER_MARKERS if markers else 0) | (0 if fit_to_minimap else L.RENDER_BOUNDS_OFFSET)
    o.out_w, o.out_h = int(out_w), int(out_h)
    for i in range(4):
        o.quad[i] = viewport.quad[i]
        o.background[i] = int(background[i])
    o.viewport_scale[0], o.viewport_scale[1] = viewport.scale_factor_w, viewport.scale_factor_h
    o.viewport_top_left[0], o.viewport_top_left[1] = viewport.top_left
    return o


RenderOptions = L.RenderOptions

# ---- layers (smhv_batch_render_layers / smhv_render_map_layers): what the window shows beside the map view ----------------
CUSTOM_MARKER_COLOR = (255, 0, 255, 255)                          # [1, 0, 1] (src/ui/draw.rs), also the scale bars' (debug.rs:317)
MEASURE_MARKER_COLOR = (255, 0, 0, 255)                           # [1, 0, 0]
_f32 = np.float32


def prim(x0, y0, x1, y1, rgba, kind):
    """One smhv_render_prim as a tuple (x0, y0, x1, y1, (r, g, b, a), kind): map-ROI coordinates as C floats' values."""
    return (float(_f32(x0)), float(_f32(y0)), float(_f32(x1)), float(_f32(y1)), tuple(int(v) for v in rgba), int(kind))


def _long_enough(a, b, threshold):
    """is_line_long_enough (draw.rs:34-36) in f32: sum((a - b)^2) >= threshold^2."""
    d0, d1 = _f32(a[0]) - _f32(b[0]), _f32(a[1]) - _f32(b[1])
    t = _f32(threshold)
    return bool(_f32(d0 * d0) + _f32(d1 * d1) >= t * t)


def ctl_marker_prims(custom, drag=None, measure=None, drag_threshold=6.0):
    """draw::render (draw.rs:135-198) as prims painted BELOW the detected markers: every custom marker ((x0, y0), (x1, y1)) in
    magenta; `drag` = (start, mouse) in magenta and `measure` = (start, mouse) in red, each only when it is at least
    `drag_threshold` long (imgui's mouse_drag_threshold, 6 by default).  Map-ROI coordinates."""
    out = [prim(p0[0], p0[1], p1[0], p1[1], CUSTOM_MARKER_COLOR, L.PRIM_LINE) for p0, p1 in custom]
    for pair, color in ((drag, CUSTOM_MARKER_COLOR), (measure, MEASURE_MARKER_COLOR)):
        if pair is not None and _long_enough(pair[0], pair[1], drag_threshold):
            out.append(prim(pair[0][0], pair[0][1], pair[1][0], pair[1][1], color, L.PRIM_LINE))
    return out


def _color_byte(v):
    v = _f32(v)
    v = _f32(0.0) if not v > 0 else (_f32(1.0) if v > 1 else v)   # clamp01 (a NaN is 0)
    return int(np.uint8(v * _f32(255.0) + _f32(0.5)))


def ocr_box_prims(boxes, brq_w, brq_h):
    """The Debug menu's OCR overlay (debug.rs:290-303): boxes = [(left, top, right, bottom, confidence)] in the bottom right
    quadrant's pixels, moved by (brq_w, brq_h) into map-ROI coordinates as src/vision/mod.rs:154-157 does; 1 px outlines above
    everything, coloured [1 - c/100, c/100, 0]."""
    out = []
    for left, top, right, bottom, conf in boxes:
        f = _f32(conf) / _f32(100.0)
        color = (_color_byte(_f32(1.0) - f), _color_byte(f), 0, 255)
        out.append(prim(int(left) + int(brq_w), int(top) + int(brq_h), int(right) + int(brq_w), int(bottom) + int(brq_h), color,
                        L.PRIM_RECT | L.PRIM_FOREGROUND))
    return out


def scale_label_prims(labels, brq_w, brq_h, confidence=100.0):
    """The boxes of the scale labels the device found (ScaleLabel records) as the OCR overlay draws its hits: ocr_box_prims on
    (left, top, right, bottom, confidence).  The device reads no glyphs, so the confidence -- the colour -- is the caller's."""
    return ocr_box_prims([(lb.left, lb.top, lb.right, lb.bottom, confidence) for lb in labels], brq_w, brq_h)


def scale_bar_prims(bars, brq_w, brq_h):
    """The Debug menu's scale overlay (debug.rs:306-320): bars = [(left, y, right, found)] as calc_meters_to_px_ratio(...,
    want_bars=True) returns them, moved by (brq_w, brq_h) (mod.rs:205-210); 2 px magenta lines above everything.  Bars that
    were not found are skipped."""
    return [prim(int(left) + int(brq_w), int(y) + int(brq_h), int(right) + int(brq_w), int(y) + int(brq_h), CUSTOM_MARKER_COLOR,
                 L.PRIM_LINE | L.PRIM_FOREGROUND) for left, y, right, found in bars if found]


class RenderLayers:
    """What a render call with layers draws beside the map view: prims (tuples of prim(), or an iterable of them from the
    builders above), the records' minimap bounds, and a debug view (a VIEW_* of _lib) as the map quad's texture."""

    def __init__(self, prims=(), minimap_bounds=False, map_source=0):
        self.prims = list(prims)
        self.minimap_bounds = bool(minimap_bounds)
        self.map_source = int(map_source)

    def struct(self):
        """-> (smhv_render_layers, the array it points to: keep it alive for the call)."""
        n = len(self.prims)
        arr = (L.RenderPrim * max(n, 1))()
        for i, (x0, y0, x1, y1, rgba, kind) in enumerate(self.prims):
            arr[i].x0, arr[i].y0, arr[i].x1, arr[i].y1 = x0, y0, x1, y1
            for k in range(4):
                arr[i].rgba[k] = rgba[k]
            arr[i].kind = kind
        ly = L.RenderLayersStruct()
        ly.size = C.sizeof(L.RenderLayersStruct)
        ly.flags = L.LAYER_MINIMAP_BOUNDS if self.minimap_bounds else 0
        ly.map_source = self.map_source
        ly.n_prims = n
        ly.prims = C.cast(arr, C.POINTER(L.RenderPrim)) if n else None
        return ly, arr


# ---- labels (smhv_batch_render_labels / smhv_render_map_labeled): the firing solution of a line as text beside it -------------
def label_lines(custom, drag=None, measure=None, drag_threshold=6.0):
    """The label side of ctl_marker_prims: the lines draw::render (draw.rs:135-198) hands to markers::draw, as ((x0, y0, x1, y1),
    rgba) in its order -- every custom marker in magenta, `drag` in magenta and `measure` in red, each only when it is at least
    `drag_threshold` long (is_line_long_enough).  Map-ROI coordinates."""
    out = [((float(_f32(p0[0])), float(_f32(p0[1])), float(_f32(p1[0])), float(_f32(p1[1]))), CUSTOM_MARKER_COLOR) for p0, p1 in custom]
    for pair, color in ((drag, CUSTOM_MARKER_COLOR), (measure, MEASURE_MARKER_COLOR)):
        if pair is not None and _long_enough(pair[0], pair[1], drag_threshold):
            out.append(((float(_f32(pair[0][0])), float(_f32(pair[0][1])), float(_f32(pair[1][0])), float(_f32(pair[1][1]))), color))
    return out


class LabelOptions:
    """What a label call draws: `extra` = [((x0, y0, x1, y1), rgba)] (label_lines()), detected = the detected lines too, scale =
    window pixels per font unit (1 .. 4, 0 = 2), mpx = the per-call path's meters per pixel (a batch takes its records')."""

    def __init__(self, extra=(), detected=True, scale=0, mpx=None):
        self.extra = list(extra)
        self.detected = bool(detected)
        self.scale = int(scale)
        self.mpx = mpx

    def struct(self):
        """-> (smhv_label_options, what it points to: keep it alive for the call)."""
        n = len(self.extra)
        arr = (L.LabelLine * max(n, 1))()
        for i, (line, rgba) in enumerate(self.extra):
            arr[i].line.x0, arr[i].line.y0, arr[i].line.x1, arr[i].line.y1 = line
            for k in range(4):
                arr[i].rgba[k] = rgba[k]
        mpx = C.c_double(self.mpx) if self.mpx is not None else None
        o = L.LabelOptionsStruct()
        o.size = C.sizeof(L.LabelOptionsStruct)
        o.flags = L.LABEL_DETECTED if self.detected else 0
        o.scale = self.scale
        o.n_extra = n
        o.extra = C.cast(arr, C.POINTER(L.LabelLine)) if n else None
        o.mpx = C.pointer(mpx) if mpx is not None else None
        return o, (arr, mpx)


# ---- reach map (smhv_batch_reach / smhv_reach_map): the firing solution from an origin to every window pixel ---------------------
class ReachOptions:
    """What a reach call computes: origin = (x, y) in map-ROI coordinates, or ("p0", i) / ("p1", i): that end of each frame's line i
    (a batch only); ring_m = metres between range rings (0: none); paint / classes = tint the render slab / write the class bytes;
    palette = None (the library's, smhv_reach_defaults) or dict(out_of_range=rgba, band=[8 rgba], ring=rgba), a = the blend weight."""

    def __init__(self, origin=(0.0, 0.0), ring_m=0.0, paint=True, classes=False, palette=None):
        self.origin = origin
        self.ring_m = float(ring_m)
        self.paint = bool(paint)
        self.classes = bool(classes)
        self.palette = palette

    def struct(self):
        """-> smhv_reach_options."""
        o = L.ReachOptionsStruct()
        L.check(L.load().smhv_reach_defaults(C.byref(o)))
        o.flags = (L.REACH_PAINT if self.paint else 0) | (L.REACH_CLASSES if self.classes else 0)
        if isinstance(self.origin[0], str):
            o.origin_mode = {"p0": L.REACH_ORIGIN_LINE_P0, "p1": L.REACH_ORIGIN_LINE_P1}[self.origin[0]]
            o.line = int(self.origin[1])
        else:
            o.origin_mode = L.REACH_ORIGIN_POINT
            o.origin[0], o.origin[1] = float(self.origin[0]), float(self.origin[1])
        o.ring_m = self.ring_m
        if self.palette is not None:
            for k in range(4):
                o.out_of_range[k] = int(self.palette["out_of_range"][k])
                o.ring[k] = int(self.palette["ring"][k])
                for j in range(8):
                    o.band[j][k] = int(self.palette["band"][j][k])
        return o


def reach_thresholds():
    """The seven tan(mils * pi / 3200), mils = 900 .. 1500, that split the in-range classes (smhv_reach_thresholds; host only)."""
    out = (C.c_double * 7)()
    L.check(L.load().smhv_reach_thresholds(out))
    return [float(v) for v in out]


# ---- ballistics (smhv_batch_ballistic_map / smhv_ballistic_map): a caller-supplied weapon's reach map ------------------------------
class BallisticOptions:
    """What a ballistic-map call computes: origin as ReachOptions takes it; iso_s = seconds between isochrones (0: none); paint /
    classes / tof = tint the render slab / write the class bytes / write the f32 time-of-flight plane; palette = None (the
    library's, smhv_ballistic_defaults) or dict(pal=[12 rgba, classes 1 .. 12], iso=rgba), a = the blend weight."""

    def __init__(self, origin=(0.0, 0.0), iso_s=0.0, paint=True, classes=False, tof=False, palette=None):
        self.origin = origin
        self.iso_s = float(iso_s)
        self.paint = bool(paint)
        self.classes = bool(classes)
        self.tof = bool(tof)
        self.palette = palette

    def struct(self):
        """-> smhv_ballistic_options."""
        o = L.BallisticOptionsStruct()
        L.check(L.load().smhv_ballistic_defaults(C.byref(o)))
        o.flags = (L.BMAP_PAINT if self.paint else 0) | (L.BMAP_CLASSES if self.classes else 0) | (L.BMAP_TOF if self.tof else 0)
        if isinstance(self.origin[0], str):
            o.origin_mode = {"p0": L.REACH_ORIGIN_LINE_P0, "p1": L.REACH_ORIGIN_LINE_P1}[self.origin[0]]
            o.line = int(self.origin[1])
        else:
            o.origin_mode = L.REACH_ORIGIN_POINT
            o.origin[0], o.origin[1] = float(self.origin[0]), float(self.origin[1])
        o.iso_s = self.iso_s
        if self.palette is not None:
            for k in range(4):
                o.iso[k] = int(self.palette["iso"][k])
                for j in range(12):
                    o.pal[j][k] = int(self.palette["pal"][j][k])
        return o


# ---- ballistic clearance (smhv_batch_ballistic_clearance / _lines / smhv_batch_ballistic_clearance_map / smhv_ballistic_clearance_map)
class BallisticClearanceOptions:
    """What a ballistic-clearance call computes: samples = S (1 .. 256); margin_m = metres an arc must keep over the terrain.  The map
    only: origin as ReachOptions takes it; paint / bytes / margin = tint the render slab / write the class bytes / write the f32 plane of
    the own arc's least margin; palette = None (the library's, smhv_ballistic_clearance_defaults) or dict(pal=[4 rgba: out of range,
    unusable, clear, blocked], switch_arc=rgba, los=rgba), a = the blend weight."""

    def __init__(self, samples=64, margin_m=0.0, origin=(0.0, 0.0), paint=True, bytes=False, margin=False, palette=None):
        self.samples = int(samples)
        self.margin_m = float(margin_m)
        self.origin = origin
        self.paint = bool(paint)
        self.bytes = bool(bytes)
        self.margin = bool(margin)
        self.palette = palette

    def struct(self):
        """-> smhv_ballistic_clearance_options."""
        o = L.BallisticClearanceOptionsStruct()
        L.check(L.load().smhv_ballistic_clearance_defaults(C.byref(o)))
        o.flags = (L.BCLR_PAINT if self.paint else 0) | (L.BCLR_BYTES if self.bytes else 0) | (L.BCLR_MARGIN if self.margin else 0)
        o.samples = self.samples
        o.margin_m = self.margin_m
        if isinstance(self.origin[0], str):
            o.origin_mode = {"p0": L.REACH_ORIGIN_LINE_P0, "p1": L.REACH_ORIGIN_LINE_P1}[self.origin[0]]
            o.line = int(self.origin[1])
        else:
            o.origin_mode = L.REACH_ORIGIN_POINT
            o.origin[0], o.origin[1] = float(self.origin[0]), float(self.origin[1])
        if self.palette is not None:
            for k in range(4):
                o.switch_arc[k] = int(self.palette["switch_arc"][k])
                o.los[k] = int(self.palette["los"][k])
                for j in range(4):
                    o.pal[j][k] = int(self.palette["pal"][j][k])
        return o


# ---- terrain clearance (smhv_batch_clearance / smhv_clearance_lines / smhv_batch_clearance_map / smhv_clearance_map) ------------------
class ClearanceOptions:
    """What a clearance call computes: samples = S, how many steps the line of fire is cut into (1 .. 256); margin_m = metres the arc
    must keep over the terrain.  The map only: origin = (x, y) in map-ROI coordinates, or ("p0", i) / ("p1", i): that end of each
    frame's line i (a batch only); paint / bytes = tint the render slab / write the status bytes; palette = None (the library's,
    smhv_clearance_defaults) or dict(out_of_range=rgba, clear=rgba, blocked=rgba, los=rgba), a = the blend weight."""

    def __init__(self, samples=64, margin_m=0.0, origin=(0.0, 0.0), paint=True, bytes=False, palette=None):
        self.samples = int(samples)
        self.margin_m = float(margin_m)
        self.origin = origin
        self.paint = bool(paint)
        self.bytes = bool(bytes)
        self.palette = palette

    def struct(self):
        """-> smhv_clearance_options."""
        o = L.ClearanceOptionsStruct()
        L.check(L.load().smhv_clearance_defaults(C.byref(o)))
        o.flags = (L.CLEAR_PAINT if self.paint else 0) | (L.CLEAR_BYTES if self.bytes else 0)
        o.samples = self.samples
        o.margin_m = self.margin_m
        if isinstance(self.origin[0], str):
            o.origin_mode = {"p0": L.REACH_ORIGIN_LINE_P0, "p1": L.REACH_ORIGIN_LINE_P1}[self.origin[0]]
            o.line = int(self.origin[1])
        else:
            o.origin_mode = L.REACH_ORIGIN_POINT
            o.origin[0], o.origin[1] = float(self.origin[0]), float(self.origin[1])
        if self.palette is not None:
            for k in range(4):
                for name in ("out_of_range", "clear", "blocked", "los"):
                    getattr(o, name)[k] = int(self.palette[name][k])
        return o


# ---- terrain relief (smhv_batch_relief / smhv_relief_map): contour lines, hillshade and heights of every window pixel ---------------
def relief_light(azimuth_deg=315.0, altitude_deg=45.0):
    """The unit vector from the ground towards a light at compass azimuth (0 = north = up on the map, 90 = east) and altitude above
    the horizon, in heightmap axes (x right, y down, z up) -> (lx, ly, lz).  A host convenience: the library takes the vector."""
    az, alt = math.radians(float(azimuth_deg)), math.radians(float(altitude_deg))
    return (math.sin(az) * math.cos(alt), -math.cos(az) * math.cos(alt), math.sin(alt))


class ReliefOptions:
    """What a relief call computes: interval_m = metres between contour levels (0: none), base_m = the height of level 0, major_every
    = every M-th level is an index contour (0: none); exaggeration, light = the hillshade's slope factor and its vector towards the
    light (relief_light()); nearest = the nearest texel's height, not the bilinear one; paint / bytes / shades / heights = tint the
    render slab / write that plane; contour, major = rgba with a = the blend weight, shade_weight = the hillshade's (None: the
    library's, smhv_relief_defaults)."""

    def __init__(self, interval_m=None, base_m=None, major_every=None, exaggeration=None, light=None, nearest=False, paint=True, bytes=False,
                 shades=False, heights=False, contour=None, major=None, shade_weight=None):
        self.interval_m, self.base_m, self.major_every, self.exaggeration, self.light = interval_m, base_m, major_every, exaggeration, light
        self.nearest, self.paint, self.bytes, self.shades, self.heights = bool(nearest), bool(paint), bool(bytes), bool(shades), bool(heights)
        self.contour, self.major, self.shade_weight = contour, major, shade_weight

    def struct(self):
        """-> smhv_relief_options."""
        o = L.ReliefOptionsStruct()
        L.check(L.load().smhv_relief_defaults(C.byref(o)))
        o.flags = ((L.RELIEF_PAINT if self.paint else 0) | (L.RELIEF_BYTES if self.bytes else 0) | (L.RELIEF_SHADES if self.shades else 0) |
                   (L.RELIEF_HEIGHTS if self.heights else 0) | (L.RELIEF_NEAREST if self.nearest else 0))
        for name in ("interval_m", "base_m", "exaggeration"):
            if getattr(self, name) is not None:
                setattr(o, name, float(getattr(self, name)))
        if self.major_every is not None:
            o.major_every = int(self.major_every)
        if self.shade_weight is not None:
            o.shade_weight = int(self.shade_weight)
        if self.light is not None:
            for k in range(3):
                o.light[k] = float(self.light[k])
        for name in ("contour", "major"):
            if getattr(self, name) is not None:
                for k in range(4):
                    getattr(o, name)[k] = int(getattr(self, name)[k])
        return o


# ---- map grid (smhv_batch_grid / smhv_grid_map / smhv_batch_grid_refs / smhv_grid_refs): grid lines, cell labels, keypad references --------
class GridOptions:
    """What a grid call computes: cell_m = the side of a cell in metres, levels = keypad levels below the cell (0 .. 3), origin_m =
    metres from the map's top-left corner to the corner of A1; min_px = a level is drawn when its cells are at least this many
    pixels wide and high, label_min_px = the labels when the cells are; paint / bytes / cells = draw into the render slab / write that
    plane; line = four rgba (major, keypad, sub-keypad, sub-sub-keypad) and label = one, a = the blend weight (None: the library's,
    smhv_grid_defaults)."""

    def __init__(self, cell_m=None, levels=None, origin_m=None, min_px=None, label_min_px=None, paint=True, bytes=False, cells=False, line=None,
                 label=None):
        self.cell_m, self.levels, self.origin_m, self.min_px, self.label_min_px = cell_m, levels, origin_m, min_px, label_min_px
        self.paint, self.bytes, self.cells = bool(paint), bool(bytes), bool(cells)
        self.line, self.label = line, label

    def struct(self):
        """-> smhv_grid_options."""
        o = L.GridOptionsStruct()
        L.check(L.load().smhv_grid_defaults(C.byref(o)))
        o.flags = (L.GRID_PAINT if self.paint else 0) | (L.GRID_BYTES if self.bytes else 0) | (L.GRID_CELLS if self.cells else 0)
        for name in ("cell_m", "min_px", "label_min_px"):
            if getattr(self, name) is not None:
                setattr(o, name, float(getattr(self, name)))
        if self.levels is not None:
            o.levels = int(self.levels)
        if self.origin_m is not None:
            o.origin_m[0], o.origin_m[1] = float(self.origin_m[0]), float(self.origin_m[1])
        if self.line is not None:
            for k in range(4):
                for j in range(4):
                    o.line[k][j] = int(self.line[k][j])
        if self.label is not None:
            for j in range(4):
                o.label[j] = int(self.label[j])
        return o


def grid_ref_text(col, row1, digits=()):
    """The text of a grid reference (smhv_grid_ref_text): column 0 = A, row1 from 1, digits = the keypad digits of levels 1 .. ->
    "B4-7-3"."""
    d = (C.c_uint8 * 3)(*[int(v) for v in digits])
    out = C.create_string_buffer(16)
    L.check(L.load().smhv_grid_ref_text(int(col), int(row1), d, len(digits), out))
    return out.raw.rstrip(b"\0").decode("ascii")


# ---- debug text and the vision debugger (smhv_batch_probe / smhv_batch_render_debug / smhv_render_map_debug) ------------------------
def text_run(x, y, text, rgba=(255, 255, 255, 255), map_coords=False):
    """One smhv_text_run as a tuple (x, y, (r, g, b, a), flags, bytes): `text` a str (encoded as Latin-1) or bytes, '\\n' starts a
    new line at the run's x; map_coords: (x, y) are map-ROI coordinates and go through the viewport, otherwise window pixels."""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    return (float(_f32(x)), float(_f32(y)), tuple(int(v) for v in rgba), L.TEXT_MAP_COORDS if map_coords else 0, data)


def _font_has(byte):
    return 0x20 <= byte <= 0x7E or byte in (0xB0, 0xB1)


def rust_debug_str(text):
    """Rust's {:?} of a str -- quotes around it, a backslash before '"' and a backslash, \\t \\r \\n as two characters, \\u{..} for
    what char::escape_debug escapes -- restricted to what the text font can print: None when a character that {:?} leaves as
    it is has no glyph (anything outside ASCII but the degree and plus-minus signs)."""
    out = ['"']
    for ch in text:
        o = ord(ch)
        if ch in '"\\':
            out.append("\\" + ch)
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\n":
            out.append("\\n")
        elif o == 0:
            out.append("\\0")
        elif o < 0x20 or 0x7F <= o < 0xA0:
            out.append("\\u{%x}" % o)                               # a control character: escape_debug's \u{..}
        elif o < 0x100 and _font_has(o):
            out.append(ch)
        else:
            return None
    out.append('"')
    return "".join(out)


def ocr_text_runs(boxes, brq_w, brq_h):
    """The text of the Debug menu's OCR overlay (debug.rs:300-301), beside ocr_box_prims: boxes = [(left, top, right, bottom,
    confidence, text)] in the bottom right quadrant's pixels; "{:.2}%\\n{:?}" at (left, bottom) moved by (brq_w, brq_h), in the box's
    colour.  ("%.2f" is Rust's {:.2}: both round the exact binary value.)  A run the font cannot print or that is longer than a
    run may be is skipped."""
    out = []
    for left, top, right, bottom, conf, text in boxes:
        f = _f32(conf) / _f32(100.0)
        color = (_color_byte(_f32(1.0) - f), _color_byte(f), 0, 255)
        dbg = rust_debug_str(text)
        if dbg is None:
            continue
        s = "%.2f%%\n" % float(_f32(conf)) + dbg                   # (the confidence is an f32, vision-ocr/src/lib.rs:111)
        if len(s) > L.TEXT_MAX_BYTES:
            continue
        out.append(text_run(int(left) + int(brq_w), int(bottom) + int(brq_h), s, color, map_coords=True))
    return out


def scale_text_runs(bars, brq_w, brq_h):
    """The text of the Debug menu's scale overlay (debug.rs:315), beside scale_bar_prims: bars = [(meters, left, y, right,
    found)]; "{meters}m" at the bar's p0 = (left, y) moved by (brq_w, brq_h), magenta.  Bars that were not found are skipped."""
    return [text_run(int(left) + int(brq_w), int(y) + int(brq_h), "%dm" % int(meters), CUSTOM_MARKER_COLOR, map_coords=True)
            for meters, left, y, right, found in bars if found]


def probe_points(points):
    """[(mx, my)] -> a ctypes array of smhv_probe_point (one entry at least, so it can always be passed)."""
    pts = (L.ProbePoint * max(len(points), 1))()
    for i, (x, y) in enumerate(points):
        pts[i].x, pts[i].y = x, y
    return pts


class DebugOptions:
    """What a debug pass draws: runs = [text_run()], probes = [(mx, my)] window positions of the vision debugger, draw_probes =
    the debugger's picture for every valid probe, minimap_caption = the red caption on frames without a minimap rectangle,
    scale = window pixels per font unit (1 .. 4, 0 = 2)."""

    def __init__(self, runs=(), probes=(), draw_probes=False, minimap_caption=False, scale=0):
        self.runs = list(runs)
        self.probes = [(float(_f32(x)), float(_f32(y))) for x, y in probes]
        self.draw_probes = bool(draw_probes)
        self.minimap_caption = bool(minimap_caption)
        self.scale = int(scale)

    def struct(self):
        """-> (smhv_debug_options, what it points to: keep it alive for the call)."""
        n, m = len(self.runs), len(self.probes)
        arr = (L.TextRun * max(n, 1))()
        for i, (x, y, rgba, flags, data) in enumerate(self.runs):
            arr[i].x, arr[i].y, arr[i].flags, arr[i].n = x, y, flags, len(data)
            for k in range(4):
                arr[i].rgba[k] = rgba[k]
            for k, b in enumerate(data[:L.TEXT_MAX_BYTES]):
                arr[i].text[k] = b
        pts = probe_points(self.probes)
        o = L.DebugOptionsStruct()
        o.size = C.sizeof(L.DebugOptionsStruct)
        o.flags = (L.DEBUG_DRAW_PROBES if self.draw_probes else 0) | (L.DEBUG_MINIMAP_CAPTION if self.minimap_caption else 0)
        o.scale = self.scale
        o.n_runs = n
        o.runs = C.cast(arr, C.POINTER(L.TextRun)) if n else None
        o.n_probes = m
        o.probes = C.cast(pts, C.POINTER(L.ProbePoint)) if m else None
        return o, (arr, pts)


def probe_text(probe):
    """The string the vision debugger prints for a Probe (smhv_probe_text; needs no device)."""
    buf = C.create_string_buffer(256)
    L.check(L.load().smhv_probe_text(C.byref(probe), buf, 256))
    return buf.value.decode("latin-1")
