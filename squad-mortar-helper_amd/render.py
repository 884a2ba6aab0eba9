"""The map view (smhv_batch_render / smhv_render_map): the viewport the app's window shows the map through, and the options of a
render call.  MapViewport is the app's own (src/ui/map.rs:14-126): calc letter-boxes the map into the window, zooms and pans;
the same object feeds the firing solutions (firing_viewport), so the numbers and the picture use one viewport."""
import ctypes as C

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
