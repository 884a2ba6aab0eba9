"""ctypes binding of libsmh_vision_hip.so (the C ABI declared in include/smh_vision_hip.h).

The product path has NO CPU fallback: if the shared library (and with it the gfx950 code object) is
missing, importing this module raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C squad-mortar-helper_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMH_VISION_HIP_LIB") or os.path.join(_HERE, "libsmh_vision_hip.so")   # env override: diagnostic builds only

MAX_LINES = 32
MAX_SCALES = 3

STAGE_MARKERS, STAGE_UI_MAP, STAGE_OCR, STAGE_SCALES, STAGE_ALL = 0x1, 0x2, 0x4, 0x8, 0xF
STAGE_MINIMAP = 0x10
STAGE_EXACT_STATS = 0x20
STAGE_LSD_HELPERS = 0x40
STAGE_FIRING = 0x80                        # firing solutions (needs STAGE_MARKERS; the heightmap branch needs STAGE_MINIMAP)
STAGE_HEIGHTMAP_OVERLAY = 0x100            # the heightmap's colours over the ui_map (needs STAGE_UI_MAP, STAGE_MINIMAP, a bound heightmap)
FIRING_BOUNDS_OFFSET = 1                   # smhv_firing_options.flags: the app's "fit to minimap" switched off
FIRING_NONE, FIRING_SCALES, FIRING_HEIGHTMAP = 0, 1, 2   # smhv_firing.source
VIEW_NONE, VIEW_OCR_INPUT, VIEW_FIND_SCALES_INPUT, VIEW_LSD_PREPROCESS, VIEW_LSD_INPUT, VIEW_CROPPED_BRQ = range(6)
IMAGE_UI_MAP = 100
IMAGE_HEIGHTMAP_OVERLAY = 101
RENDER_HEIGHTMAP, RENDER_MARKERS, RENDER_BOUNDS_OFFSET = 1, 2, 4   # smhv_render_options.flags
RENDER_MAX_LINES = 256                     # explicit lines of one smhv_render_map call
PRIM_LINE, PRIM_RECT, PRIM_FOREGROUND, PRIM_SHIFT1 = 0, 1, 0x100, 0x200   # smhv_render_prim.kind
RENDER_MAX_PRIMS = 256                     # prims of one render call with layers
LAYER_MINIMAP_BOUNDS = 1                   # smhv_render_layers.flags
RENDER_FORM_RULE, RENDER_FORM_GATHER, RENDER_FORM_STAGED, RENDER_FORM_TABLE = 0, 1, 2, 3   # smhv_debug_render_form

WEB_MAP, WEB_MARKERS, WEB_UPDATE_STATE, WEB_HEIGHTMAP, WEB_FIT_TO_MINIMAP = 1, 2, 3, 4, 5   # the web server's event ids (SMHV_WEB_*)
WEB_MAP_TILES = 6                          # the feed's own message (smhv_batch_feed_tiles / smhv_feed_frame_tiles): the reference has none
FEED_SNAPSHOT = 1                          # smhv_batch_feed / smhv_feed_frame flags: what a client that has just connected gets

E_INVALID, E_GEOMETRY, E_HIP, E_NO_DEVICE, E_STATE = -1, -2, -3, -4, -5
FRAME_OK, FRAME_LSD_STUCK = 0, 1          # smhv_frame_result.status


class Line(C.Structure):
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float)]


class FrameResult(C.Structure):
    _fields_ = [
        ("map_open", C.c_uint32), ("n_lines", C.c_uint32),
        ("lines", Line * MAX_LINES),
        ("mpx", C.c_double), ("has_mpx", C.c_uint32), ("n_mask_px", C.c_uint32),
        ("red_pixels", C.c_uint32), ("rounds", C.c_uint32), ("ray_steps", C.c_uint64),
        ("length_px", C.c_double * MAX_LINES), ("meters", C.c_double * MAX_LINES), ("angle", C.c_float * MAX_LINES),
        ("minimap", C.c_uint32 * 4), ("has_minimap", C.c_uint32), ("status", C.c_uint32),
    ]


class Anchors(C.Structure):
    _fields_ = [("n", C.c_uint32), ("scales_start_y", C.c_uint32), ("scales", (C.c_uint32 * 3) * MAX_SCALES)]


class BatchLayout(C.Structure):
    _fields_ = [
        ("frame_w", C.c_uint32), ("frame_h", C.c_uint32), ("roi", C.c_uint32 * 4), ("button", C.c_uint32 * 4),
        ("brq_w", C.c_uint32), ("brq_h", C.c_uint32),
        ("ui_pitch", C.c_uint64), ("ui_stride", C.c_uint64), ("ui_offset", C.c_uint64),
        ("mask_pitch", C.c_uint64), ("mask_stride", C.c_uint64), ("mask_offset", C.c_uint64),
        ("ocr_pitch", C.c_uint64), ("ocr_stride", C.c_uint64), ("ocr_offset", C.c_uint64),
        ("scales_pitch", C.c_uint64), ("scales_stride", C.c_uint64), ("scales_offset", C.c_uint64),
        ("bits_pitch_words", C.c_uint64), ("bits_stride", C.c_uint64), ("bits_xoff", C.c_uint64),
    ]


class FiringOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("viewport_scale", C.c_float * 2), ("viewport_top_left", C.c_float * 2)]


class RenderOptions(C.Structure):
    """smhv_render_options (include/smh_vision_hip.h): the window, the map quad and the viewport of a map view."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("quad", C.c_float * 4),
                ("viewport_scale", C.c_float * 2), ("viewport_top_left", C.c_float * 2), ("background", C.c_uint8 * 4)]


class RenderPrim(C.Structure):
    """smhv_render_prim: a line or a rectangle outline in map-ROI coordinates (24 bytes)."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("rgba", C.c_uint8 * 4), ("kind", C.c_uint32)]


class RenderLayersStruct(C.Structure):
    """smhv_render_layers: what a render call with layers draws beside the map view."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("map_source", C.c_uint32), ("n_prims", C.c_uint32), ("prims", C.POINTER(RenderPrim))]


class Firing(C.Structure):
    _fields_ = [("meters", C.c_double), ("alt_delta", C.c_double), ("mils", C.c_double * 2), ("bearing", C.c_float * 2),
                ("source", C.c_uint32), ("reserved", C.c_uint32)]


class FiringResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint32), ("reserved", C.c_uint32), ("line", Firing * MAX_LINES)]


LABEL_DETECTED, LABEL_MAX_EXTRA, LABEL_SLOTS = 1, 64, 64 + MAX_LINES


class LabelLine(C.Structure):
    """smhv_label_line: an extra line to label, with its colour (20 bytes)."""
    _fields_ = [("line", Line), ("rgba", C.c_uint8 * 4)]


class LabelOptionsStruct(C.Structure):
    """smhv_label_options: which lines get a label, and the text's scale."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_uint32), ("n_extra", C.c_uint32), ("extra", C.POINTER(LabelLine)),
                ("mpx", C.POINTER(C.c_double))]


class LabelRun(C.Structure):
    """smhv_label_run: one row of text, placed in half font units (24 bytes)."""
    _fields_ = [("x2", C.c_int16), ("y2", C.c_int16), ("n", C.c_uint8), ("pad", C.c_uint8 * 3), ("text", C.c_uint8 * 16)]


class Label(C.Structure):
    """smhv_label: a slot -- the numbers, the placement, the colour and the runs of one line (216 bytes)."""
    _fields_ = [("firing", Firing), ("mid", C.c_float * 2), ("dir", C.c_float * 2), ("rgba", C.c_uint8 * 4), ("n_runs", C.c_uint32), ("run", LabelRun * 6)]


class LabelResult(C.Structure):
    _fields_ = [("n_labels", C.c_uint32), ("reserved", C.c_uint32), ("label", Label * LABEL_SLOTS)]


REACH_PAINT, REACH_CLASSES = 1, 2                                      # smhv_reach_options.flags
REACH_ORIGIN_POINT, REACH_ORIGIN_LINE_P0, REACH_ORIGIN_LINE_P1 = 0, 1, 2   # smhv_reach_options.origin_mode
REACH_OUT_OF_RANGE, REACH_BAND0, REACH_RING = 1, 2, 0x80              # the class byte


class ReachOptionsStruct(C.Structure):
    """smhv_reach_options: what a reach map is computed from and how it is painted (80 bytes)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("origin_mode", C.c_uint32), ("line", C.c_uint32), ("origin", C.c_float * 2),
                ("ring_m", C.c_double), ("out_of_range", C.c_uint8 * 4), ("band", (C.c_uint8 * 4) * 8), ("ring", C.c_uint8 * 4),
                ("reserved", C.c_uint32 * 2)]


class ReachResult(C.Structure):
    """smhv_reach_result: a frame's summary of its reach map (64 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("source_mask", C.c_uint32), ("origin", C.c_float * 2), ("count", C.c_uint32 * 9), ("ring", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


RELIEF_PAINT, RELIEF_BYTES, RELIEF_SHADES, RELIEF_HEIGHTS, RELIEF_NEAREST = 1, 2, 4, 8, 16   # smhv_relief_options.flags
RELIEF_HAS_HEIGHT, RELIEF_CONTOUR, RELIEF_MAJOR = 1, 2, 4             # the flag byte


class ReliefOptionsStruct(C.Structure):
    """smhv_relief_options: contour spacing, the hillshade's light and the paint of a terrain relief (80 bytes)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("major_every", C.c_uint32), ("reserved0", C.c_uint32), ("interval_m", C.c_double),
                ("base_m", C.c_double), ("exaggeration", C.c_double), ("light", C.c_double * 3), ("contour", C.c_uint8 * 4), ("major", C.c_uint8 * 4),
                ("shade_weight", C.c_uint32), ("reserved", C.c_uint32)]


class ReliefResult(C.Structure):
    """smhv_relief_result: a frame's summary of its terrain relief (48 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("n_height", C.c_uint32), ("n_contour", C.c_uint32), ("n_major", C.c_uint32), ("z_min", C.c_double),
                ("z_max", C.c_double), ("reserved", C.c_uint32 * 4)]


class ReliefPlanes(C.Structure):
    """smhv_relief_planes: the device memory of the planes a batch call writes (24 bytes)."""
    _fields_ = [("bytes", C.c_void_p), ("shades", C.c_void_p), ("heights", C.c_void_p)]


GRID_PAINT, GRID_BYTES, GRID_CELLS = 1, 2, 4                          # smhv_grid_options.flags
GRID_HAS_CELL, GRID_LABEL = 1, 0x10                                   # the flag byte; bits 1 .. 3 = line level + 1
GRID_NONE, GRID_SCALES, GRID_HEIGHTMAP = 0, 1, 2                      # smhv_grid_result.source


class GridOptionsStruct(C.Structure):
    """smhv_grid_options: the cells, their keypad levels and the paint of a map grid (80 bytes)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("levels", C.c_uint32), ("reserved0", C.c_uint32), ("cell_m", C.c_double),
                ("origin_m", C.c_double * 2), ("min_px", C.c_double), ("label_min_px", C.c_double), ("line", (C.c_uint8 * 4) * 4),
                ("label", C.c_uint8 * 4), ("reserved", C.c_uint32)]


class GridResult(C.Structure):
    """smhv_grid_result: a frame's summary of its map grid (64 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("source", C.c_uint32), ("drawn_levels", C.c_uint32), ("n_cell", C.c_uint32), ("n_line", C.c_uint32 * 4),
                ("n_label", C.c_uint32), ("col_first", C.c_uint32), ("col_last", C.c_uint32), ("row_first", C.c_uint32), ("row_last", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class GridPlanes(C.Structure):
    """smhv_grid_planes: the device memory of the planes a batch call writes (16 bytes)."""
    _fields_ = [("bytes", C.c_void_p), ("cells", C.c_void_p)]


class GridRef(C.Structure):
    """smhv_grid_ref: the grid reference of a point (48 bytes)."""
    _fields_ = [("x_m", C.c_double), ("y_m", C.c_double), ("col", C.c_uint32), ("row1", C.c_uint32), ("digit", C.c_uint8 * 3), ("valid", C.c_uint8),
                ("reserved", C.c_uint32), ("text", C.c_char * 16)]


class GridRefsResult(C.Structure):
    """smhv_grid_refs_result: the references of the ends of a frame's lines (3088 bytes)."""
    _fields_ = [("n_lines", C.c_uint32), ("source", C.c_uint32), ("reserved", C.c_uint32 * 2), ("ref", (GridRef * 2) * MAX_LINES)]


ARC_HIGH, ARC_LOW = 0, 1                                               # smhv_weapon.arc; the index into BallisticSolution.arc
ANGLE_MILS6400, ANGLE_MILS6000, ANGLE_DEGREES = 0, 1, 2                # smhv_weapon.unit
BAL_OUT_OF_RANGE, BAL_BELOW_MIN_RANGE, BAL_ELEV_LOW, BAL_ELEV_HIGH = 1, 2, 4, 8   # smhv_ballistic_arc.status
BMAP_PAINT, BMAP_CLASSES, BMAP_TOF = 1, 2, 4                           # smhv_ballistic_options.flags
BMAP_OUT_OF_RANGE, BMAP_BELOW_MIN_RANGE, BMAP_ELEV_LOW, BMAP_ELEV_HIGH, BMAP_BAND0, BMAP_ISO = 1, 2, 3, 4, 5, 0x80   # the class byte


class WeaponStruct(C.Structure):
    """smhv_weapon: a caller-supplied weapon (80 bytes)."""
    _fields_ = [("size", C.c_uint32), ("arc", C.c_uint32), ("unit", C.c_uint32), ("reserved0", C.c_uint32), ("velocity", C.c_double),
                ("gravity", C.c_double), ("elev_min", C.c_double), ("elev_max", C.c_double), ("range_min", C.c_double), ("dispersion", C.c_double),
                ("reserved", C.c_uint32 * 4)]


class WeaponRule(C.Structure):
    """smhv_weapon_rule: the weapon in the rule's terms (136 bytes)."""
    _fields_ = [("v", C.c_double), ("g", C.c_double), ("v2", C.c_double), ("v4", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double),
                ("band", C.c_double * 7), ("t_disp", C.c_double), ("range_min", C.c_double), ("unit_deg", C.c_double), ("arc", C.c_uint32),
                ("unit", C.c_uint32)]


class BallisticArc(C.Structure):
    """smhv_ballistic_arc: one root of a solution (48 bytes)."""
    _fields_ = [("elevation", C.c_double), ("tof", C.c_double), ("apex", C.c_double), ("fall", C.c_double), ("along", C.c_double),
                ("status", C.c_uint32), ("band", C.c_uint32)]


class BallisticSolution(C.Structure):
    """smhv_ballistic_solution: both arcs of one (meters, alt) (128 bytes)."""
    _fields_ = [("meters", C.c_double), ("alt_delta", C.c_double), ("cross", C.c_double), ("source", C.c_uint32), ("reserved", C.c_uint32),
                ("arc", BallisticArc * 2)]


class Ballistic(C.Structure):
    """smhv_ballistic: a line's two directions (256 bytes)."""
    _fields_ = [("dir", BallisticSolution * 2)]


class BallisticResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint32), ("reserved", C.c_uint32 * 3), ("line", Ballistic * MAX_LINES)]


class BallisticOptionsStruct(C.Structure):
    """smhv_ballistic_options: what a ballistic map is computed from and how it is painted (96 bytes)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("origin_mode", C.c_uint32), ("line", C.c_uint32), ("origin", C.c_float * 2),
                ("iso_s", C.c_double), ("pal", (C.c_uint8 * 4) * 12), ("iso", C.c_uint8 * 4), ("reserved", C.c_uint32 * 3)]


class BallisticMapResult(C.Structure):
    """smhv_ballistic_map_result: a frame's summary of its ballistic map (96 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("source_mask", C.c_uint32), ("origin", C.c_float * 2), ("count", C.c_uint32 * 12), ("iso", C.c_uint32),
                ("n_tof", C.c_uint32), ("tof_min", C.c_double), ("tof_max", C.c_double), ("reserved", C.c_uint32 * 2)]


class BallisticPlanes(C.Structure):
    """smhv_ballistic_planes: the device memory of the planes a batch call writes (16 bytes)."""
    _fields_ = [("classes", C.c_void_p), ("tof", C.c_void_p)]


BCLR_PAINT, BCLR_BYTES, BCLR_MARGIN = 1, 2, 4                          # smhv_ballistic_clearance_options.flags
BCLR_NONE, BCLR_OUT_OF_RANGE, BCLR_UNUSABLE, BCLR_CLEAR, BCLR_BLOCKED, BCLR_LOS = 0, 1, 2, 3, 4, 0x80   # an arc's class; the map's byte


class BallisticClearanceOptionsStruct(C.Structure):
    """smhv_ballistic_clearance_options: how the terrain is sampled against both arcs of a weapon and painted (80 bytes)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("samples", C.c_uint32), ("origin_mode", C.c_uint32), ("line", C.c_uint32),
                ("reserved0", C.c_uint32), ("origin", C.c_float * 2), ("margin_m", C.c_double), ("pal", (C.c_uint8 * 4) * 4), ("switch_arc", C.c_uint8 * 4),
                ("los", C.c_uint8 * 4), ("reserved", C.c_uint32 * 4)]


class ArcClearance(C.Structure):
    """smhv_arc_clearance: one arc of one direction against the terrain (32 bytes)."""
    _fields_ = [("status", C.c_uint32), ("first_blocked", C.c_uint32), ("n_blocked", C.c_uint32), ("bal", C.c_uint32), ("min_margin", C.c_double),
                ("min_at", C.c_uint32), ("reserved", C.c_uint32)]


class BallisticClearanceDir(C.Structure):
    """smhv_ballistic_clearance_dir: both arcs of one direction of a line (96 bytes)."""
    _fields_ = [("arc", ArcClearance * 2), ("meters", C.c_double), ("alt_delta", C.c_double), ("los_blocked", C.c_uint32), ("valid", C.c_uint32),
                ("choice", C.c_uint32), ("reserved", C.c_uint32)]


class BallisticClearance(C.Structure):
    """smhv_ballistic_clearance: a line's two directions (192 bytes)."""
    _fields_ = [("dir", BallisticClearanceDir * 2)]


class BallisticClearanceResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint32), ("reserved", C.c_uint32 * 3), ("line", BallisticClearance * MAX_LINES)]


class BallisticClearanceMapResult(C.Structure):
    """smhv_ballistic_clearance_map_result: a frame's summary of its ballistic clearance map (64 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("reserved0", C.c_uint32), ("origin", C.c_float * 2), ("own", C.c_uint32 * 4), ("other", C.c_uint32 * 4),
                ("los_blocked", C.c_uint32), ("switch_arc", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class BallisticClearancePlanes(C.Structure):
    """smhv_ballistic_clearance_planes: the device memory of the planes a batch call writes (16 bytes)."""
    _fields_ = [("bytes", C.c_void_p), ("margin", C.c_void_p)]


CLEAR_MAX_SAMPLES = 256
CLEAR_PROFILE = CLEAR_MAX_SAMPLES + 1                                  # floats of a line's profile row
CLEAR_PAINT, CLEAR_BYTES = 1, 2                                        # smhv_clearance_options.flags
CLEAR_NONE, CLEAR_OUT_OF_RANGE, CLEAR_CLEAR, CLEAR_BLOCKED, CLEAR_LOS_BLOCKED = 0, 1, 2, 3, 0x80   # the status; the map's byte


class ClearanceOptionsStruct(C.Structure):
    """smhv_clearance_options: how the terrain between the ends of a line of fire is sampled and painted (64 bytes)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("samples", C.c_uint32), ("origin_mode", C.c_uint32), ("line", C.c_uint32),
                ("reserved0", C.c_uint32), ("origin", C.c_float * 2), ("margin_m", C.c_double), ("out_of_range", C.c_uint8 * 4), ("clear", C.c_uint8 * 4),
                ("blocked", C.c_uint8 * 4), ("los", C.c_uint8 * 4), ("reserved", C.c_uint32 * 2)]


class ClearanceDir(C.Structure):
    """smhv_clearance_dir: the verdict of one direction of a line (32 bytes)."""
    _fields_ = [("status", C.c_uint32), ("first_blocked", C.c_uint32), ("n_blocked", C.c_uint32), ("los_blocked", C.c_uint32), ("min_margin", C.c_double),
                ("min_at", C.c_uint32), ("reserved", C.c_uint32)]


class Clearance(C.Structure):
    _fields_ = [("dir", ClearanceDir * 2)]


class ClearanceResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint32), ("reserved", C.c_uint32), ("line", Clearance * MAX_LINES)]


class ClearanceMapResult(C.Structure):
    """smhv_clearance_map_result: a frame's summary of its clearance map (32 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("origin", C.c_float * 2), ("count", C.c_uint32 * 3), ("los_blocked", C.c_uint32)]


MAX_SCALE_LABELS, LABEL_MAX_RUNS, LABEL_CROP_W, LABEL_CROP_H = 8, 4096, 128, 32
LABELS_RUNS_OVERFLOW = 1                                               # smhv_scale_label_frame.flags


class ScaleLabel(C.Structure):
    """smhv_scale_label: a word's box, the scale bar under it and the bar's width (32 bytes)."""
    _fields_ = [("left", C.c_uint32), ("top", C.c_uint32), ("right", C.c_uint32), ("bottom", C.c_uint32), ("bar_left", C.c_uint32), ("bar_y", C.c_uint32),
                ("bar_right", C.c_uint32), ("width", C.c_uint32)]


class ScaleLabelFrame(C.Structure):
    """smhv_scale_label_frame: a frame's scale labels (288 bytes)."""
    _fields_ = [("n", C.c_uint32), ("n_found", C.c_uint32), ("n_words", C.c_uint32), ("n_runs", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3),
                ("label", ScaleLabel * MAX_SCALE_LABELS)]


LABEL_MAX_GLYPHS, ATLAS_MAX_TEMPLATES = 16, 32
LABEL_TEXT_TOO_MANY = 1                                                # smhv_label_text_entry.flags


class GlyphTemplate(C.Structure):
    """smhv_glyph_template: a glyph's code and its tight bitmap, bit x of rows[y] (132 bytes)."""
    _fields_ = [("code", C.c_uint8), ("w", C.c_uint8), ("h", C.c_uint8), ("reserved", C.c_uint8), ("rows", C.c_uint32 * 32)]


class GlyphAtlasOptions(C.Structure):
    _fields_ = [("accept_num", C.c_uint32), ("accept_den", C.c_uint32)]


class LabelTextEntry(C.Structure):
    """smhv_label_text_entry: a label's text as the device read it (112 bytes)."""
    _fields_ = [("text", C.c_char * LABEL_MAX_GLYPHS), ("n_glyphs", C.c_uint32), ("flags", C.c_uint32), ("meters", C.c_uint32), ("reserved", C.c_uint32),
                ("best", C.c_uint16 * LABEL_MAX_GLYPHS), ("second", C.c_uint16 * LABEL_MAX_GLYPHS), ("tmpl", C.c_uint8 * LABEL_MAX_GLYPHS)]


class LabelTextFrame(C.Structure):
    """smhv_label_text_frame: a frame's label texts, its anchors and meters per pixel (960 bytes)."""
    _fields_ = [("n", C.c_uint32), ("has", C.c_uint32), ("mpx", C.c_double), ("anchors", Anchors), ("reserved", C.c_uint32),
                ("label", LabelTextEntry * MAX_SCALE_LABELS)]


assert C.sizeof(GlyphTemplate) == 132 and C.sizeof(LabelTextEntry) == 112 and C.sizeof(LabelTextFrame) == 960

TEXT_MAX_RUNS, TEXT_MAX_BYTES, TEXT_MAX_LINES, TEXT_MAP_COORDS = 64, 64, 8, 1
MAX_PROBES = 16
DEBUG_DRAW_PROBES, DEBUG_MINIMAP_CAPTION = 1, 2   # smhv_debug_options.flags


class TextRun(C.Structure):
    """smhv_text_run: a run of debug text, its anchor and colour (84 bytes)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("rgba", C.c_uint8 * 4), ("flags", C.c_uint32), ("n", C.c_uint32), ("text", C.c_uint8 * TEXT_MAX_BYTES)]


class ProbePoint(C.Structure):
    """smhv_probe_point: a window position of the vision debugger."""
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class Probe(C.Structure):
    """smhv_probe: what the vision debugger prints about the pixel under a window position (32 bytes)."""
    _fields_ = [("valid", C.c_uint32), ("px", C.c_uint32), ("py", C.c_uint32), ("rgb", C.c_uint8 * 3), ("luma", C.c_uint8), ("h", C.c_uint16),
                ("s", C.c_uint8), ("v", C.c_uint8), ("mono", C.c_uint16), ("brightness", C.c_uint8), ("reserved0", C.c_uint8),
                ("team_bits", C.c_uint32), ("reserved1", C.c_uint32)]


class DebugOptionsStruct(C.Structure):
    """smhv_debug_options: the text runs, the probes and the switches of a debug pass."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_uint32), ("n_runs", C.c_uint32), ("runs", C.POINTER(TextRun)),
                ("n_probes", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.POINTER(ProbePoint))]


class FeedEntry(C.Structure):
    """smhv_feed_entry: a message of a feed's buffer (24 bytes)."""
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("frame", C.c_uint32), ("kind", C.c_uint32), ("crc", C.c_uint32)]


class FeedHeader(C.Structure):
    """smhv_feed_header: what a feed's last call wrote (32 bytes)."""
    _fields_ = [("n_entries", C.c_uint32), ("frames_done", C.c_uint32), ("n_maps", C.c_uint32), ("has_last_crc", C.c_uint32),
                ("last_crc", C.c_uint32), ("reserved", C.c_uint32), ("bytes_used", C.c_uint64)]


PIXELS_NV12, PIXELS_I420 = 5, 6            # SMHV_PIXELS_*: 8-bit 4:2:0 video frames
YUV_ROI_ONLY = 1                           # smhv_yuv_to_bgra_device flags
VIDEO_SRC_RGBA = 1                         # smhv_bgra_to_yuv_device src_flags: the source bytes are R, G, B, A
VIDEO_RENDER, VIDEO_UI_MAP = 0, 1          # smhv_batch_video sources


class YuvLayout(C.Structure):
    """smhv_yuv_layout: pitches and plane offsets of a decoded surface, in bytes (a zero member: tight)."""
    _fields_ = [("y_pitch", C.c_uint64), ("uv_pitch", C.c_uint64), ("u_offset", C.c_uint64), ("v_offset", C.c_uint64), ("frame_stride", C.c_uint64)]


LOG_FN = C.CFUNCTYPE(None, C.c_int, C.c_char_p)

# name -> (restype, argtypes); every symbol include/smh_vision_hip.h declares
SIGNATURES = {
    "smhv_init": (C.c_int, [C.c_int, LOG_FN, C.POINTER(C.c_void_p)]),
    "smhv_shutdown": (None, [C.c_void_p]),
    "smhv_thread_ctx": (C.c_int, [C.c_void_p]),
    "smhv_set_ray_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "smhv_last_error": (C.c_char_p, []),
    "smhv_map_bounds": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "smhv_button_bounds": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "smhv_load_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "smhv_load_frame_view": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6),
    "smhv_load_frame_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "smhv_crop_to_map": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_void_p]),
    "smhv_red_pixels": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "smhv_ocr_preprocess": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "smhv_find_scales_preprocess": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_isolate_map_markers": (C.c_int, [C.c_void_p]),
    "smhv_mask_marker_lines": (C.c_int, [C.c_void_p]),
    "smhv_get_lsd_image": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_find_longest_line": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.POINTER(Line), C.POINTER(C.c_float)]),
    "smhv_find_marker_lines": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(Line), C.POINTER(C.c_uint32)]),
    "smhv_lsd_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "smhv_calc_meters_to_px_ratio": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "smhv_find_minimap": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "smhv_get_debug_view": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_batch_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "smhv_batch_destroy": (None, [C.c_void_p]),
    "smhv_batch_layout_get": (C.c_int, [C.c_void_p, C.POINTER(BatchLayout)]),
    "smhv_batch_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]),
    "smhv_batch_device_ptrs": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6),
    "smhv_batch_tile_mask": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    "smhv_batch_read_tile_mask": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "smhv_batch_read_results": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(FrameResult)]),
    "smhv_batch_read_image": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "smhv_batch_set_scales_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smhv_batch_wait_map_pass": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smhv_batch_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "smhv_batch_lsd_coop_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "smhv_batch_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "smhv_pipeline_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "smhv_pipeline_create_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_pipeline_hold": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_debug_pipeline_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "smhv_debug_pipeline_peek": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "smhv_pipeline_destroy": (None, [C.c_void_p]),
    "smhv_pipeline_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "smhv_pipeline_wait": (C.c_int, [C.c_void_p, C.c_uint32]),
    "smhv_pipeline_wait_all": (C.c_int, [C.c_void_p]),
    "smhv_pipeline_slot": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "smhv_shard_range": (None, [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "smhv_node_create": (C.c_int, [C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, LOG_FN, C.POINTER(C.c_void_p)]),
    "smhv_node_destroy": (None, [C.c_void_p]),
    "smhv_node_ctx": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "smhv_node_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]),
    "smhv_node_gather": (C.c_int, [C.c_void_p, C.POINTER(FrameResult), C.POINTER(C.c_uint32)]),
    "smhv_debug_lsd_classic": (C.c_int, [C.c_int]),
    "smhv_debug_lsd_tile_cap": (C.c_int, [C.c_uint32]),
    "smhv_debug_lsd_spin_limit": (C.c_int, [C.c_uint32]),
    "smhv_debug_lsd_threads": (C.c_int, [C.c_uint32]),
    "smhv_debug_skip_line_search": (C.c_int, [C.c_int]),
    "smhv_debug_no_host_atomics": (C.c_int, [C.c_int]),
    "smhv_debug_side_kernel": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_trait_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "smhv_ui_map": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_debug_pattern_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "smhv_debug_batch_mask_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "smhv_debug_batch_ui_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "smhv_debug_batch_materialize_ui": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smhv_debug_mask_expand": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_debug_marker_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smhv_ingest_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "smhv_ingest_create_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "smhv_crc32_host": (C.c_uint32, [C.c_void_p, C.c_uint64]),
    "smhv_debug_map_band_rows": (C.c_int, [C.c_uint32]),
    "smhv_debug_band_rows": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "smhv_debug_ingest_feed": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "smhv_debug_ingest_feed_pixels": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    "smhv_debug_crc32_host_level": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]),
    "smhv_ingest_destroy": (None, [C.c_void_p]),
    "smhv_ingest_local_cpus": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "smhv_ingest_bind_thread": (C.c_int, [C.c_void_p]),
    "smhv_ingest_acquire": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_ingest_commit": (C.c_int, [C.c_void_p]),
    "smhv_ingest_push": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smhv_ingest_commit_pixels": (C.c_int, [C.c_void_p, C.c_uint32]),
    "smhv_ingest_push_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "smhv_ingest_staging_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "smhv_yuv_to_bgra_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(YuvLayout), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                          C.c_uint32, C.c_void_p]),
    "smhv_bgra_to_yuv_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.POINTER(YuvLayout), C.c_void_p]),
    "smhv_batch_video": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(YuvLayout), C.c_void_p]),
    "smhv_video_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "smhv_ingest_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_ingest_reset": (C.c_int, [C.c_void_p]),
    "smhv_ingest_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "smhv_crc32_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
    "smhv_heightmap_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_void_p)]),
    "smhv_heightmap_destroy": (None, [C.c_void_p]),
    "smhv_heightmap_color_map": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smhv_debug_heightmap_color_map_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "smhv_batch_set_firing": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FiringOptions)]),
    "smhv_pipeline_set_firing": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FiringOptions)]),
    "smhv_batch_read_firing": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(FiringResult)]),
    "smhv_batch_firing_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_firing_solutions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p,
                                        C.POINTER(FiringOptions), C.POINTER(Firing)]),
    "smhv_batch_overlay_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_heightmap_overlay": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FiringOptions), C.c_void_p]),
    "smhv_map_viewport_calc": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.POINTER(RenderOptions)]),
    "smhv_batch_render": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.c_void_p]),
    "smhv_batch_render_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "smhv_batch_render_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_batch_read_render": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_batch_render_layers": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(RenderLayersStruct), C.c_void_p]),
    "smhv_render_map_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(RenderLayersStruct), C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_render_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_label_font": (C.c_int, [C.c_uint8, C.POINTER(C.c_uint8)]),
    "smhv_batch_render_labels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(LabelOptionsStruct), C.c_void_p]),
    "smhv_batch_read_labels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(LabelResult)]),
    "smhv_batch_labels_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_render_map_labeled": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(RenderLayersStruct), C.c_void_p, C.c_uint32,
                                          C.POINTER(LabelOptionsStruct), C.c_void_p, C.POINTER(LabelResult)]),
    "smhv_text_font": (C.c_int, [C.c_uint8, C.POINTER(C.c_uint8)]),
    "smhv_probe_text": (C.c_int, [C.POINTER(Probe), C.c_char_p, C.c_size_t]),
    "smhv_batch_probe": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RenderOptions), C.POINTER(ProbePoint), C.c_uint32, C.c_void_p]),
    "smhv_batch_read_probes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Probe)]),
    "smhv_batch_probes_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_batch_render_debug": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RenderOptions), C.POINTER(DebugOptionsStruct), C.c_void_p]),
    "smhv_render_map_debug": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(RenderLayersStruct), C.c_void_p, C.c_uint32,
                                        C.POINTER(LabelOptionsStruct), C.POINTER(DebugOptionsStruct), C.c_void_p, C.POINTER(LabelResult), C.POINTER(Probe)]),
    "smhv_feed_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "smhv_feed_destroy": (None, [C.c_void_p]),
    "smhv_feed_reset": (C.c_int, [C.c_void_p]),
    "smhv_batch_feed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "smhv_feed_read": (C.c_int, [C.c_void_p, C.POINTER(FeedHeader), C.POINTER(FeedEntry), C.c_uint32, C.c_void_p, C.c_uint64]),
    "smhv_feed_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "smhv_feed_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32]),
    "smhv_web_event_markers": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "smhv_web_event_heightmap": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p, C.c_uint64,
                                           C.POINTER(C.c_uint64)]),
    "smhv_web_event_fit": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "smhv_web_interaction_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "smhv_debug_feed_rows": (C.c_int, [C.c_uint32]),
    "smhv_debug_feed_gray_form": (C.c_int, [C.c_uint32]),
    "smhv_batch_feed_view": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "smhv_feed_frame_view": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]),
    "smhv_batch_feed_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "smhv_feed_frame_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32]),
    "smhv_reach_defaults": (C.c_int, [C.POINTER(ReachOptionsStruct)]),
    "smhv_reach_thresholds": (C.c_int, [C.POINTER(C.c_double)]),
    "smhv_batch_reach": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(ReachOptionsStruct), C.c_void_p,
                                   C.c_void_p]),
    "smhv_batch_read_reach": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ReachResult)]),
    "smhv_batch_reach_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_reach_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(ReachOptionsStruct), C.POINTER(C.c_double),
                                 C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.POINTER(ReachResult)]),
    "smhv_clearance_defaults": (C.c_int, [C.POINTER(ClearanceOptionsStruct)]),
    "smhv_batch_clearance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(FiringOptions), C.POINTER(ClearanceOptionsStruct), C.c_void_p,
                                       C.c_void_p]),
    "smhv_batch_read_clearance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ClearanceResult)]),
    "smhv_batch_clearance_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_clearance_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(FiringOptions),
                                       C.POINTER(ClearanceOptionsStruct), C.POINTER(Clearance), C.c_void_p]),
    "smhv_batch_clearance_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(ClearanceOptionsStruct),
                                           C.c_void_p, C.c_void_p]),
    "smhv_batch_read_clearance_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ClearanceMapResult)]),
    "smhv_batch_clearance_map_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_clearance_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(ClearanceOptionsStruct), C.POINTER(C.c_uint32), C.c_void_p,
                                     C.c_void_p, C.POINTER(ClearanceMapResult)]),
    "smhv_relief_defaults": (C.c_int, [C.POINTER(ReliefOptionsStruct)]),
    "smhv_batch_relief": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(ReliefOptionsStruct),
                                    C.POINTER(ReliefPlanes), C.c_void_p]),
    "smhv_batch_read_relief": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ReliefResult)]),
    "smhv_batch_relief_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_grid_defaults": (C.c_int, [C.POINTER(GridOptionsStruct)]),
    "smhv_grid_ref_text": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.c_char_p]),
    "smhv_batch_grid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(GridOptionsStruct),
                                  C.POINTER(GridPlanes), C.c_void_p]),
    "smhv_batch_read_grid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(GridResult)]),
    "smhv_batch_grid_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_grid_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(GridOptionsStruct), C.POINTER(C.c_double),
                                C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GridResult)]),
    "smhv_batch_grid_refs": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(GridOptionsStruct), C.c_void_p]),
    "smhv_batch_read_grid_refs": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(GridRefsResult)]),
    "smhv_batch_grid_refs_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_grid_refs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(RenderOptions),
                                 C.POINTER(GridOptionsStruct), C.POINTER(GridRef)]),
    "smhv_relief_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(ReliefOptionsStruct), C.POINTER(C.c_uint32), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReliefResult)]),
    "smhv_batch_scale_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_batch_read_scale_labels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ScaleLabelFrame), C.c_void_p]),
    "smhv_batch_scale_labels_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "smhv_scale_labels": (C.c_int, [C.c_void_p, C.POINTER(ScaleLabelFrame), C.c_void_p]),
    "smhv_glyph_templates_check": (C.c_int, [C.POINTER(GlyphTemplate), C.c_uint32]),
    "smhv_glyph_templates_from_label": (C.c_int, [C.c_void_p, C.POINTER(ScaleLabel), C.c_char_p, C.POINTER(GlyphTemplate), C.POINTER(C.c_uint32)]),
    "smhv_glyph_atlas_create": (C.c_int, [C.c_void_p, C.POINTER(GlyphTemplate), C.c_uint32, C.POINTER(GlyphAtlasOptions), C.POINTER(C.c_void_p)]),
    "smhv_glyph_atlas_destroy": (None, [C.c_void_p]),
    "smhv_batch_label_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "smhv_batch_read_label_text": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(LabelTextFrame)]),
    "smhv_batch_label_text_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "smhv_label_text": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LabelTextFrame)]),
    "smhv_batch_run_label_anchors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p]),
    "smhv_scale_labels_anchors": (C.c_int, [C.POINTER(ScaleLabel), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(Anchors), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int)]),
    "smhv_debug_render_form": (C.c_int, [C.c_uint32]),
    "smhv_debug_render_rule": (C.c_int, [C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "smhv_weapon_defaults": (C.c_int, [C.POINTER(WeaponStruct)]),
    "smhv_weapon_check": (C.c_int, [C.POINTER(WeaponStruct)]),
    "smhv_weapon_thresholds": (C.c_int, [C.POINTER(WeaponStruct), C.POINTER(WeaponRule)]),
    "smhv_ballistic_solve": (C.c_int, [C.POINTER(WeaponStruct), C.c_double, C.c_double, C.POINTER(BallisticSolution)]),
    "smhv_ballistic_defaults": (C.c_int, [C.POINTER(BallisticOptionsStruct)]),
    "smhv_batch_ballistics": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(FiringOptions), C.POINTER(WeaponStruct), C.c_void_p]),
    "smhv_batch_read_ballistics": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BallisticResult)]),
    "smhv_batch_ballistics_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_ballistic_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(FiringOptions),
                                       C.POINTER(WeaponStruct), C.POINTER(Ballistic)]),
    "smhv_batch_ballistic_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(WeaponStruct),
                                           C.POINTER(BallisticOptionsStruct), C.POINTER(BallisticPlanes), C.c_void_p]),
    "smhv_batch_read_ballistic_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BallisticMapResult)]),
    "smhv_batch_ballistic_map_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_ballistic_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(WeaponStruct), C.POINTER(BallisticOptionsStruct),
                                     C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BallisticMapResult)]),
    "smhv_ballistic_clearance_defaults": (C.c_int, [C.POINTER(BallisticClearanceOptionsStruct)]),
    "smhv_ballistic_clearance_check": (C.c_int, [C.POINTER(BallisticClearanceOptionsStruct)]),
    "smhv_batch_ballistic_clearance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(FiringOptions), C.POINTER(WeaponStruct),
                                                 C.POINTER(BallisticClearanceOptionsStruct), C.c_void_p]),
    "smhv_batch_read_ballistic_clearance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BallisticClearanceResult)]),
    "smhv_batch_ballistic_clearance_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_ballistic_clearance_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(FiringOptions),
                                                 C.POINTER(WeaponStruct), C.POINTER(BallisticClearanceOptionsStruct), C.POINTER(BallisticClearance)]),
    "smhv_batch_ballistic_clearance_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(WeaponStruct),
                                                     C.POINTER(BallisticClearanceOptionsStruct), C.POINTER(BallisticClearancePlanes), C.c_void_p]),
    "smhv_batch_read_ballistic_clearance_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BallisticClearanceMapResult)]),
    "smhv_batch_ballistic_clearance_map_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smhv_ballistic_clearance_map": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(WeaponStruct),
                                               C.POINTER(BallisticClearanceOptionsStruct), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(BallisticClearanceMapResult)]),
}


def firing_options(fit_to_minimap=True, viewport=None):
    """smhv_firing_options: fit_to_minimap=False is the app's switch off (SMHV_FIRING_BOUNDS_OFFSET); viewport = None or
    (scale_w, scale_h, top_left_x, top_left_y), the app's MapViewport."""
    o = FiringOptions()
    o.size = C.sizeof(FiringOptions)
    o.flags = 0 if fit_to_minimap else FIRING_BOUNDS_OFFSET
    if viewport is not None:
        sw, sh, tx, ty = viewport
        o.viewport_scale[0], o.viewport_scale[1] = sw, sh
        o.viewport_top_left[0], o.viewport_top_left[1] = tx, ty
    return o


# smhv_firing as a numpy structured dtype (the layout the header declares: 48 bytes)
FIRING_DTYPE = None


def firing_dtype():
    import numpy as np
    global FIRING_DTYPE
    if FIRING_DTYPE is None:
        FIRING_DTYPE = np.dtype([("meters", "<f8"), ("alt_delta", "<f8"), ("mils", "<f8", (2,)), ("bearing", "<f4", (2,)),
                                 ("source", "<u4"), ("reserved", "<u4")], align=True)
        assert FIRING_DTYPE.itemsize == C.sizeof(Firing)
    return FIRING_DTYPE


class PipelineOptions(C.Structure):
    """smhv_pipeline_options (include/smh_vision_hip.h): every 0 is the library's default."""
    _fields_ = [("size", C.c_uint32), ("search", C.c_uint32), ("streams", C.c_uint32), ("idle_close_us", C.c_uint32), ("occupancy_policy", C.c_uint32),
                ("late_helpers", C.c_uint32), ("service_workgroups", C.c_uint32), ("flags", C.c_uint32), ("remote_after", C.c_uint32), ("remote_tickets", C.c_uint32), ("remote_last", C.c_uint32), ("room_for_others", C.c_uint32)]


SEARCH_AUTO, SEARCH_BATCH, SEARCH_FRAME = 0, 1, 2
PIPE_NO_TEAM_HELP, PIPE_NO_STREAM_PRIORITY, PIPE_NO_PROLOGUE, PIPE_NO_REMOTE_HELP, PIPE_HELP_FIRST, PIPE_WALK_BIT_ROWS, PIPE_THREE_LOAD_SETS = 1, 2, 4, 8, 16, 32, 64


class VisionError(RuntimeError):
    """Any non-zero status from the library (the reference's anyhow::Error)."""

    def __init__(self, code, msg):
        super().__init__("smh_vision_hip error %d: %s" % (code, msg))
        self.code = code
        self.records = None   # E_STATE from read_results / gather: the records that were copied out before the error was raised


_lib = None


def load():
    """dlopen the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: the HIP extension is not built (run __graft_entry__.build() or "
                "`make -C squad-mortar-helper_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP runtimes in
        # one process do not work ("No HIP GPUs are available"), so when torch is installed it is
        # imported first and this library binds to the runtime torch loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _hm(heightmap):
    """The library's handle of a Heightmap, or None for none."""
    return heightmap._hm if heightmap is not None else None


def check(rc):
    if rc != 0:
        raise VisionError(rc, load().smhv_last_error().decode("utf-8", "replace"))
