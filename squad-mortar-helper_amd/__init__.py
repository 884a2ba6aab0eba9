"""squad-mortar-helper_amd: MI355X-native vision hot path of squad-mortar-helper.

Product code only -- nothing here imports oracle/.  Importing the binding submodules requires the
built HIP library (see _lib.load); geometry helpers and the synthetic generator also need it
because the screen-relative bounds are computed by the library itself.
"""
from . import _lib  # noqa: F401
from ._lib import VisionError, STAGE_ALL, STAGE_EXACT_STATS, STAGE_FIRING, STAGE_HEIGHTMAP_OVERLAY, STAGE_MARKERS, STAGE_MINIMAP, STAGE_LSD_HELPERS, STAGE_OCR, STAGE_SCALES, STAGE_UI_MAP  # noqa: F401
from .vision import DebugView, HipVision, VisionResults, VisionState, button_bounds, map_bounds, parse_ocr_labels  # noqa: F401
from .batch import FrameBatch, Pipeline, make_anchors, results_to_dicts  # noqa: F401
from .ingest import IngestQueue, crc32_device  # noqa: F401
from . import yuv  # noqa: F401
from .heightmap import Heightmap  # noqa: F401
from .render import MapViewport, RenderOptions, render_options  # noqa: F401
from .render import RenderLayers, ctl_marker_prims, ocr_box_prims, prim, scale_bar_prims  # noqa: F401
from .render import LabelOptions, label_lines  # noqa: F401
from .render import ReachOptions, reach_thresholds  # noqa: F401
from .render import ClearanceOptions  # noqa: F401
from .render import BallisticOptions  # noqa: F401
from .render import BallisticClearanceOptions  # noqa: F401
from . import ballistics  # noqa: F401
from .ballistics import Weapon  # noqa: F401
from .render import ReliefOptions, relief_light  # noqa: F401
from .render import GridOptions, grid_ref_text  # noqa: F401
from .render import scale_label_prims  # noqa: F401
from .vision import scale_label_hits, scale_labels_anchors  # noqa: F401
from ._lib import LABEL_CROP_H, LABEL_CROP_W, LABEL_MAX_RUNS, LABELS_RUNS_OVERFLOW, MAX_SCALE_LABELS, ScaleLabel, ScaleLabelFrame  # noqa: F401
from .glyphs import GlyphAtlas, entry_text, glyph_templates_check, glyph_templates_from_label  # noqa: F401
from ._lib import ATLAS_MAX_TEMPLATES, LABEL_MAX_GLYPHS, LABEL_TEXT_TOO_MANY, GlyphTemplate, LabelTextEntry, LabelTextFrame  # noqa: F401
from .render import DebugOptions, ocr_text_runs, probe_points, probe_text, rust_debug_str, scale_text_runs, text_run  # noqa: F401
from ._lib import DEBUG_DRAW_PROBES, DEBUG_MINIMAP_CAPTION, MAX_PROBES, TEXT_MAP_COORDS, TEXT_MAX_BYTES, TEXT_MAX_LINES, TEXT_MAX_RUNS  # noqa: F401
from ._lib import LAYER_MINIMAP_BOUNDS, PRIM_FOREGROUND, PRIM_LINE, PRIM_RECT, PRIM_SHIFT1, RENDER_MAX_PRIMS  # noqa: F401
from ._lib import RENDER_BOUNDS_OFFSET, RENDER_HEIGHTMAP, RENDER_MARKERS  # noqa: F401
from .web import MapTexture, WebFeed, decode_map_tiles, encode_fit, encode_heightmap, encode_markers, parse_interaction  # noqa: F401
from ._lib import FEED_SNAPSHOT, WEB_FIT_TO_MINIMAP, WEB_HEIGHTMAP, WEB_MAP, WEB_MAP_TILES, WEB_MARKERS, WEB_UPDATE_STATE  # noqa: F401
