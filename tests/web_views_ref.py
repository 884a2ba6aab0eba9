"""A debug view as the remote-viewer feed's Map, restated in numpy: the reference shows and sends debug_view.unwrap_or(map)
(src/ui/map.rs:210-226), and include/smh_vision_hip.h ("Map sources" under "map view: layers") pins a batch's view bytes.
view_bytes() gives (w, h, bytes) -- what tests/web_ref.py's feed() takes per frame in the ui_map's place.  Pure numpy; needs
neither the library nor a device.  The frame sizes of the device tests and what they cover are stated here too, so that the host
suite can check the coverage without a device."""
import numpy as np

import render_layers_cases as LC
import web_ref as W

VIEW_NONE, VIEW_OCR_INPUT, VIEW_FIND_SCALES_INPUT, VIEW_LSD_PREPROCESS, VIEW_LSD_INPUT, VIEW_CROPPED_BRQ = range(6)
VIEWS = (VIEW_OCR_INPUT, VIEW_FIND_SCALES_INPUT, VIEW_LSD_PREPROCESS, VIEW_LSD_INPUT, VIEW_CROPPED_BRQ)

# Frame sizes of tests/test_web_views_gpu.py: the cropped quarter's start column mod 4 (the residual lead-in of its rows in the ui
# slab) takes 2, 0, 3, 1, 0, 3 and the quarter's width mod 4 every value; 347 x 363 has a map of 33 columns, a quarter of 16.
SIZES = ((451, 360), (454, 361), (347, 363), (568, 361), (1280, 1024), (1920, 1080))
Q_XOFF = (2, 0, 3, 1, 0, 3)
BRQ_W = (70, 71, 16, 128, 197, 493)
FEED_ROWS = (0, 1, 3, 8, 64)                 # smhv_debug_feed_rows: the rule, and forced splits of the rows over the waves


def gray(plane):
    """(L, L, L, 255) of a plane of one byte per pixel."""
    p = np.asarray(plane, np.uint8)
    return np.dstack([p, p, p, np.full_like(p, 255)])


def view_size(which, rw, rh):
    """Width and height of the Map a source sends for a map ROI of rw x rh."""
    return (rw, rh) if which in (VIEW_NONE, VIEW_LSD_PREPROCESS, VIEW_LSD_INPUT) else (rw // 2, rh // 2)


def view_image(which, ui=None, mask=None, ocr=None, scales=None):
    """The view as uint8 [h, w, 4].  ui: the COLOUR ui_map, RGBA [rh, rw, 4]; mask [rh, rw], ocr / scales [rh // 2, rw // 2]: the
    planes of one byte per pixel."""
    if which == VIEW_OCR_INPUT:
        return gray(ocr)
    if which == VIEW_FIND_SCALES_INPUT:
        return gray(scales)
    if which == VIEW_LSD_INPUT:
        return gray(mask)
    ui = np.asarray(ui, np.uint8)
    rh, rw = ui.shape[:2]
    if which == VIEW_LSD_PREPROCESS:                           # every pixel that fails the marker predicate (0, 0, 0); alpha 255
        out = ui.copy()
        out[..., 3] = 255
        out[~LC.marker_predicate(ui[..., 0], ui[..., 1], ui[..., 2])] = (0, 0, 0, 255)
        return out
    if which == VIEW_CROPPED_BRQ:                              # pixel (x, y) = the ui_map's (x + w/2, y + h/2), w/2 x h/2; alpha 255
        out = ui[rh // 2:rh // 2 + rh // 2, rw // 2:rw // 2 + rw // 2].copy()
        out[..., 3] = 255
        return out
    raise ValueError("unknown view %r" % (which,))


def view_bytes(which, ui=None, mask=None, ocr=None, scales=None):
    """-> (w, h, the Map payload's bytes)."""
    img = np.ascontiguousarray(view_image(which, ui, mask, ocr, scales))
    return img.shape[1], img.shape[0], img.tobytes()


def worst_case(which, rw, rh):
    """One frame's worst case in the buffer for a source: the Map has the SOURCE's width and height."""
    return W.worst_case(*view_size(which, rw, rh))


def coverage(map_bounds):
    """[(q_xoff, brq_w)] of SIZES from a map_bounds(W, H) -> (x, y, w, h) function."""
    out = []
    for Wd, Ht in SIZES:
        x, _, rw, _ = map_bounds(Wd, Ht)
        out.append(((x + rw // 2) % 4, rw // 2))
    return out


def check_coverage(map_bounds):
    cov = coverage(map_bounds)
    assert tuple(q for q, _ in cov) == Q_XOFF and tuple(w for _, w in cov) == BRQ_W, cov
    assert {q for q, _ in cov} == {0, 1, 2, 3} and {w % 4 for _, w in cov} == {0, 1, 2, 3}
    assert 16 in BRQ_W                                         # a quarter of exactly one 16-byte group of a plane, four of the slab
    return cov
