"""Glyph atlases of the scale labels' text (smh_vision_hip.h, "scale labels: text"): the library ships no glyph shapes -- a caller
who has read one frame's labels once (by eye, with an OCR engine, through label_reader=) learns the templates from it, and
every later frame is read on the device."""
import ctypes as C

import numpy as np

from . import _lib as L


def entry_text(entry):
    """A LabelTextEntry's text as a str (sixteen glyphs fill the field: there is no terminator then)."""
    return C.string_at(C.addressof(entry), L.LABEL_MAX_GLYPHS).split(b"\0", 1)[0].decode("latin-1")


def _template_array(templates):
    templates = list(templates)
    arr = (L.GlyphTemplate * max(len(templates), 1))()
    for i, t in enumerate(templates):
        C.memmove(C.addressof(arr[i]), C.addressof(t), C.sizeof(L.GlyphTemplate))
    return arr, len(templates)


def glyph_templates_check(templates):
    """smhv_glyph_templates_check: raises VisionError (E_INVALID) naming the first template that is none."""
    arr, n = _template_array(templates)
    L.check(L.load().smhv_glyph_templates_check(arr, n))


def glyph_templates_from_label(crop, box, text):
    """smhv_glyph_templates_from_label: cuts one label by the rule and pairs glyph k with text[k].  crop: the label's cell, uint8
    [LABEL_CROP_H, LABEL_CROP_W]; box: a ScaleLabel or (left, top, right, bottom) -> [GlyphTemplate]."""
    cell = np.ascontiguousarray(crop, np.uint8)
    if cell.shape != (L.LABEL_CROP_H, L.LABEL_CROP_W):
        raise ValueError("a cell is uint8 [%d, %d]" % (L.LABEL_CROP_H, L.LABEL_CROP_W))
    if isinstance(box, L.ScaleLabel):
        lb = box
    else:
        lb = L.ScaleLabel()
        lb.left, lb.top, lb.right, lb.bottom = [int(v) for v in box[:4]]
    out = (L.GlyphTemplate * L.LABEL_MAX_GLYPHS)()
    n = C.c_uint32()
    L.check(L.load().smhv_glyph_templates_from_label(cell.ctypes.data, C.byref(lb), text.encode("latin-1"), out, C.byref(n)))
    res = []
    for i in range(n.value):
        t = L.GlyphTemplate()
        C.memmove(C.addressof(t), C.addressof(out[i]), C.sizeof(t))
        res.append(t)
    return res


class GlyphAtlas:
    """A device-resident glyph atlas (smhv_glyph_atlas): pass it to FrameBatch.label_text, HipVision.label_text or as
    VisionState.process(label_reader=)."""

    def __init__(self, vision, templates, accept_num=None, accept_den=None):
        self._lib = L.load()
        self._vision = vision                      # keeps the context alive
        arr, n = _template_array(templates)
        opt = None
        if accept_num is not None or accept_den is not None:
            opt = L.GlyphAtlasOptions(1 if accept_num is None else accept_num, 3 if accept_den is None else accept_den)
        a = C.c_void_p()
        L.check(self._lib.smhv_glyph_atlas_create(vision._ctx, arr if n else None, n, C.byref(opt) if opt is not None else None, C.byref(a)))
        self._a = a
        self.templates = [arr[i] for i in range(n)]
        self._keep = arr
        self.codes = "".join(chr(t.code) for t in self.templates)

    @classmethod
    def from_templates(cls, vision, templates, accept_num=None, accept_den=None):
        return cls(vision, templates, accept_num, accept_den)

    @classmethod
    def from_labels(cls, vision, labels, accept_num=None, accept_den=None):
        """labels: [(crop, box, text)] as a label_reader saw and read them.  Labels the helper cannot pair (the glyph count differs
        from the text's length, ...) raise; duplicate (code, bitmap) pairs are dropped, the first ATLAS_MAX_TEMPLATES kept."""
        return cls(vision, learn_templates(labels), accept_num, accept_den)

    def close(self):
        if getattr(self, "_a", None):
            self._lib.smhv_glyph_atlas_destroy(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def learn_templates(labels):
    """[(crop, box, text)] -> [GlyphTemplate]: glyph_templates_from_label on each, without duplicate (code, bitmap) pairs, at most
    ATLAS_MAX_TEMPLATES."""
    seen, out = set(), []
    for crop, box, text in labels:
        for t in glyph_templates_from_label(crop, box, text):
            key = bytes(t)
            if key not in seen and len(out) < L.ATLAS_MAX_TEMPLATES:
                seen.add(key)
                out.append(t)
    return out
