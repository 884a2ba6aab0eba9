"""Independent restatement of the scale-label rule (include/smh_vision_hip.h, "scale labels"; test infrastructure): which
blobs of the ocr_preprocess plane are words, their boxes, the scale bar under each and the glyph crops.

It works on PIXELS: every row is smeared (gaps of at most g background pixels between two foreground pixels are filled), the
smeared image is flood-filled with 8-connectivity, and the boxes are the extents of the filled pixels.  The device works on row
runs and a union-find over them; nothing here is formulated over runs, except that the header's n_runs is counted as the
number of maximal horizontal segments of the smeared image.  The bars come from the oracle's find_scale_width on the oracle's
find_scales_preprocess image with start row 0.
"""
import numpy as np

from oracle import oracle as o

MAX_LABELS = 8
MAX_RUNS = 4096
CROP_W, CROP_H = 128, 32
RUNS_OVERFLOW = 1


def gap(qw):
    """max(1, round(4.0 / 640.0 * qw)), f64::round (half away from zero), as the oracle rounds max_scale_y_offset."""
    v = (4.0 / 640.0) * float(qw)
    n = int(v)
    return max(1, n + 1 if v - n >= 0.5 else n)


def smear(fg, g):
    """fg: bool[h, w] -> bool[h, w]: a background pixel becomes foreground when it lies between two foreground pixels of its
    row that have at most g background pixels between them (a morphological closing of the row with g + 1 pixels)."""
    h, w = fg.shape
    ext = np.zeros((h, w + 2 * g), bool)
    ext[:, g:g + w] = fg
    dil = np.zeros((h, w + g), bool)                       # dil[x] = any fg in [x - g, x], x in [0, w + g)
    for k in range(g + 1):
        dil |= ext[:, g - k:g - k + w + g]
    out = np.ones((h, w), bool)                            # out[x] = all dil in [x, x + g]
    for k in range(g + 1):
        out &= dil[:, k:k + w]
    return out


def count_runs(sm):
    """Maximal horizontal segments of the smeared image."""
    first = sm.copy()
    first[:, 1:] &= ~sm[:, :-1]
    return int(first.sum())


def components(sm):
    """8-connected components of a bool image by flood fill -> [(left, top, right, bottom)], right / bottom exclusive."""
    todo = set(zip(*np.nonzero(sm)))                       # (y, x)
    boxes = []
    while todo:
        y0, x0 = todo.pop()
        stack = [(y0, x0)]
        l, t, r, b = x0, y0, x0, y0
        while stack:
            y, x = stack.pop()
            l, t, r, b = min(l, x), min(t, y), max(r, x), max(b, y)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    p = (y + dy, x + dx)
                    if p in todo:
                        todo.remove(p)
                        stack.append(p)
        boxes.append((int(l), int(t), int(r) + 1, int(b) + 1))
    return boxes


def scale_labels(P, S0):
    """P: the ocr_preprocess plane uint8[qh, qw]; S0: find_scales_preprocess with start row 0 ->
    dict(header=(n, n_found, n_words, n_runs, flags), labels=[(left, top, right, bottom, bar_left, bar_y, bar_right, width)]
    (the n written ones), all=[...] (all n_found, in order), crops=uint8[n, 32, 128])."""
    qh, qw = P.shape
    sm = smear(P != 255, gap(qw))
    n_runs = count_runs(sm)
    empty = np.zeros((0, CROP_H, CROP_W), np.uint8)
    if n_runs > MAX_RUNS:
        return dict(header=(0, 0, 0, n_runs, RUNS_OVERFLOW), labels=[], all=[], crops=empty)
    boxes = components(sm)
    found = []
    for (l, t, r, b) in boxes:
        if not (3 <= r - l <= CROP_W and 3 <= b - t <= CROP_H):
            continue
        bar = o.find_scale_width(1, (l + r) // 2, b, S0)
        if bar is None:
            continue
        bl, by, br = bar[1][:3]
        if br <= bl:                                       # the u32 wrap the reference tolerates is not a proposal
            continue
        found.append((l, t, r, b, bl, by, br, br - bl))
    found.sort(key=lambda p: (p[1], p[0], p[2], p[3]))
    labels = found[:MAX_LABELS]
    crops = np.full((len(labels), CROP_H, CROP_W), 255, np.uint8)
    for i, (l, t, r, b) in enumerate(p[:4] for p in labels):
        crops[i, :b - t, :r - l] = P[t:b, l:r]
    return dict(header=(len(labels), len(found), len(boxes), n_runs, 0), labels=labels, all=found, crops=crops)


def of_frame(frame_bgra):
    """The restatement on a whole BGRA frame: None when the oracle finds the map closed."""
    c = o.crop_to_map(frame_bgra, True)
    if c is None:
        return None
    brq = c["cropped_brq"]
    return scale_labels(o.ocr_preprocess(brq), o.find_scales_preprocess(brq, 0))
