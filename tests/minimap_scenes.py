"""Synthetic frames whose minimap rectangle is chosen, for the tests of everything that reads a heightmap through that rectangle.

synth.make_frame's terrain is noisy enough that the four walks of find_minimap (src/vision/find_minimap.rs:63-129) never stop on
it.  A stripe of one flat non-marker colour, 3 px thick and centred on ROI column c, has a middle column whose eight neighbours are
all the stripe's: the walk from the ROI's centre stops there (edginess 0) and finds the flat run it asks for along the stripe, so a
stripe at column l gives left = l + 1, one at column r gives right = r - 1, and the same for rows t and b.  A side without a stripe
walks to the ROI's own edge: 0, rw - 1, 0, rh - 1.  The stripes are painted over the marker lines (a line may not break the flat
run) and the scale bars are drawn again after them, so they stay as make_frame left them."""
import numpy as np

W, H = 1024, 768
STRIPE = (70, 80, 90)                                            # RGB; saturation far below a marker colour's
N_SCENES = 10
NO_ANCHORS = 4                                                   # the very flat scene: its line lies outside the rectangle, so its firing source is "none"


def roi():
    from squad_mortar_helper_amd import map_bounds
    return map_bounds(W, H)


def _specs(rw, rh):
    """(name, l, r, t, b, line) per open frame: stripe positions (None: that stripe is left out) and the marker line's end points."""
    cx, cy = rw // 2, rh // 2
    return [
        ("generic", 41, 322, 57, 533, (75, 95, 150, 240)),
        ("hugs the centre on the left", cx - 4, 330, 40, 560, (200, 60, 300, 250)),
        ("far sides are the ROI's edges", 60, None, 90, None, (80, 110, 160, 250)),
        ("very narrow", cx - 10, cx + 9, 30, 570, (30, 40, 140, 230)),
        ("very flat", 20, 340, cy - 7, cy + 8, (30, 40, 150, 220)),
        ("hugs the centre below, left side is the ROI's edge", None, 300, 100, cy + 3, (40, 120, 160, 270)),
        ("no stripes: the whole ROI", None, None, None, None, (50, 60, 150, 250)),
        ("generic, off centre", 120, 260, 200, 480, (130, 215, 160, 272)),
        ("near the ROI's edges", 5, rw - 6, 6, rh - 7, (30, 330, 160, 560)),
    ]


def designed_rect(spec, rw, rh):
    _, l, r, t, b, _ = spec
    return (0 if l is None else l + 1, rw - 1 if r is None else r - 1, 0 if t is None else t + 1, rh - 1 if b is None else b - 1)


def make_scenes(first_idx=4000):
    """-> (frames uint8 [N_SCENES, H, W, 4] BGRA, per-frame (scales_start_y, anchors) list for make_anchors, designed rectangles
    (left, right, top, bottom; None for the closed last frame), scene names).  Frame NO_ANCHORS has no anchors (no m/px)."""
    from squad_mortar_helper_amd import synth
    x, y, rw, rh = roi()
    specs = _specs(rw, rh)
    assert len(specs) == N_SCENES - 1
    frames = np.empty((N_SCENES, H, W, 4), np.uint8)
    anchors, rects, names = [], [], []
    colour = np.array(synth.TEAM_RGB[0], np.uint8)[::-1]
    stripe = np.array(STRIPE, np.uint8)[::-1]
    _, _, bars, _ = synth.scale_bar_layout(W, H)
    # find_scale_width looks round(20 / 640 * quadrant width) = 6 rows down from a label's anchor at this frame size; synth's anchors
    # lie 6 rows above their bars (made for 1080p, 15 rows), so the anchors here lie 3 rows above: the frames have a m/px
    labels = [(m, (xl + xr) // 2, yb - 3) for (m, xl, xr, yb) in bars]
    start_y = min(a[2] for a in labels)
    for i, spec in enumerate(specs):
        name, l, r, t, b, line = spec
        f, info = synth.make_frame(W, H, frame_idx=first_idx + i, n_lines=0)
        m = f[y:y + rh, x:x + rw, :3]                            # (a view: BGR)
        # a marker line with its blob, clear of the centre row and column
        p0, p1 = np.array(line[:2], float), np.array(line[2:], float)
        ts = np.linspace(0.0, 1.0, int(np.hypot(*(p1 - p0)) * 2) + 1)
        xs, ys = np.rint(p0[0] + (p1[0] - p0[0]) * ts).astype(int), np.rint(p0[1] + (p1[1] - p0[1]) * ts).astype(int)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m[ys + dy, xs + dx] = colour
        m[int(p0[1]) - 11:int(p0[1]) + 11, int(p0[0]) - 11:int(p0[0]) + 11] = colour
        lo_x, hi_x = min(line[0], line[2]) - 12, max(line[0], line[2]) + 12
        lo_y, hi_y = min(line[1], line[3]) - 12, max(line[1], line[3]) + 12
        assert (hi_x < rw // 2 - 1 or lo_x > rw // 2 + 1) and (hi_y < rh // 2 - 1 or lo_y > rh // 2 + 1), name
        for c in (l, r):
            if c is not None:
                assert 3 <= c - 1 and c + 1 <= rw - 4 and abs(c - rw // 2) >= 3, name
                m[:, c - 1:c + 2] = stripe
        for c in (t, b):
            if c is not None:
                assert 3 <= c - 1 and c + 1 <= rh - 4 and abs(c - rh // 2) >= 3, name
                m[c - 1:c + 2, :] = stripe
        ox, oy = rw // 2, rh // 2
        for (_, xl, xr, yb) in bars:                             # the scale bars as make_frame draws them
            m[oy + yb, ox + xl:ox + xr + 1] = 0
            m[oy + yb:oy + yb + 7, ox + xl] = 0
            m[oy + yb:oy + yb + 7, ox + xr] = 0
        frames[i] = f
        anchors.append((start_y, [] if i == NO_ANCHORS else labels))
        rects.append(designed_rect(spec, rw, rh))
        names.append(name)
    f, info = synth.make_frame(W, H, frame_idx=first_idx + N_SCENES - 1, map_open=False)
    frames[N_SCENES - 1] = f
    anchors.append((start_y, labels))
    rects.append(None)
    names.append("closed")
    return frames, anchors, rects, names
