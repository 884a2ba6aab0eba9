"""The inputs of the tests of the map view's layers (tests/test_render_layers_gpu.py, tests/test_render_layers_host.py): a list of
256 prims of both kinds around the tile borders and the window's last column and row, and the minima every case has to change in
the restatement for its comparison to mean something.  Pure numpy: nothing here touches the library."""
import numpy as np

import render_geometry_cases as G
import render_layers_ref as LR

f32 = np.float32
WINDOW = G.WINDOW                                                # 515 x 67: tile borders at x = 256, 512 and y = 32, 64
N_BELOW = 160                                                    # prims [0, 160) lie below the marker lines, [160, 256) on the foreground
COVERING, ENCLOSING = 0, 1                                       # list indices: the window's own rectangle, and one around it
NON_FINITE = {30: (LR.RECT, (np.nan, 5.0, 50.0, 50.0)), 90: (LR.RECT, (10.0, 10.0, np.inf, 20.0)), 170: (LR.LINE, (10.0, 10.0, -np.inf, 300.0)),
              230: (LR.LINE, (np.nan, 5.0, 50.0, 50.0)), 231: (LR.RECT, (np.nan, np.nan, np.nan, np.nan))}
THIN = {40: (300.0, 40.0, 301.0, 60.0), 41: (310.0, 45.0, 330.0, 46.0), 42: (320.25, 40.0, 321.75, 50.0)}   # 1 px wide, 1 px high, 1.5 wide


def edge_family():
    """(kind, (x0, y0, x1, y1)) in window coordinates: rectangle edges and line ends at every quarter pixel from -1.5 to +1.5 around
    the tile border x = 256, the tile border y = 32, and the window's last column (x = 515) and row (y = 67)."""
    ow, oh = WINDOW
    out = []
    for k, o in enumerate(G.OFFSETS):
        out.append((LR.RECT, (256 + o, 5 * k + 0.5, 256 + o + 7.0, 5 * k + 4.25)))            # left edge beside x = 256
        out.append((LR.RECT, (256 + o - 9.0, 5 * k + 1.0, 256 + o, 5 * k + 4.5)))             # right edge beside it
        out.append((LR.RECT, (ow + o - 6.0, 5 * k, ow + o, 5 * k + 4.0)))                     # right edge around the last column
        out.append((LR.RECT, (10 + 18 * k, 32 + o, 22 + 18 * k, 32 + o + 5.0)))               # top edge beside y = 32
        out.append((LR.RECT, (14 + 18 * k, 32 + o - 6.0, 23 + 18 * k, 32 + o)))               # bottom edge beside it
        out.append((LR.RECT, (270 + 18 * k, oh + o - 5.0, 281 + 18 * k, oh + o)))             # bottom edge around the last row
        out.append((LR.LINE, (256 + o - 12.0, 3 + 5 * k, 256 + o, 3 + 5 * k)))                # a line that ends beside x = 256
        out.append((LR.LINE, (ow + o - 12.0, 2 + 5 * k, ow + o, 2 + 5 * k)))                  # ... around the last column
        out.append((LR.LINE, (380 + 9 * k, 32 + o - 10.0, 380 + 9 * k, 32 + o)))              # ... beside y = 32
        out.append((LR.LINE, (30 + 9 * k, oh + o - 10.0, 30 + 9 * k, oh + o)))                # ... around the last row
    return out


def prim_list(view, seed=21):
    """256 prims in map-ROI coordinates that `view` brings to WINDOW: the window's own rectangle and one around it, the edge
    family, thin rectangles, three pairs that cross at the list indices G.PAIRS (the last prim a wave compacts and the first of the
    next), lines of zero length at G.ZERO_LENGTH, prims with Inf / NaN coordinates, and short random lines and small rectangles, an
    eighth of them with SMHV_PRIM_SHIFT1.  Prims from N_BELOW on are foreground ones, so with no marker lines the kernel's list
    has the list's order.  -> list of prim tuples."""
    ow, oh = WINDOW
    rng = np.random.default_rng(seed)
    fixed = {COVERING: (LR.RECT, (0.0, 0.0, float(ow), float(oh))), ENCLOSING: (LR.RECT, (-5.0, -5.0, ow + 5.0, oh + 5.0))}
    for i, w in THIN.items():
        fixed[i] = (LR.RECT, w)
    for (i, j), (cx, cy) in zip(G.PAIRS, G.PAIR_CENTRES):
        fixed[i] = (LR.LINE, (cx - 15, cy - 9, cx + 15, cy + 9))
        fixed[j] = (LR.LINE if i != 127 else LR.RECT, (cx - 15, cy + 9, cx + 15, cy - 9) if i != 127 else (cx, cy - 6, cx + 9, cy + 1))
    for i in G.ZERO_LENGTH:
        fixed[i] = (LR.LINE, (300.0 + i, 20.0, 300.0 + i, 20.0))
    fam = edge_family()
    rest = list(fam)
    while len(rest) + len(fixed) + len(NON_FINITE) < 256:
        x, y = rng.uniform(265.0, 500.0), rng.uniform(2.0, 60.0)
        if rng.integers(0, 2):
            a, ln = rng.uniform(0.0, 2 * np.pi), rng.uniform(3.0, 25.0)
            rest.append((LR.LINE, (x, y, x + ln * np.cos(a), y + ln * np.sin(a))))
        else:
            rest.append((LR.RECT, (x, y, x + rng.uniform(-20.0, 20.0), y + rng.uniform(-12.0, 12.0))))
    order = rng.permutation(len(rest))
    prims, k = [], 0
    for i in range(256):
        shift = 0
        if i in NON_FINITE:
            kind, w = NON_FINITE[i]
        elif i in fixed:
            kind, w = fixed[i]
        else:
            kind, w = rest[order[k]]
            k += 1
            shift = LR.SHIFT1 if rng.integers(0, 8) == 0 else 0
        with np.errstate(all="ignore"):
            c = view.from_window(w[0], w[1]) + view.from_window(w[2], w[3])   # (Inf stays Inf, NaN stays NaN)
        c = [float(f32(v)) for v in c]
        if i in G.ZERO_LENGTH:
            c[2:] = c[:2]
        rgba = tuple(int(v) for v in rng.integers(0, 256, 3)) + (255,)
        prims.append((c[0], c[1], c[2], c[3], rgba, kind | shift | (LR.FOREGROUND if i >= N_BELOW else 0)))
    assert k == len(rest) and len(prims) == 256
    return prims


def check_prim_list(prims, view):
    """What the list must do in the restatement for a comparison on it to mean something -> the prims' masks."""
    ow, oh = WINDOW
    masks = [LR.prim_mask(ow, oh, p, view.scale, view.top_left) for p in prims]
    edge = np.zeros((oh, ow), bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    assert np.array_equal(masks[COVERING], edge) and not masks[ENCLOSING].any()
    for i in G.ZERO_LENGTH:
        assert not masks[i].any(), i
    assert not masks[30].any() and not masks[230].any() and not masks[231].any() and masks[90].any() and masks[170].any()
    for (i, j), (cx, cy) in zip(G.PAIRS, G.PAIR_CENTRES):
        assert masks[i][cy, cx] and masks[j][cy, cx], (i, j)
    return masks


def views(rw, rh):
    return G.line_views(rw, rh)


# ---- what a case must change for its comparison to mean something ----------------------------------------------------------------
# Chosen on the CPU from the restatement (four fifths of the count it gives, rounded down), against the same render without the layer.
# The 256 prims over a plain ui_map, per view of views(): the pixels at least one prim paints.
PRIMS_MIN = {"identity": 6444, "zoom 10, far pan": 6444}
# The minimap bounds of the nine open scenes of tests/minimap_scenes.py, the frame's pixels inside the window: through the identity
# at the ROI's size, and through the "anisotropic" view of render_geometry_cases at WINDOW.
BOUNDS_MIN = {"identity": (1201, 1068, 1262, 884, 526, 784, 1505, 662, 1464), "anisotropic": (718, 436, 768, 129, 364, 716, 923, 363, 891)}
# A source at the identity viewport of its own size against the ui_map through the same options, over the open scenes, keyed by
# SMHV_VIEW_*: the gray planes and the isolated map differ from the colour terrain nearly everywhere, the bottom right quarter
# shows other texels than the top left one.
SOURCE_MIN = {1: 42048, 2: 42046, 3: 167146, 4: 168319, 5: 42014}


def marker_predicate(r8, g8, b8):
    """hsv + is_any_map_marker_color in vectorised numpy float32 -- the suite's second restatement of the marker predicate
    (tests/test_oracle_golden.py, written from util/src/image.rs:159-187 and vision-common/src/markers/mod.rs:17-54; shares no
    code with the library) -> bool array."""
    r, g, b = (np.asarray(v).astype(f32) / f32(255.0) for v in (r8, g8, b8))
    mx = np.maximum(r, np.maximum(g, b))
    mn = np.minimum(r, np.minimum(g, b))
    delta = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(mx == mn, f32(0.0),
                     np.where(mx == r, f32(60.0) * np.fmod((g - b) / delta, f32(6.0)),
                              np.where(mx == g, f32(60.0) * ((b - r) / delta + f32(2.0)), f32(60.0) * ((r - g) / delta + f32(4.0))))).astype(f32)
        s = (f32(100.0) * delta) / mx
    v = f32(100.0) * mx
    hm = np.fmod(h, f32(360.0))
    hm = np.where(hm < 0, hm + f32(360.0), hm)
    H = np.nan_to_num(hm, nan=0.0).astype(np.int64)
    S = np.nan_to_num(s, nan=0.0).astype(np.int64)
    V = v.astype(np.int64)
    hit = np.zeros(H.shape, bool)
    for mh, ms, mv in ((105, 100, 100), (285, 46, 85), (158, 60, 91)):
        sat_ok = (np.abs(ms - S) <= 15) | (np.abs(S - (ms - 50)) <= 15)
        hit |= (np.abs(mh - H) <= 15) & sat_ok & (np.abs(mv - V) <= 15)
    return hit & (S >= 35)


def changed(a, b):
    return G.changed(a, b)
