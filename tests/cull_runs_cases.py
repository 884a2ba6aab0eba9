"""Crafted frames for the run rule of the sector cull (csrc/smh_cull_rule.h; tests/test_cull_runs_gpu.py): white runs placed as the blob's
candidate sees them.  The blob is the 2 x 2 seeds of tests/cull_chain_cases.py's arc cases at the anchor: dilated (a seed becomes a plus of
five pixels) its first pixel in raster order is (0, -1), get_centre puts the start point at (0.5, 0.5), and the culling scan counts offsets
from (0, 0) -- the seeds' own origin.  A bar of n seeds on row y is a run of n + 2 pixels on row y and runs of n pixels on rows y - 1 and
y + 1; every other white pixel of a frame is a candidate of its own, with the same runs at other offsets.

  tangent   bars of 40 and 70 px about ox = 0 on the rows oy = +-19 and +-35: tangent to the inner edge of the middle and of the outer
            annulus of T = 15 ([19, 34] and [35, 50]) -- a run that enters its annulus at both ends and leaves it in the middle
  across    bars on the rows oy = +-30 from ox = -45 to 45: through the outer annulus, the middle one and the outer one again, across ox = 0
  axis      bars on oy = 0 (with their dilation: oy = -1, 0, 1) to the right, where the units wrap at 359.9 degrees, and to the left
  border    two seeds at ox = 11, 12: on the rows above and below them a run of two pixels, the last pixel of one 32-column cell
            (ox = -20 .. 11) and the first of the next; with their neighbours one pixel to either side
  lengths   runs of 1, 2 and 33 pixels (a run longer than a cell), and two runs one pixel apart in one cell
  edges     the blob within 52 px of each corner of the map, bars beside it: the annuli are cut by the border
  blobs     the blob with an arc 40 px away (outer annulus of T = 15 alone), and with a second arc 26 px away (both)

Every case runs at the thresholds 15, 23 and 47 (every annulus by runs), 24 (the middle annulus [1, 25] pixel by pixel) and 48 (the outer
annulus [2, 50] pixel by pixel)."""
import collections
import functools

import numpy as np

import cull_chain_cases as CC
import lsd_cases as C

MAX_GAPS = (15, 23, 24, 47, 48)
SIZES = CC.SIZES
BLOB = [(0, 0), (1, 0), (0, 1), (1, 1)]

Case = collections.namedtuple("Case", "name anchor seeds runs")            # runs: [(ox0, ox1, oy)] white runs the mask must hold, from the blob
Ref = collections.namedtuple("Ref", "case lines rounds n_mask_px steps mask")


def _bar(x0, y, n):
    """n seeds from (x0, y) on -> (seeds, the three runs they dilate to)"""
    return C.hbar(x0, y, n), [(x0 - 1, x0 + n, y), (x0, x0 + n - 1, y - 1), (x0, x0 + n - 1, y + 1)]


@functools.lru_cache(maxsize=1)
def cases():
    cs = []

    def add(name, anchor, parts, origin=(0, 0)):
        seeds, runs = list(BLOB), []
        for s_, r_ in parts:
            seeds += s_
            runs += r_
        seeds = [(x + origin[0], y + origin[1]) for x, y in sorted(set(seeds))]
        cs.append(Case(name, anchor, np.array(seeds, int).reshape(-1, 2), [(a + origin[0], b + origin[0], y + origin[1]) for a, b, y in runs]))

    for oy in (19, -19, 35, -35):
        for n in (40, 70):
            add("tangent_%s%d_%d" % ("m" if oy < 0 else "p", abs(oy), n), "tile", [_bar(-(n - 2) // 2, oy, n - 2)])   # (n pixels on the row itself)
    for oy in (30, -30):
        add("across_%s30" % ("m" if oy < 0 else "p"), "tile", [_bar(-45, oy, 91)])
    add("axis_right", "tile", [_bar(22, 0, 40)])
    add("axis_left", "tile", [_bar(-61, 0, 40)])
    add("axis_right_thick", "tile", [_bar(22, -1, 40), _bar(22, 0, 40), _bar(22, 1, 40)])
    add("border", "tile", [_bar(11, 40, 2), _bar(10, 44, 2), _bar(12, 48, 2), _bar(11, -40, 2)])
    add("lengths", "tile", [_bar(-16, 40, 33), _bar(-35, 25, 1), _bar(30, 28, 2)])
    add("two_runs_one_cell", "tile", [_bar(20, 40, 2), _bar(23, 40, 2), _bar(-10, -38, 2), _bar(-7, -38, 2)])
    # the blob 10 px inside each corner, bars on the side that exists
    add("edge_tl", "tl", [_bar(-8, 38, 30), _bar(30, 2, 20)], (10, 10))
    add("edge_tr", "tr", [_bar(-20, 38, 28), _bar(-50, 2, 20)], (-12, 10))
    add("edge_bl", "bl", [_bar(-8, -38, 30), _bar(30, -2, 20)], (10, -12))
    add("edge_br", "br", [_bar(-20, -38, 28), _bar(-50, -2, 20)], (-12, -12))
    chain = {c.name: c for c in CC.cases()}
    for n in ("arc_outer_only", "arc_both"):
        cs.append(Case(n, chain[n].anchor, chain[n].seeds, []))
    return tuple(cs)


def frame(case, W, H):
    x, y, rw, rh = C.ROI[(W, H)]
    ax, ay = C.ANCHORS[case.anchor](rw, rh)
    f = C._blank((W, H)).copy()
    xs, ys = case.seeds[:, 0] + ax, case.seeds[:, 1] + ay
    assert xs.min() >= 1 and ys.min() >= 1 and xs.max() < rw - 1 and ys.max() < rh - 1, case.name
    f[y + ys, x + xs] = C.COLOURS[[c.name for c in cases()].index(case.name) % 3]
    return f


def check_mask(case, mask, size):
    """The oracle's mask holds the runs the case claims, as maximal runs, and the blob where the offsets count from."""
    _, _, rw, rh = C.ROI[size]
    ax, ay = C.ANCHORS[case.anchor](rw, rh)
    by_row = collections.defaultdict(list)
    for a, b, oy in case.runs:
        by_row[oy].append((a, b))
    for oy, rs in by_row.items():
        row = mask[ay + oy] == 255
        for a, b in rs:
            inside = row[ax + a:ax + b + 1].all()
            # (a run of a thick bar or of a neighbouring bar's dilation may continue it: then the claim is the containing run's)
            assert inside, (case.name, oy, a, b)
    if case.runs and case.anchor == "tile":
        blob = mask[ay - 1:ay + 3, ax - 1:ax + 3] == 255
        assert blob.sum() == 12 and not blob[0, 0] and blob[0, 1], (case.name, blob)


@functools.lru_cache(maxsize=None)
def reference(size, max_gap):
    """{name: Ref}: the oracle's record and mask of every case at a frame size and a threshold; the cases' claims asserted on its masks.
    Shared by a session's tests; nothing may write to it."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o

    def one(c):
        r = o.process_frame(frame(c, *size), stages=0x1, max_gap=max_gap, want_images=True)
        assert r["map_open"] == 1
        r["lsd"].setflags(write=False)
        check_mask(c, r["lsd"], size)
        return Ref(c, r["lines"], r["rounds"], r["n_mask_px"], r["steps"], r["lsd"])

    C._blank(size)
    with ThreadPoolExecutor(8) as ex:
        return {R_.case.name: R_ for R_ in ex.map(one, cases())}


def coded_table(exe, max_gap):
    """The condensed table as the device holds it, from tests/cull_runs_check.cpp's `codes`: (in_outer bool[105, 105], in_middle, units int
    object[105, 105] -- what a pixel's byte code stands for, folded)."""
    import subprocess
    rows = subprocess.run([exe, "codes", str(max_gap)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    ent = [ln.split() for ln in rows[1:]]
    full = (1 << CC.UNITS) - 1

    def units(code):
        if code == 0xFF:
            return full
        r = ((2 << (code >> 6)) - 1) << (code & 63)
        return (r | (r >> CC.UNITS)) & full

    return (np.array([[e[0] == "1" for e in ln] for ln in ent]), np.array([[e[1] == "1" for e in ln] for ln in ent]),
            np.array([[units(int(e[2:], 16)) for e in ln] for ln in ent], object))


def seen_units(mask, fx, fy, in_a, units):
    """The units the white pixels of an annulus can be seen by from the candidate whose start point lies in pixel (fx, fy): pixel by pixel."""
    h, w = mask.shape
    acc = 0
    for oy in range(-CC.R, CC.R + 1):
        for ox in range(-CC.R, CC.R + 1):
            if in_a[oy + CC.R, ox + CC.R] and 0 <= fy + oy < h and 0 <= fx + ox < w and mask[fy + oy, fx + ox] == 255:
                acc |= units[oy + CC.R, ox + CC.R]
    return acc
