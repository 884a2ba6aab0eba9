"""Crafted cases of Vision::find_longest_line (mode 1 of k_lsd) at its decision boundaries (tests/test_longest_line_host.py,
tests/test_longest_line_gpu.py), in the idiom of tests/lsd_cases.py, whose helpers they reuse.

A case is a name, a family, a mask and a list of calls.  The mask is seeds painted into the marker-free frame (lsd_cases.frame's
recipe: every seed becomes a plus of five pixels), or no seeds at all; the reference mask is always the oracle's own lsd image of
that frame.  A call is (px, py, max_gap) in ROI coordinates, at most 16 per case.  check(P) is asserted on the REFERENCE only (the
C oracle, and the numpy walker below for per-ray quantities): it proves that the case still sits on its edge.  A case whose check
fails on the oracle is a broken case.

rays() is a third statement of the reference's ray walk (after oracle/smh_oracle.c and tests/independent_lsd.py, which the host
test holds it against bit for bit): it also reports, per ray, the step K at which the fatal gap started, the sample at which the
ray stopped, and takes the walk's rules as knobs (the host test's mutants).

Families ("What find_longest_line alone must get right"):
  short      the winner's gap starts at step K = 2 .. 66 (pass 1 keeps only K per ray, pass 2 re-walks the units within 2 of the
             largest K): horizontal, vertical, 45 and 30 degree bars from their first pixel and from that pixel + (0.5, 0.25); two
             bars from one start with K = k and k - 1 / k - 2 (pass 2's margin); a second-best ray of the same K in another unit.
             K = 1 cannot win on a dilated mask: every white pixel has a white 4-neighbour, so some axis ray has K >= 2.
  handover   rays that stop about sample 64 (phase A -> queue -> phase B): fatal gaps from step 62 .. 65, a 15 / 16 sample gap
             closed by white at sample 64 / 65 under max_gap 14, 15, 16, a gap that starts in batch 0 and is fatal in batch 1,
             one that starts in batch 1 and is fatal in phase B
  overflow   a filled disc of radius 80 and a filled 200 x 120 rectangle: more than LSD_QCAP rays alive after 64 samples from the
             centre, fewer from the rim, and a start that leaves the count within 8 of LSD_QCAP
  ties       bit-equal maxima in different 64-ray units: lsd_cases' diagonals from their get_centre point, plus-shaped crosses
             with arms of 70 (every tied ray finishes in phase B), 40 (pass 2), 70 / 40 (phase B; from the integer centre the two
             long arms' rays differ in the last bit and nothing ties) and 40 / 70 (two lanes of ONE unit tie), a start on black with
             no white in reach, the empty mask.  Bit-equal len² means equal K up to a step, so no cross ties a pass-2 ray with a
             phase-B ray; the tie between phases that exists is across the queue's capacity: a disc with two mirrored spokes, one
             tied ray queued for phase B, the other finished exactly where pass 1 found the queue full
  residency  ROWS / XWIN / GLOBAL by the mask's bounding box (mode_for restates lsd_mode_for): starts inside the box, one row /
             pixel outside the kept rows / word columns, at the ROI's corners and last row / column, and in GLOBAL two calls
             further apart than the row cache
  outside    starts outside the image next to white at that edge
  gaps       max_gap <= 0, fractional, 60000 and the next float, inf, NaN on a short and a handover case
  nonfinite  NaN / inf starts: every ray's len² is NaN and the answer is ray 3599's
"""
import collections
import functools
import os
import re

import numpy as np

import independent_lsd as ind
import lsd_cases as C
from lsd_cases import HD, QHD, ROI, SMALL, WIDE, diag, hbar, seg, vbar

f32 = np.float32
NAN, INF = float("nan"), float("inf")
GAP_NEXT_60000 = float(np.nextafter(f32(60000), f32(INF)))        # 60000.004: the first max_gap the batched walker does not take

Case = collections.namedtuple("Case", "name family anchor seeds calls check sizes modes")
Placed = collections.namedtuple("Placed", "case size mask calls ax ay")       # mask: the oracle's lsd image; calls: absolute ROI coordinates

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "squad-mortar-helper_amd", "csrc", "smh_lsd.hip")


@functools.lru_cache(maxsize=None)
def kernel_constant(name):
    """An integer #define of csrc/smh_lsd.hip."""
    m = re.search(r"^#define %s (\d+)u?\b" % name, open(_SRC).read(), re.M)
    assert m, name
    return int(m.group(1))


# ---- the ray walk, with its rules as knobs -------------------------------------------------------------------------------------

Rays = collections.namedtuple("Rays", "xe ye len2 K stop aborted")     # per ray; K: step at which the last gap began; stop: the sample it aborted at / first position outside


def _cast(v, wrap):
    """Rust's `f32 as u32` (saturating, NaN -> 0); wrap: through i64 and truncated to 32 bits instead, as a C cast chain would."""
    if not wrap:
        return ind._as_u32(v)
    t = np.trunc(np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    return np.mod(t, 4294967296.0).astype(np.int64)


def rays(img, px, py, max_gap, abort_gt=False, no_restore=False, end_at_x=False, wrap_cast=False, floor_T=False, short_mul=False):
    """All 3600 rays of one start point.  All knobs off: vision-cpu/src/lib.rs:388-432."""
    h, w = img.shape
    DX, DY = ind.DX, ind.DY
    n = len(DX)
    xs, ys = f32(px), f32(py)
    x = np.full(n, xs, f32); y = np.full(n, ys, f32)
    xo = np.zeros(n, f32); yo = np.zeros(n, f32)
    g0 = np.zeros(n, f32); g1 = np.zeros(n, f32); g2 = np.zeros(n, f32)
    K = np.zeros(n, np.int64); stop = np.zeros(n, np.int64); aborted = np.zeros(n, bool)
    walking = np.ones(n, bool)
    mg = f32(max_gap)
    if floor_T:
        mg = f32(np.floor(mg) + f32(1))
    it = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            inside = (x >= 0) & (y >= 0) & (x < f32(w)) & (y < f32(h))
            stop[walking & ~inside] = it
            walking &= inside
            if not walking.any():
                break
            idx = np.nonzero(walking)[0]
            white = img[y[idx].astype(np.int64), x[idx].astype(np.int64)] == 255
            gi = g0[idx]
            abort = ~white & ((gi > mg) if abort_gt else (gi >= mg))
            first = ~white & ~abort & (gi == 0)
            more = ~white & ~abort & (gi != 0)
            g0[idx[white]] = 0; g1[idx[white]] = 0; g2[idx[white]] = 0
            ia = idx[abort]
            if not no_restore:
                x[ia] = g1[ia]; y[ia] = g2[ia]
            walking[ia] = False; aborted[ia] = True; stop[ia] = it
            i1 = idx[first]
            g0[i1] = 1; g1[i1] = x[i1]; g2[i1] = y[i1]; K[i1] = it
            g0[idx[more]] += f32(1)
            ic = idx[~abort]
            xo[ic] = xo[ic] + DX[ic]; yo[ic] = yo[ic] + DY[ic]
            x[ic] = xo[ic] + xs; y[ic] = yo[ic] + ys
            it += 1
        xi, yi = _cast(x, wrap_cast), _cast(y, wrap_cast)
        ok = (xi < w) & (yi < h)
        zero = np.zeros(n, bool)
        zero[ok] = img[yi[ok], xi[ok]] == 0
        xe = np.where(zero, x if end_at_x else x - DX, xs).astype(f32); ye = np.where(zero, y if end_at_x else y - DY, ys).astype(f32)
        if short_mul:                       # what pass 1 knows of a short ray: K - 1 unit steps from the start
            s = aborted & zero & (K >= 1) & (K <= 49)
            xe[s] = (xs + (K[s] - 1).astype(f32) * DX[s]).astype(f32); ye[s] = (ys + (K[s] - 1).astype(f32) * DY[s]).astype(f32)
        ddx = (xs - xe).astype(f32); ddy = (ys - ye).astype(f32)
        len2 = (ddx * ddx + ddy * ddy).astype(f32)
    return Rays(xe, ye, len2, K, stop, aborted)


def winner(R, first=False):
    """The reduce of lib.rs:434-447: `if a.len > b.len { a } else { b }` in index order -- the LAST maximum, and with NaN lengths the last ray."""
    best, bl = 0, f32(0)
    if np.isnan(R.len2).any():
        for i in range(len(R.len2)):
            if not (bl > R.len2[i]):
                best, bl = i, R.len2[i]
        return best
    m = np.nonzero(R.len2 == R.len2.max())[0]
    return int(m[0 if first else -1])


def longest(img, px, py, max_gap, first_max=False, **knobs):
    R = rays(img, px, py, max_gap, **knobs)
    i = winner(R, first_max)
    return np.array([f32(px), f32(py), R.xe[i], R.ye[i]], f32), R.len2[i]


def alive_after(R, samples=64):
    """Rays that have taken `samples` samples inside the image without aborting: what pass 1 hands to the queue."""
    return int((R.stop >= samples).sum())


def same(a, b):
    """(line, len²) pairs equal bit for bit, NaN equal to NaN."""
    return np.array_equal(np.asarray(a[0], f32), np.asarray(b[0], f32), equal_nan=True) and (a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1])))


# ---- residency -----------------------------------------------------------------------------------------------------------------

ROWS, XWIN, GLOBAL = "ROWS", "XWIN", "GLOBAL"


def geometry(size):
    """(bits_pitch_w, m_xoff) of a frame size: smh_runtime.cpp's geometry of the bit-packed mask rows."""
    rx, _, rw, _ = ROI[size]
    xoff = rx & 3
    quads = (rw + xoff + 3) // 4
    return ((quads + 15) & ~15) // 8, xoff


def box(mask, size):
    """(y_min, y_max, w_min, w_max) of the white pixels: rows, and words of the bit-packed rows (FrameAux)."""
    _, xoff = geometry(size)
    ys, xs = np.nonzero(mask)
    return int(ys.min()), int(ys.max()), int((xs.min() + xoff) >> 5), int((xs.max() + xoff) >> 5)


def mode_for(mask, size):
    """lsd_mode_for (csrc/smh_lsd.hip) restated: only the bounding box of the mask decides."""
    cap = kernel_constant("LSD_WIN_WORDS_CAP")
    if not mask.any():
        return GLOBAL
    gp, _ = geometry(size)
    y0, y1, w0, w1 = box(mask, size)
    wrows, wwords = y1 - y0 + 1, w1 - w0 + 1
    if (wrows + 2) * (gp | 1) + 4 <= cap:
        return ROWS
    if (wrows + 2) * ((wwords + 2) | 1) <= cap:
        return XWIN
    return GLOBAL


def cache_rows(size):
    """Rows of GLOBAL's LDS row cache (frame_setup: c_cap_rows)."""
    gp, _ = geometry(size)
    return min(ROI[size][3], kernel_constant("LSD_WIN_WORDS_CAP") // (gp | 1))


def in_box(P, px, py):
    """Is the start inside the rows and word columns that hold white (what ROWS and XWIN keep in LDS)?  Never, on an empty mask."""
    if not P.mask.any():
        return False
    y0, y1, w0, w1 = box(P.mask, P.size)
    _, xoff = geometry(P.size)
    return y0 <= py <= y1 and w0 * 32 - xoff <= px < (w1 + 1) * 32 - xoff


# ---- checks --------------------------------------------------------------------------------------------------------------------

def _oracle(P, k):
    from oracle import oracle as o
    px, py, gap = P.calls[k]
    return o.find_longest_line(P.mask, px, py, gap)


def _rays_of(P, k):
    px, py, gap = P.calls[k]
    return rays(P.mask, px, py, gap)


def _winner_K(*ks):
    """Call j's winning ray aborted, and its fatal gap began at step ks[j] (None: not looked at)."""
    def check(P):
        for j, k in enumerate(ks):
            if k is None:
                continue
            R = _rays_of(P, j)
            i = winner(R)
            assert R.aborted[i] and R.K[i] == k, (P.case.name, j, i, int(R.K[i]), k)
            line, l2 = _oracle(P, j)
            assert (line[2], line[3], l2) == (R.xe[i], R.ye[i], R.len2[i]), (P.case.name, j)
    return check


def _winner_K_stop(spec):
    """spec[j] = (K, stop, alive): call j's winner began its last gap at step K and aborted at sample `stop`; alive: it took 64 samples (queued)."""
    def check(P):
        for j, (k, stop, alive) in enumerate(spec):
            R = _rays_of(P, j)
            i = winner(R)
            assert R.aborted[i] and (int(R.K[i]), int(R.stop[i]), bool(R.stop[i] >= 64)) == (k, stop, alive), (P.case.name, j, i, int(R.K[i]), int(R.stop[i]), spec[j])
    return check


def _two_bars(k, d):
    """The winner has K = k; the best ray of another 64-ray unit has K = k - d, and that unit holds no ray of K > k - d."""
    def check(P):
        R = _rays_of(P, 0)
        i = winner(R)
        assert R.aborted[i] and R.K[i] == k, (P.case.name, i, int(R.K[i]))
        unit = np.arange(len(R.K)) // 64
        kmax = np.array([R.K[(unit == u) & R.aborted].max(initial=0) for u in range(57)])
        assert (kmax == k - d).any() and kmax[unit[i]] == k, (P.case.name, kmax)
    return check


def _same_K_other_unit(P):
    """The winner and the best ray of some other unit have the same K: only the exact len² tells them apart."""
    R = _rays_of(P, 0)
    i = winner(R)
    unit = np.arange(len(R.K)) // 64
    others = R.aborted & (unit != unit[i]) & (R.K == R.K[i])
    assert R.aborted[i] and others.any() and R.len2[others].max() < R.len2[i], (P.case.name, i, int(R.K[i]))
    assert R.K[R.aborted].max() == R.K[i], P.case.name


def _alive(spec):
    """spec[j] = (lo, hi): the number of call j's rays still alive after 64 samples lies in [lo, hi]."""
    def check(P):
        for j, (lo, hi) in enumerate(spec):
            a = alive_after(_rays_of(P, j))
            assert lo <= a <= hi, (P.case.name, j, a, lo, hi)
    return check


def _tie(min_units=2, phase=None):
    """Call 0's maximum is held bit-equal by rays of at least two 64-ray units, the last one's end point is the oracle's and differs from
    the first one's.  phase: "B" every tied ray took 64 samples (queue, phase B), "2" none did and all aborted (pass 2), "mixed" both kinds."""
    def check(P):
        R = _rays_of(P, 0)
        t = np.nonzero(R.len2 == R.len2.max())[0]
        assert len(set(int(i) // 64 for i in t)) >= min_units, (P.case.name, t)
        line, l2 = _oracle(P, 0)
        assert (line[2], line[3]) == (R.xe[t[-1]], R.ye[t[-1]]) and (line[2], line[3]) != (R.xe[t[0]], R.ye[t[0]]), (P.case.name, t)
        q = R.stop[t] >= 64
        if phase == "B":
            assert q.all(), (P.case.name, R.stop[t])
        elif phase == "2":
            assert not q.any() and R.aborted[t].all(), (P.case.name, R.stop[t])
        elif phase == "mixed":
            assert q.any() and not q.all(), (P.case.name, R.stop[t])
    return check


def _tie_across_the_queue(P):
    for j in range(len(P.calls)):
        R = _rays_of(P, j)
        t = np.nonzero(R.len2 == R.len2.max())[0]
        qcap = kernel_constant("LSD_QCAP")
        assert alive_after(R) > qcap and t[0] < qcap <= t[-1], (P.case.name, j, t)
        assert (_oracle(P, j)[0][2], _oracle(P, j)[0][3]) == (R.xe[t[-1]], R.ye[t[-1]]), (P.case.name, j)


def _all_rays_alike(P):
    """No white within reach: every ray aborts with the same K (0: the start is black) and ends one step behind the start, so len² is
    |d|² to a rounding; the oracle's answer is the last of the maxima."""
    for j in range(len(P.calls)):
        R = _rays_of(P, j)
        a = R.aborted                       # (from a start on the ROI's edge some rays leave at once: they end where they started)
        assert a.sum() >= 850 and (R.K[a] == 0).all() and (np.abs(R.len2[a] - 1) < 1e-3).all() and (R.len2[~a] < 1e-3).all(), (P.case.name, j)
        i = winner(R)
        line, l2 = _oracle(P, j)
        assert (line[2], line[3], l2) == (R.xe[i], R.ye[i], R.len2[i]) and l2 == R.len2.max(), (P.case.name, j)


def in_image(P, j):
    px, py, _ = P.calls[j]
    h, w = P.mask.shape
    return 0 <= px < w and 0 <= py < h


def _nonfinite(P):
    for j in range(len(P.calls)):
        R = _rays_of(P, j)
        assert np.isnan(R.len2).all(), (P.case.name, j)
        line, l2 = _oracle(P, j)
        assert np.isnan(l2) and np.array_equal(line[2:], np.array([R.xe[3599], R.ye[3599]], f32), equal_nan=True), (P.case.name, j, line)


def _white_next_to(*edges):
    def check(P):
        m = P.mask
        for e in edges:
            assert {"left": m[:, 0], "right": m[:, -1], "top": m[0], "bottom": m[-1]}[e].any(), (P.case.name, e)
        for j in range(len(P.calls)):
            if not in_image(P, j):
                assert _oracle(P, j)[1] >= 0            # a number: finite starts
    return check


def _edges_of_the_box(P):
    """White sits on the first and last kept row and on the first and last pixel of the first / last kept word column."""
    y0, y1, w0, w1 = box(P.mask, P.size)
    _, xoff = geometry(P.size)
    ys, xs = np.nonzero(P.mask)
    assert xs.min() == w0 * 32 - xoff and xs.max() == (w1 + 1) * 32 - xoff - 1, (P.case.name, xs.min(), xs.max(), w0, w1)


def _both(*checks):
    def check(P):
        for c in checks:
            c(P)
    return check


# ---- the cases -----------------------------------------------------------------------------------------------------------------

SHORT_KS = (2, 3, 31, 32, 33, 48, 49, 50, 51, 63, 64, 65, 66)


def _bar(kind, n):
    """Seeds of a bar of n steps from the anchor, and its first white pixel (where the calls start)."""
    if kind == "h":
        return hbar(1, 0, n), (0.0, 0.0)
    if kind == "v":
        return vbar(0, 1, n), (0.0, 0.0)
    if kind == "d45":
        return diag(0, 1, n), (0.0, 0.0)              # seeds (i, 1 + i): the plus of the first one reaches (0, 0)
    return seg(1, 1, 30.0, n), (0.0, 1.0)


def design_short(kind, ks=SHORT_KS, nmax=90):
    """(Design time.)  {K: n}: the shortest bar of each kind whose winner from the first pixel has K, on the dilated seeds at the tile anchor."""
    out = {}
    for n in range(1, nmax):
        seeds, (sx, sy) = _bar(kind, n)
        m = synthetic_mask(seeds, SMALL, "tile")
        ax, ay = C.ANCHORS["tile"](*ROI[SMALL][2:])
        R = rays(m, ax + sx, ay + sy, 15.0)
        i = winner(R)
        if R.aborted[i] and int(R.K[i]) in ks and int(R.K[i]) not in out:
            out[int(R.K[i])] = n
    return out


def synthetic_mask(seeds, size, anchor):
    """The seeds' dilation by the cross, clipped to the ROI: what the oracle's mask of the frame is (asserted by the host test)."""
    _, _, rw, rh = ROI[size]
    ax, ay = C.ANCHORS[anchor](rw, rh)
    m = np.zeros((rh, rw), np.uint8)
    s = np.asarray(seeds, np.int64).reshape(-1, 2)
    for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
        xs, ys = s[:, 0] + ax + dx, s[:, 1] + ay + dy
        ok = (xs >= 0) & (xs < rw) & (ys >= 0) & (ys < rh)
        m[ys[ok], xs[ok]] = 255
    return m


# design_short()'s answers: kind -> {K: seeds}.  The winner is seldom the bar's own axis ray (a slightly tilted one runs a step further
# through the three-pixel-thick bar), and on the slanted bars K jumps, so not every K has a length there; every K of SHORT_KS is held by
# some bar (K = 2 and 3 by a single plus).  The host test asserts every K again on the oracle's mask, at every size.
BAR_LEN = {
    "h": {31: 28, 32: 29, 33: 30, 48: 45, 49: 46, 50: 47, 51: 48, 63: 60, 64: 61, 65: 62, 66: 63},
    "v": {31: 28, 32: 29, 33: 30, 48: 45, 49: 46, 50: 47, 51: 48, 63: 60, 64: 61, 65: 62, 66: 63},
    "d45": {32: 21, 33: 22, 49: 33, 50: 34, 51: 35, 63: 43, 64: 44, 66: 45},
    "d30": {31: 28, 32: 29, 48: 45, 49: 46, 50: 47, 51: 48, 64: 60, 65: 62, 66: 63},
}


def _disc(r):
    return [(i, j) for i in range(-r, r + 1) for j in range(-r, r + 1) if i * i + j * j <= r * r]


def _rect(w, h):
    return [(i, j) for i in range(-(w // 2), w - w // 2) for j in range(-(h // 2), h - h // 2)]


def _cross(ah, av):
    return hbar(-ah, 0, 2 * ah + 1) + vbar(0, -av, 2 * av + 1)


GAPS = (-1.0, 0.0, 0.25, 0.5, 1.0, 1.5, 14.5, 15.0, 15.5, 60000.0, GAP_NEXT_60000, INF, NAN)
BOTH = (SMALL, HD)

# residency layout at 2560 x 1440 (ROI 1314 x 1096, m_xoff 3: word c holds pixels 32 c - 3 .. 32 c + 28)
Q_X0, Q_X1 = 32 * 10 - 3, 32 * 22 - 3 - 1          # first pixel of word 10, last pixel of word 21


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, family, seeds, calls, check=None, anchor="tile", sizes=BOTH, modes=None):
        s = np.array(sorted(set(map(tuple, seeds)), key=lambda q: (q[1], q[0])), np.int64).reshape(-1, 2)
        s.setflags(write=False)
        assert name not in [c.name for c in out], name
        assert callable(calls) or 1 <= len(calls) <= 16, name
        out.append(Case(name, family, anchor, s, calls, check, tuple(sizes), modes or {}))

    # -- short
    for kind in ("h", "v", "d45", "d30"):
        for K, n in sorted(BAR_LEN[kind].items()):
            seeds, (sx, sy) = _bar(kind, n)
            add("short_%s_K%d" % (kind, K), "short", seeds, [(sx, sy, 15.0), (sx + 0.5, sy + 0.25, 15.0)], _winner_K(K, None))
    add("short_plus_K2", "short", [(0, 0)], [(0.5, 0.5, 15.0), (0.25, 0.5, 15.0)], _winner_K(2, None))
    add("short_plus_K3", "short", [(0, 0)], [(0.0, 0.0, 15.0), (1.0, 0.0, 15.0), (0.0, 1.0, 15.0)], _winner_K(3, 3, 3))
    add("short_plus_K4", "short", [(0, 0)], [(1.9, 0.9, 15.0)], _winner_K(4))
    for k in (20, 40, 49, 50):
        # two bars from one start: along x with K = k, along y with K = k - 1 / k - 2 (other units: 90 degrees apart)
        for d in (1, 2):
            add("short_two_bars_K%d_minus_%d" % (k, d), "short", hbar(1, 0, k - 3) + vbar(0, 1, k - 3 - d), [(0.0, 0.0, 15.0)], _two_bars(k, d))
    # two bars of one length from a fractional start: the best rays of two units have the same K, and the exact len² decides
    for k in (49, 50):
        add("short_same_K%d_other_unit" % k, "short", hbar(-(k - 2), 0, 2 * (k - 2) + 1), [(0.5, 0.25, 15.0)], _same_K_other_unit)
    for k in (30, 39):
        add("short_same_K%d_other_unit" % k, "short", hbar(1, 0, k - 2) + vbar(0, -(k - 2), k - 2), [(0.5, 0.25, 15.0)], _same_K_other_unit)

    # -- handover: horizontal bars.  The winner is a ray a degree or less off the axis: its k-th sample lies a little short of k px, so it
    # still finds white at step n + 2 of a bar of n seeds and its gap starts at step n + 3
    def gapped(a, gap, tail=12):
        return hbar(1, 0, a - 2) + hbar(a + gap + 1, 0, tail)
    for a in (62, 63, 64, 65):
        add("hand_fatal_from_%d" % a, "handover", hbar(1, 0, a - 3), [(0.0, 0.0, 15.0)], _winner_K_stop([(a, a + 15, True)]))
    add("hand_white_again_at_64", "handover", gapped(48, 15), [(0.0, 0.0, 14.0), (0.0, 0.0, 15.0), (0.0, 0.0, 16.0)],
        _winner_K_stop([(49, 63, False), (78, 93, True), (78, 94, True)]))
    add("hand_white_again_at_65", "handover", gapped(48, 16), [(0.0, 0.0, 15.0), (0.0, 0.0, 16.0), (0.0, 0.0, 17.0)],
        _winner_K_stop([(49, 64, True), (79, 95, True), (79, 96, True)]))
    add("hand_batch0_to_batch1", "handover", hbar(1, 0, 17), [(0.0, 0.0, 15.0), (0.0, 0.0, 31.0), (0.0, 0.0, 40.0)],
        _winner_K_stop([(20, 35, False), (20, 51, False), (20, 60, False)]))
    add("hand_batch1_to_phase_b", "handover", hbar(1, 0, 52), [(0.0, 0.0, 15.0), (0.0, 0.0, 8.0), (0.0, 0.0, 9.0), (0.0, 0.0, 31.0), (0.0, 0.0, 40.0)],
        _winner_K_stop([(55, 70, True), (55, 63, False), (55, 64, True), (55, 86, True), (55, 95, True)]))
    add("hand_batch0_to_phase_b", "handover", hbar(1, 0, 27), [(0.0, 0.0, 33.0), (0.0, 0.0, 34.0), (0.0, 0.0, 49.0), (0.0, 0.0, 50.0)],
        _winner_K_stop([(30, 63, False), (30, 64, True), (30, 79, True), (30, 80, True)]))

    # -- overflow.  Calls: the centre, the centre + (0.5, 0.5), 70 px off centre (all above the queue's capacity), a start below it, and starts that
    # leave the count within 8 of it on either side (found on the walker by moving the start along the radius: 1027 and 1019 for the disc, 1027 and
    # 1015 for the rectangle).  From the disc's own rim 1480 rays are alive -- the chords of 64 px and more span 133 degrees -- so its start below the
    # capacity lies on black 11 px outside the rim (857); the rectangle's is its corner (923).
    qcap = kernel_constant("LSD_QCAP")
    add("over_disc_80", "overflow", _disc(80), [(0.0, 0.0, 15.0), (0.5, 0.5, 15.0), (70.0, 0.0, 15.0), (92.0, 0.0, 15.0), (90.375, 0.25, 15.0), (90.125, 2.0, 15.0),
                                               (80.0, 0.0, 15.0)],
        _alive([(qcap + 1, 3600), (qcap + 1, 3600), (qcap + 1, 3600), (1, qcap - 1), (qcap + 1, qcap + 8), (qcap - 8, qcap - 1), (qcap + 1, 3600)]))
    add("over_rect_200x120", "overflow", _rect(200, 120), [(0.0, 0.0, 15.0), (0.5, 0.5, 15.0), (70.0, 0.0, 15.0), (-100.0, -60.0, 15.0), (5.0, 70.375, 15.0), (5.0, 70.5, 15.0)],
        _alive([(qcap + 1, 3600), (qcap + 1, 3600), (qcap + 1, 3600), (1, qcap - 1), (qcap + 1, qcap + 8), (qcap - 16, qcap - 1)]))

    # -- ties
    for c in C.cases():
        if c.family == "ties":
            add("tie_" + c.name[4:], "ties", [tuple(q) for q in c.seeds.tolist()], _centre_call(c.seeds), _tie())
    add("tie_cross_70", "ties", _cross(70, 70), [(0.0, 0.0, 15.0), (0.5, 0.5, 15.0)], _tie(2, "B"))
    add("tie_cross_40", "ties", _cross(40, 40), [(0.0, 0.0, 15.0), (0.5, 0.5, 15.0)], _tie(2, "2"))
    add("tie_cross_70_40", "ties", _cross(70, 40), [(0.5, 0.5, 15.0), (0.0, 0.0, 15.0)], _tie(2, "B"))      # (from (0, 0) rays 1 and 3599 differ in the last bit: no tie)
    add("tie_cross_40_70", "ties", _cross(40, 70), [(0.5, 0.5, 15.0), (0.0, 0.0, 15.0)], _tie(1, "B"))      # (rays 896 and 904: two lanes of ONE unit hold the maximum)
    # a tie across the queue's capacity: a disc that keeps all 3600 rays alive for 64 samples, and two spokes that mirror each other in the ROI's
    # diagonal, at -6 and 96 degrees.  The queue holds 1024 rays -- sixteen units' worth; the waves take units 0 .. 15 first -- so one tied ray
    # (959 / 961, unit 14 / 15) finishes in phase B and the other (3541 / 3539, unit 55) where pass 1 found the queue full
    spoke = seg(0, 0, -6.0, 140)
    add("tie_disc_spokes", "ties", _disc(80) + spoke + [(y, x) for x, y in spoke], [(0.0, 0.0, 15.0), (0.5, 0.5, 15.0)], _both(_tie(2, "B"), _tie_across_the_queue))
    add("tie_black_no_white_in_reach", "ties", hbar(-150, -150, 5), [(0.0, 0.0, 15.0), (0.5, 0.25, 15.0), (100.0, 200.0, 3.0)], _all_rays_alike)
    add("tie_empty_mask", "ties", [], lambda rw, rh, ax, ay: [(160.0, 160.0, 15.0), (160.5, 160.25, 15.0), (0.0, 0.0, 15.0), (rw - 1.0, rh - 1.0, 15.0), (rw / 2.0, 3.0, 1.0)],
        _all_rays_alike, sizes=(SMALL, HD, QHD), modes={s: GLOBAL for s in (SMALL, HD, QHD)})

    # -- residency (2560 x 1440)
    def probes(extra=()):
        def calls(rw, rh, ax, ay):
            return [(px + ax, py + ay, g) for px, py, g in extra] + [(0.0, 0.0, 15.0), (rw - 1.0, 0.0, 15.0), (0.0, rh - 1.0, 15.0), (rw - 1.0, rh - 1.0, 15.0), (rw - 0.5, rh - 0.5, 15.0),
                                  (rw - 1.0, rh / 2.0, 15.0), (rw / 2.0, rh - 1.0, 15.0)]
        return calls
    # ROWS: rows 300 .. 800; white on the first pixel of word 10 and the last pixel of word 21, on the first and the last row
    rows_seeds = hbar(Q_X0 + 1, 301, 60) + hbar(Q_X1 - 60, 799, 60) + vbar(Q_X0 + 1, 301, 70) + vbar(Q_X1 - 1, 730, 70) + seg(Q_X0 + 40, 340, 55.0, 540)
    add("res_rows", "residency", rows_seeds,
        probes([(Q_X0 + 30.0, 300.0, 15.0), (Q_X0 + 200.5, 531.25, 15.0), (Q_X0 + 20.0, 299.0, 15.0), (Q_X1 - 20.0, 801.0, 15.0), (Q_X0 - 1.0, 330.0, 15.0),
                (Q_X1 + 1.0, 760.0, 15.0), (Q_X0 + 20.0, 290.0, 15.0), (Q_X1 - 20.0, 812.0, 15.0), (Q_X0 - 10.0, 330.0, 15.0)]),
        _edges_of_the_box, anchor="tl", sizes=(QHD,), modes={QHD: ROWS})
    # XWIN: rows 100 .. 1000, words 10 .. 21
    xwin_seeds = hbar(Q_X0 + 1, 101, 60) + hbar(Q_X1 - 60, 999, 60) + vbar(Q_X0 + 1, 101, 70) + vbar(Q_X1 - 1, 930, 70) + seg(Q_X0 + 40, 140, 70.0, 900)
    add("res_xwin", "residency", xwin_seeds,
        probes([(Q_X0 + 30.0, 100.0, 15.0), (Q_X0 + 200.5, 600.25, 15.0), (Q_X0 + 20.0, 99.0, 15.0), (Q_X1 - 20.0, 1001.0, 15.0), (Q_X0 - 1.0, 130.0, 15.0),
                (Q_X1 + 1.0, 960.0, 15.0), (Q_X0 + 20.0, 90.0, 15.0), (Q_X1 - 20.0, 1012.0, 15.0), (Q_X0 - 10.0, 130.0, 15.0)]),
        _edges_of_the_box, anchor="tl", sizes=(QHD,), modes={QHD: XWIN})
    # GLOBAL: two shapes in opposite corners of the ROI; consecutive calls further apart than the row cache
    glob_seeds = hbar(1, 1, 80) + vbar(1, 1, 80) + diag(5, 5, 90) + [(1314 - 2 - i, 1096 - 2) for i in range(80)] + [(1314 - 2, 1096 - 2 - i) for i in range(80)] + \
        [(1314 - 6 - i, 1096 - 6 - i) for i in range(90)]
    add("res_global", "residency", glob_seeds,
        probes([(40.0, 40.0, 15.0), (1314 - 41.0, 1096 - 41.0, 15.0), (30.5, 30.25, 15.0), (1314 - 30.5, 1096 - 30.25, 15.0), (600.0, 548.0, 15.0), (4.0, 100.0, 15.0),
                (1314 - 5.0, 950.0, 15.0), (700.0, 5.0, 15.0), (-2.0, 50.0, 15.0)]),
        _white_next_to("left", "top", "right", "bottom"), anchor="tl", sizes=(QHD,), modes={QHD: GLOBAL})
    # the corners again wherever the ROI ends: all four sizes (ROI column 2048 and beyond at 3440 x 1440)
    add("res_corners", "residency", hbar(1, 1, 60) + vbar(1, 1, 60), probes([(1.0, 1.0, 15.0)]), _white_next_to("left", "top"), anchor="tl", sizes=C.SIZES)
    add("res_corner_br", "residency", hbar(-61, -1, 60) + vbar(-1, -61, 60) + diag(-70, -70, 66), probes([(-1.0, -1.0, 15.0)]), _white_next_to("right", "bottom"),
        anchor="br", sizes=C.SIZES)
    add("res_col_2048", "residency", hbar(-70, 0, 140) + vbar(0, -70, 140), [(0.0, 0.0, 15.0), (-0.5, 0.25, 15.0), (-69.0, 0.0, 15.0), (70.0, 0.0, 15.0), (0.0, -70.0, 15.0)],
        None, anchor="col2048", sizes=(WIDE,))

    # -- outside
    add("out_top_left", "outside", hbar(1, 1, 40) + vbar(1, 1, 40) + diag(2, 2, 45), lambda rw, rh, ax, ay: [(-0.25, 10.0, 15.0), (10.0, -3.0, 15.0), (-0.25, -0.25, 15.0), (-3.0, 20.0, 15.0),
                                                                                                  (-1.5, 5.0, 15.0), (-3.0, 20.0, 0.0), (30.0, -3.0, NAN), (-2.0, 300.0, 15.0)],
        _white_next_to("left", "top"), anchor="tl")
    add("out_bottom_right", "outside", hbar(-41, -1, 40) + vbar(-1, -41, 40) + diag(-47, -47, 45),
        lambda rw, rh, ax, ay: [(float(rw), rh - 10.0, 15.0), (rw + 5.0, rh + 1.0, 15.0), (rw - 10.0, float(rh), 15.0), (rw + 5.0, rh - 20.0, 15.0), (rw - 20.0, rh + 1.0, 0.5),
                        (float(rw), float(rh), INF)],
        _white_next_to("right", "bottom"), anchor="br")

    # -- gaps
    add("gaps_short_K33", "gaps", hbar(1, 0, 31), [(0.0, 0.0, g) for g in GAPS])
    add("gaps_handover_K64", "gaps", gapped(64, 15), [(0.0, 0.0, g) for g in GAPS])
    add("gaps_fractional_start", "gaps", gapped(49, 15) + vbar(0, 1, 30), [(0.5, 0.25, g) for g in GAPS])

    # -- nonfinite
    add("nonfinite_starts", "nonfinite", hbar(1, 1, 40) + vbar(1, 1, 40), [(NAN, 10.0, 15.0), (10.0, NAN, 15.0), (INF, 10.0, 15.0), (-INF, -INF, 15.0), (NAN, NAN, 15.0),
                                                                       (10.0, -INF, 0.0), (NAN, 10.0, NAN)],
        _nonfinite, anchor="tl", sizes=(SMALL, HD))
    add("nonfinite_starts_global", "nonfinite", [], [(NAN, 10.0, 15.0), (10.0, NAN, 15.0), (INF, 10.0, 15.0), (-INF, -INF, 15.0), (10.0, INF, 15.0)], _nonfinite, anchor="tl",
        sizes=(SMALL, QHD), modes={SMALL: GLOBAL, QHD: GLOBAL})
    return out


def _centre_call(seeds):
    """The get_centre point of the shape's first white pixel in raster order, relative to the anchor: where find_lines starts its first cast."""
    m = synthetic_mask(seeds, SMALL, "tile")
    ax, ay = C.ANCHORS["tile"](*ROI[SMALL][2:])
    ys, xs = np.nonzero(m)
    cx, cy = ind.get_centre(m, f32(xs[0]), f32(ys[0]))
    return [(float(cx) - ax, float(cy) - ay, 15.0)]


FAMILIES = ("short", "handover", "overflow", "ties", "residency", "outside", "gaps", "nonfinite")
MAX_CALLS = 150          # per (size, family)


def cases_at(size, family=None):
    return [c for c in cases() if size in c.sizes and (family is None or c.family == family)]


def anchor_of(case, size):
    _, _, rw, rh = ROI[size]
    return C.ANCHORS[case.anchor](rw, rh)


def calls_of(case, size):
    """The case's calls in ROI coordinates at a size: lists are relative to the anchor, callables give absolute positions from the ROI's
    size and the anchor."""
    _, _, rw, rh = ROI[size]
    ax, ay = anchor_of(case, size)
    if callable(case.calls):
        raw = case.calls(rw, rh, ax, ay)
        assert 1 <= len(raw) <= 16, case.name
        return [(float(px), float(py), float(g)) for px, py, g in raw]
    return [(float(px) + ax, float(py) + ay, float(g)) for px, py, g in case.calls]


def frame(case, W, H):
    """The BGRA frame of a case: its seeds in a marker colour over lsd_cases' marker-free frame."""
    x, y, rw, rh = ROI[(W, H)]
    ax, ay = anchor_of(case, (W, H))
    f = C._blank((W, H)).copy()
    if len(case.seeds):
        xs, ys = case.seeds[:, 0] + ax, case.seeds[:, 1] + ay
        assert xs.min() >= 0 and ys.min() >= 0 and xs.max() < rw and ys.max() < rh, case.name
        f[y + ys, x + xs] = C.COLOURS[[c.name for c in cases()].index(case.name) % 3]
    return f


@functools.lru_cache(maxsize=None)
def reference(size):
    """(Placed, ...) of cases_at(size): every case's frame through the oracle for its lsd image.  Shared by the tests of a session;
    nothing may write to it."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o
    cs = cases_at(size)

    def one(c):
        r = o.process_frame(frame(c, *size), stages=0x1, max_gap=15, want_images=True)
        assert r["map_open"] == 1
        r["lsd"].setflags(write=False)
        ax, ay = anchor_of(c, size)
        return Placed(c, size, r["lsd"], tuple(calls_of(c, size)), ax, ay)

    C._blank(size)
    with ThreadPoolExecutor(max(1, min(os.cpu_count() or 1, len(cs), 16))) as ex:
        return tuple(ex.map(one, cs))
