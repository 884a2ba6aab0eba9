"""The crafted line-search cases (tests/lsd_cases.py) on the CPU: every case's expectation holds on the oracle at every size it is
placed at, the cases are the same mask at every size, the oracle and the numpy restatement (tests/independent_lsd.py) agree on
every case -- and the cases have teeth: a copy of the restatement with one rule changed at a time differs from the oracle on at
least one case each."""
import numpy as np
import pytest

import independent_lsd as ind
import lsd_cases as C
from oracle import oracle as o

f32 = np.float32
FULL_ROUNDS = 160         # cases with more rounds than this (hundreds) compare find_longest_line at named candidates instead of whole searches


def test_roi_table_and_the_blank_frame():
    for size in C.SIZES:
        assert o.map_bounds(*size) == C.ROI[size]
        r = o.process_frame(C._blank(size), stages=0x1, want_images=True)
        assert r["map_open"] == 1 and r["n_mask_px"] == 0 and r["rounds"] == 0      # marker-free: the mask of a case is its seeds alone
    names = [c.name for c in C.cases()]
    assert len(set(names)) == len(names) and set(c.family for c in C.cases()) == set(C.FAMILIES)
    assert len(C.cases_at(C.SMALL)) == len(C.cases_at(C.HD)) >= 100 and len(C.cases_at(C.QHD)) <= 24 and len(C.cases_at(C.WIDE)) >= 5
    for size in (C.SMALL, C.HD, C.QHD):
        assert set(c.family for c in C.cases_at(size)) == set(C.FAMILIES), size


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_expectations_hold_on_the_oracle(size):
    bad = []
    for R in C.reference(size):
        try:
            C.check_expectation(R)
        except AssertionError as e:
            bad.append((R.case.name, str(e)[:300]))
    assert not bad, bad


def _white(R):
    return np.argwhere(R.mask == 255) - np.array([R.ay, R.ax])


def test_cases_are_the_same_mask_at_every_size():
    """Up to the anchor's shift -- and the mask is the seeds' dilation by the cross, which is what the seeds were designed for."""
    first = {}
    for size in C.SIZES:
        for R in C.reference(size):
            w = _white(R)
            if R.case.name not in first:
                first[R.case.name] = w
                s = R.case.seeds[:, ::-1]
                cross = np.concatenate([s, s + (0, 1), s - (0, 1), s + (1, 0), s - (1, 0)])
                _, _, rw, rh = C.ROI[size]
                cross = cross[(cross[:, 0] + R.ay >= 0) & (cross[:, 0] + R.ay < rh) & (cross[:, 1] + R.ax >= 0) & (cross[:, 1] + R.ax < rw)]
                assert np.array_equal(np.unique(cross, axis=0), w), R.case.name
                assert R.n_mask_px == len(w)
            else:
                assert np.array_equal(first[R.case.name], w), (R.case.name, size)
    assert len(first) == len(C.cases())


def _crop(R):
    """The case's mask cut off below and to the right of its white pixels, behind a margin that no ray crosses (a ray aborts at its max_gap-th
    black sample in a row, so it ends inside the margin as it would in the whole image).  The origin stays: the last bits of a ray's length depend
    on the magnitude of its coordinates, and the cases sit on those bits; the ROI's own left and top edge stay the crop's."""
    m = R.case.max_gap + 4
    ys, xs = np.nonzero(R.mask)
    return np.ascontiguousarray(R.mask[:ys.max() + m + 1, :xs.max() + m + 1])


def _same(a, b):
    return a[1] == b[1] and a[0].shape == b[0].shape and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("family", C.FAMILIES)
def test_oracle_equals_the_numpy_restatement(family):
    refs = {R.case.name: R for size in (C.WIDE, C.SMALL) for R in C.reference(size)}
    n = 0
    for R in refs.values():
        if R.case.family != family:
            continue
        img = _crop(R)
        lines, st = o.find_lines(img, R.case.max_gap)
        assert st["rounds"] == R.rounds and np.array_equal(lines, R.lines), R.case.name       # the crop changes nothing
        if R.rounds <= FULL_ROUNDS:
            got = ind.find_lines(img, R.case.max_gap)
            assert _same(got, (lines, st["rounds"])), (R.case.name, got, lines, st["rounds"])
        else:                                                # named candidates: the first and last white pixel, the middle one, every line's start
            ys, xs = np.nonzero(img)
            pts = [o.get_centre(img, float(xs[i]), float(ys[i])) for i in (0, len(xs) // 2, len(xs) - 1)] + [(float(l[0]), float(l[1])) for l in lines[:3]]
            for (cx, cy) in pts:
                a, b = o.find_longest_line(img, cx, cy, float(R.case.max_gap)), ind.find_longest_line(img, cx, cy, R.case.max_gap)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1], (R.case.name, cx, cy, a, b)
                assert ind.get_centre(img, f32(a[0][2]), f32(a[0][3])) == o.get_centre(img, float(a[0][2]), float(a[0][3])), (R.case.name, cx, cy)
        n += 1
    assert n >= 3


# ---- teeth: the restatement with its rules as knobs (independent_lsd itself stays as it is) ----------------------------------

_RAYS = {}


def _rays(key, img, px, py, max_gap, abort_gt, no_restore):
    k = (key, float(px), float(py), abort_gt, no_restore)
    if k in _RAYS:
        return _RAYS[k]
    h, w = img.shape
    n = len(ind.DX)
    xs, ys = f32(px), f32(py)
    x = np.full(n, xs, f32); y = np.full(n, ys, f32)
    xo = np.zeros(n, f32); yo = np.zeros(n, f32)
    g0 = np.zeros(n, f32); g1 = np.zeros(n, f32); g2 = np.zeros(n, f32)
    walking = np.ones(n, bool)
    mg = f32(max_gap)
    while True:
        walking &= (x >= 0) & (y >= 0) & (x < f32(w)) & (y < f32(h))
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
        walking[ia] = False
        i1 = idx[first]
        g0[i1] = 1; g1[i1] = x[i1]; g2[i1] = y[i1]
        g0[idx[more]] += f32(1)
        ic = idx[~abort]
        xo[ic] = xo[ic] + ind.DX[ic]; yo[ic] = yo[ic] + ind.DY[ic]
        x[ic] = xo[ic] + xs; y[ic] = yo[ic] + ys
    xi, yi = ind._as_u32(x), ind._as_u32(y)
    inside = (xi < w) & (yi < h)
    zero = np.zeros(n, bool)
    zero[inside] = img[yi[inside], xi[inside]] == 0
    xe = np.where(zero, x - ind.DX, xs).astype(f32); ye = np.where(zero, y - ind.DY, ys).astype(f32)
    ddx = (xs - xe).astype(f32); ddy = (ys - ye).astype(f32)
    _RAYS[k] = (xe, ye, (ddx * ddx + ddy * ddy).astype(f32))
    return _RAYS[k]


def _near(x, y, line, le, clamp):
    x0, y0, x1, y1 = (f32(v) for v in line)
    dx, dy = f32(x1 - x0), f32(y1 - y0)
    u = f32(f32(f32(f32(x - x0) * dx) + f32(f32(y - y0) * dy)) / f32(f32(dx * dx) + f32(dy * dy)))
    if clamp:
        u = min(max(u, f32(0)), f32(1))
    ex, ey = f32(x - f32(x0 + f32(u * dx))), f32(y - f32(y0 + f32(u * dy)))
    d = f32(f32(ex * ex) + f32(ey * ey))
    return d <= f32(50) if le else d < f32(50)


def knob_find_lines(key, img, max_gap, accept_ge=False, near_le=False, abort_gt=False, first_max=False, clamp=False, no_restore=False, cap=32,
                    count_speculated=False):
    """independent_lsd.find_lines with its rules as arguments; all defaults = the reference's algorithm."""
    lines, rounds, speculating = [], 0, False
    ys, xs = np.nonzero(img == 255)
    for yy, xx in zip(ys, xs):
        x, y = f32(xx), f32(yy)
        if any(_near(x, y, ln, near_le, clamp) for ln in lines):
            rounds += int(speculating and count_speculated)          # a cast made ahead of the verdict that suppresses it, counted
            continue
        speculating = False
        cx, cy = ind.get_centre(img, x, y)
        xe, ye, length = _rays(key, img, cx, cy, max_gap, abort_gt, no_restore)
        m = length.max()
        best = int(np.nonzero(length == m)[0][0 if first_max else -1])
        rounds += 1
        if (m >= f32(2500)) if accept_ge else (m > f32(2500)):
            ex, ey = ind.get_centre(img, xe[best], ye[best])
            lines.append(np.array([cx, cy, ex, ey], f32))
            speculating = True
            if len(lines) == cap:
                break
    return np.array(lines, f32).reshape(-1, 4), rounds


MUTANTS = {  # name: (knobs, the family whose edge it moves)
    "accept at >= 2500": (dict(accept_ge=True), "acceptance"),         # (told apart by the acc_exactly_2500 cases alone: they are tried first)
    "near at <= 50": (dict(near_le=True), "proximity"),
    "abort at gap > max_gap": (dict(abort_gt=True), "gaps"),
    "first maximum wins": (dict(first_max=True), "ties"),
    "distance to the segment": (dict(clamp=True), "proximity"),
    "end point not restored": (dict(no_restore=True), "gaps"),
    "cap of 33": (dict(cap=33), "cap"),
    "speculated casts counted": (dict(count_speculated=True), "verdict"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_told_apart(mutant):
    """The family named for the mutant must hold a case on which it differs from the oracle (lines or rounds), and on that case the copy
    without any change must agree with the oracle."""
    knobs, family = MUTANTS[mutant]
    refs = [R for R in C.reference(C.SMALL) if R.case.family == family and not R.case.heavy and (R.rounds <= FULL_ROUNDS or family == "cap")]
    killers = []
    for R in sorted(refs, key=lambda R: ("exactly" not in R.case.name, R.rounds)):
        img = _crop(R)
        lines, st = o.find_lines(img, R.case.max_gap)
        got = knob_find_lines(R.case.name, img, R.case.max_gap, **knobs)
        if not _same(got, (lines, st["rounds"])):
            assert _same(knob_find_lines(R.case.name, img, R.case.max_gap), (lines, st["rounds"])), R.case.name
            killers.append(R.case.name)
            break
    print("%s: told apart by %s" % (mutant, killers))
    assert killers, (mutant, family)
