"""Cases for the search service's sampler of a ray's first 64 steps (tests/test_sampler_host.py, tests/test_sampler_gpu.py), built
with the seeds, the blank frame, the ROI table and the marker colours of tests/lsd_cases.py.

Every case is a set of seed pixels in ROI coordinates of the smallest frame the case builders know, 1024 x 768 (ROI 360 x 585: the
sampler sees a candidate's window, so a larger frame adds nothing), and what the search sees is their dilation by the cross.  The
reference is always the oracle's own record of the painted frame.

  edges     a bar 2 px inside each ROI edge: candidates within 4 px of the edge, so their windows have columns left of / rows above
            the image (negative window coordinates) and their rays leave the image from step 3 on -- inside the first 8, 16, 32
            and 64 steps, depending on the angle
  corners   a diagonal from 1 px inside each ROI corner
  half      bars two seeds thick (four pixels after the dilation): start points on x.5 / y.5
  steps     a vertical bar that is white to step 63 of its first candidate's downward ray and then black for 16 steps, and three
            whose gap starts at steps 49, 50 and 51 (the reject threshold is a gap that starts at step 50)
  window    two single seeds 10 rows apart (one kept window serves both candidates), then one 230 columns further right (a refill)
  gap_T     max_gap = T for T in 1, 7, 8, 15, 16, 23, 24, 31: dashes T and T + 1 apart, and bars whose first candidate's ray is white
            to step a - 1 and then black for T + 1 steps, a = 8, 16, 24, 32 -- the abort of that ray straddles the boundary of a
            group of 8 and of 16 samples, and the rays beside it abort all around it
"""
import collections
import functools

import numpy as np

import lsd_cases as C

SIZE = C.SMALL
RW, RH = C.ROI[SIZE][2:]
GAPS = (1, 7, 8, 15, 16, 23, 24, 31)
STEP_BARS = ((64, 60), (49, 120), (50, 180), (51, 240))     # (a: the first black step of the first candidate's downward ray, column)
STEP_Y0 = 40
GAP_BARS = ((8, 40), (16, 90), (24, 140), (32, 190))
GAP_Y0 = 30

Case = collections.namedtuple("Case", "name max_gap seeds")
Ref = collections.namedtuple("Ref", "case lines rounds mask n_mask_px steps")


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        Case("edges", 15, C.hbar(20, 2, 60) + C.hbar(150, RH - 3, 60) + C.vbar(2, 120, 60) + C.vbar(RW - 3, 300, 60)),
        Case("corners", 15, [(1 + i, 1 + i) for i in range(45)] + [(RW - 2 - i, 1 + i) for i in range(45)] +
             [(1 + i, RH - 2 - i) for i in range(45)] + [(RW - 2 - i, RH - 2 - i) for i in range(45)]),
        Case("half", 15, C.hbar(60, 100, 56, 2) + C.vbar(200, 200, 56, 2) + [(100 + i, 300 + j) for i in range(2) for j in range(2)]),
        Case("steps", 15, [p for a, x in STEP_BARS for p in C._straddle(a, 16, x=x, y0=STEP_Y0)]),
        Case("window", 15, [(40, 60), (44, 70), (274, 66)]),
    ]
    for T in GAPS:
        out.append(Case("gap_%d" % T, T, C._dots(T, T, x0=20, y=420) + C._dots(T, T + 1, x0=20, y=480) +
                        [p for a, x in GAP_BARS for p in C._straddle(a, T + 1, x=x, y0=GAP_Y0)]))
    return tuple(Case(c.name, c.max_gap, np.array(sorted(set(c.seeds)), np.int64).reshape(-1, 2)) for c in out)


def frame(case):
    x, y, rw, rh = C.ROI[SIZE]
    f = C._blank(SIZE).copy()
    xs, ys = case.seeds[:, 0], case.seeds[:, 1]
    assert xs.min() >= 0 and ys.min() >= 0 and xs.max() < rw and ys.max() < rh, case.name
    f[y + ys, x + xs] = C.COLOURS[[c.name for c in cases()].index(case.name) % 3]
    return f


def groups():
    """[(max_gap, [case])], as lsd_cases.groups."""
    by = collections.OrderedDict()
    for c in cases():
        by.setdefault(c.max_gap, []).append(c)
    return sorted(by.items())


@functools.lru_cache(maxsize=None)
def reference():
    """{name: Ref}: the oracle's record and mask of every case's frame, once per session; nothing may write to it."""
    from oracle import oracle as o
    out = {}
    for c in cases():
        r = o.process_frame(frame(c), stages=0x1, max_gap=c.max_gap, want_images=True)
        assert r["map_open"] == 1
        r["lsd"].setflags(write=False)
        out[c.name] = Ref(c, r["lines"], r["rounds"], r["lsd"], r["n_mask_px"], r["steps"])
    return out
