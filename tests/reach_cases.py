"""Inputs of the reach-map tests, shared by the host and the device tests.  Every case says what it is for and checks, on the
restatement (reach_ref.py), that it contains it: a case that no longer holds its decision boundary fails on the CPU."""
import collections
import functools

import numpy as np

import reach_ref as R

TW, TH = 64, 16                                                   # k_reach's tile (csrc/smh_kernels.h, SMH_REACH_TW / SMH_REACH_TH)
VG = R.FR.V2 / R.FR.G                                             # the flat-ground range, V^2 / g = 1232.25 m

Case = collections.namedtuple("Case", "name hm minimap mpx origin window viewport fit ring_m check")


def restate(c, ring_m=None):
    return R.reach(c.origin, c.window, c.viewport, c.minimap, c.mpx, c.hm, c.fit, c.ring_m if ring_m is None else ring_m)


@functools.lru_cache(maxsize=None)
def long_map():
    """1400 x 24, gentle slopes (a few metres): the range decides the band, and only ranges beyond ~900 texels reach the bands below
    1200 mils -- hence the long axis and an origin near its end."""
    y, x = np.mgrid[0:24, 0:1400]
    return ((np.sin(x / 90.0) * 0.5 + 0.5) * 2000 + y * 40).astype(np.uint16), ((0, 0), (0, 0)), (1.0, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def steep_map():
    """64 x 48 with a z scale of 1500: neighbouring texels differ by hundreds of metres."""
    rng = np.random.default_rng(11)
    return rng.integers(0, 65536, size=(48, 64)).astype(np.uint16), ((7, -5), (0, 0)), (1.0, 1.0, 1500.0)


@functools.lru_cache(maxsize=None)
def flat_map():
    """2816 x 1408, flat: a window pixel of the 64 x 32 window is exactly 44 texels (metres) on either axis."""
    return np.full((1408, 2816), 1234, np.uint16), ((0, 0), (0, 0)), (1.0, 1.0, 40.0)


def _bands(r):
    c7 = r["classes"] & 0x7F
    return set(int(v) for v in np.unique(c7))


def _check_bands(c, r):
    assert _bands(r) == set(range(1, 10)), sorted(_bands(r))       # out of range and every band 0 .. 7
    assert (r["source"] == R.HEIGHTMAP).all() and (r["classes"] & R.RING).any()


def _check_steep(c, r):
    c7 = r["classes"] & 0x7F
    near = (c7 == R.OUT_OF_RANGE) & (r["meters"] < 100.0)
    assert near.sum() >= 100 and (c7 >= R.BAND0).any(), near.sum()  # out of range by altitude alone, at short range
    assert (r["source"] == R.HEIGHTMAP).all()


def _check_present(*need):
    def check(c, r):
        assert set(need) <= _bands(r), (need, sorted(_bands(r)))
    return check


def _check_circle(radius_px):
    def check(c, r):
        c7 = r["classes"] & 0x7F
        oh, ow = c7.shape
        assert (r["source"] == R.SCALES).all()
        # in range exactly inside the circle of V^2 / g metres around the origin (pixels a hundredth of a pixel off the circle aside)
        y, x = np.mgrid[0:oh, 0:ow]
        d = np.hypot(x + 0.5 - c.origin[0], y + 0.5 - c.origin[1])
        assert ((c7 >= R.BAND0) == (d <= radius_px))[np.abs(d - radius_px) > 0.01].all()
        assert (c7 == R.OUT_OF_RANGE).any() and (c7 >= R.BAND0).any()
    return check


def _check_nothing(valid):
    def check(c, r):
        assert r["valid"] == valid and not r["classes"].any()
    return check


def _check_seam(c, r):
    full = R.reach(c.origin, (c.window[0] + 1, c.window[1] + 1), c.viewport, c.minimap, c.mpx, c.hm, c.fit, c.ring_m)
    src, m = full["source"], full["meters"]
    assert {R.SCALES, R.HEIGHTMAP} <= set(int(v) for v in np.unique(r["source"]))
    b = np.floor(m / c.ring_m)
    oh, ow = r["classes"].shape
    # a pixel whose right neighbour lies across the seam in another ring interval, and whose own interval is its other neighbour's: no ring
    own_s, own_b = src[:oh, :ow], b[:oh, :ow]
    across = (src[:oh, 1:ow + 1] != own_s) & (src[:oh, 1:ow + 1] != R.NONE) & (b[:oh, 1:ow + 1] != own_b)
    quiet = (src[1:oh + 1, :ow] != own_s) | (b[1:oh + 1, :ow] == own_b)
    sel = across & quiet & (own_s != R.NONE)
    assert sel.any() and not (r["classes"][sel] & R.RING).any()
    assert (r["classes"] & R.RING).any()


def _check_zero_range(px, py):
    def check(c, r):
        assert r["meters"][py, px] == 0.0 and (r["classes"][py, px] & 0x7F) == R.BAND0 + 7
    return check


def _check_flat(c, r):
    # by hand: a pixel (X, Y) is 44 * sqrt(X^2 + Y^2) metres from the origin's pixel (0, 0), alt = 0, so it is in range iff
    # 44^2 (X^2 + Y^2) <= (V^2 / g)^2 = 1232.25^2, that is X^2 + Y^2 <= 784 (28^2: 1232 m; 785 is 1232.79 m)
    oh, ow = r["classes"].shape
    y, x = np.mgrid[0:oh, 0:ow]
    assert 44.0 * np.sqrt(784.0) <= VG < 44.0 * np.sqrt(785.0)
    want = (x * x + y * y) <= 784
    assert np.array_equal((r["classes"] & 0x7F) >= R.BAND0, want) and np.array_equal((r["classes"] & 0x7F) == R.OUT_OF_RANGE, ~want)
    assert np.allclose(r["meters"], 44.0 * np.sqrt((x * x + y * y).astype(np.float64)), rtol=1e-15, atol=0.0)
    assert r["meters"][0, 28] == 1232.0 and (r["classes"][0, 28] & 0x7F) == R.BAND0 and (r["classes"][0, 29] & 0x7F) == R.OUT_OF_RANGE


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    # the minimap rectangle holds the whole 96 x 64 window at the identity viewport (a little more: a coordinate that ROUNDS to the
    # heightmap's width or height is outside it)
    whole = (0, 97, 0, 66)
    out.append(Case("every band", long_map(), whole, None, (20.4 * 97 / 1400, 30.0), (96, 64), None, True, 250.0, _check_bands))
    out.append(Case("out of range by altitude", steep_map(), whole, None, (40.3, 30.6), (96, 64), None, True, 10.0, _check_steep))
    # the tile's edges: 64 x 16 and one less, one more, a window of one pixel, and the issue's 65 x 33; zoomed and panned with a scale
    # per axis, so the rectangle (8 .. 56, 4 .. 40 in map-ROI coordinates) covers every window
    zoom = (1.7, 0.95, -9.25, 2.5)
    for w, h in ((65, 33), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (1, 1)):
        need = (R.OUT_OF_RANGE,) if (w, h) != (1, 1) else ()
        out.append(Case("window %d x %d" % (w, h), steep_map(), (8, 56, 4, 40), 3.0, (12.5, 6.25), (w, h), zoom, True, 10.0, _check_present(*need)))
    out.append(Case("bounds offset", steep_map(), (8, 56, 4, 40), 3.0, (20.0, 11.0), (65, 33), zoom, False, 0.0, _check_present(R.OUT_OF_RANGE)))
    # an origin outside the heightmap: the scales branch everywhere, a circle of V^2 / g metres = 1232.25 / 30 px
    out.append(Case("origin outside, m/px", steep_map(), (30, 90, 10, 60), 30.0, (12.25, 30.75), (96, 64), None, True, 250.0, _check_circle(VG / 30.0)))
    out.append(Case("origin outside, no m/px", steep_map(), (30, 90, 10, 60), None, (12.25, 30.75), (96, 64), None, True, 250.0, _check_nothing(1)))
    out.append(Case("no heightmap, no m/px", None, None, None, (12.25, 30.75), (96, 64), None, True, 0.0, _check_nothing(1)))
    # the window partly outside the rectangle: both sources in one frame
    out.append(Case("seam", long_map(), (20, 70, 10, 50), 21.0, (44.0, 31.0), (96, 64), None, True, 10.0, _check_seam))
    out.append(Case("NaN origin", steep_map(), whole, 3.0, (float("nan"), 4.0), (96, 64), None, True, 10.0, _check_nothing(0)))
    out.append(Case("inf origin", steep_map(), whole, 3.0, (4.0, float("inf")), (65, 33), None, True, 0.0, _check_nothing(0)))
    out.append(Case("m == 0, scales", None, None, 2.5, (10.5, 7.5), (65, 33), None, True, 10.0, _check_zero_range(10, 7)))
    out.append(Case("m == 0, heightmap", steep_map(), whole, None, (10.5, 7.5), (65, 33), None, True, 0.0, _check_zero_range(10, 7)))
    out.append(Case("flat circle", flat_map(), (0, 64, 0, 32), None, (0.5, 0.5), (64, 32), None, True, 250.0, _check_flat))
    return out


def checked(c):
    """The case's restatement, after the case's own check."""
    r = restate(c)
    c.check(c, r)
    return r


def samples(r, n, seed):
    """At least n window pixels of a restated window, every class present among them -> [(x, y)]."""
    rng = np.random.default_rng(seed)
    oh, ow = r["classes"].shape
    pick = set()
    c7 = r["classes"] & 0x7F
    for c in np.unique(c7):
        ys, xs = np.nonzero(c7 == c)
        for i in rng.choice(len(ys), size=min(len(ys), 8), replace=False):
            pick.add((int(xs[i]), int(ys[i])))
    flat = rng.permutation(ow * oh)
    for i in flat:
        if len(pick) >= n:
            break
        pick.add((int(i % ow), int(i // ow)))
    return sorted(pick)
