"""Inputs of the terrain-relief tests, shared by the host and the device tests.  Every case says what it is for and checks, on the
restatement (relief_ref.py), that it contains it: a case that no longer sits on its boundary fails on the CPU before it reaches a GPU.
`family` names the rule a case guards; tests/test_relief_host.py holds the restatement with that rule changed against the family."""
import collections
import functools
import math

import numpy as np

import relief_ref as R

TW, TH = 64, 16                                                   # k_relief's tile (csrc/smh_kernels.h, SMH_REACH_TW / SMH_REACH_TH)
NO_BOUNDS = ((0, 0), (0, 0))
Z_IS_V = 12799.8046875                                            # scale[2] with zscale = 65535 exactly: z is the texel's value (to an ulp)
CENTRES = (1.0, 1.0, 0.5, 0.5)                                    # with a rectangle (0, W, 0, H): px = X and py = Y exactly

Case = collections.namedtuple("Case", "name family hm minimap window viewport fit opt check")


def restate(c, mutant=None, **opt):
    return R.relief(c.window, c.viewport, c.minimap, c.hm, c.fit, dict(c.opt, **opt), mutant)


def checked(c):
    """The case's restatement, after the case's own check."""
    r = restate(c)
    c.check(c, r)
    return r


# ---- heightmaps (cached: the device tests keep one copy of each on the device)
@functools.lru_cache(maxsize=None)
def one():
    return np.array([[30000]], np.uint16), NO_BOUNDS, (1.0, 1.0, 100.0)


@functools.lru_cache(maxsize=None)
def two():
    return np.array([[0, 65535], [20000, 40000]], np.uint16), NO_BOUNDS, (1.0, 1.0, 30.0)


@functools.lru_cache(maxsize=None)
def three_five():
    return np.random.default_rng(3).integers(0, 65536, size=(5, 3)).astype(np.uint16), NO_BOUNDS, (1.0, 1.0, 20.0)


@functools.lru_cache(maxsize=None)
def flat():
    return np.full((16, 16), 1234, np.uint16), NO_BOUNDS, (1.0, 1.0, 40.0)


@functools.lru_cache(maxsize=None)
def xramp():
    """16 x 4, texel (x, y) = 1000 x, z = the texel's value."""
    return np.tile((1000 * np.arange(16)).astype(np.uint16), (4, 1)), NO_BOUNDS, (1.0, 1.0, Z_IS_V)


@functools.lru_cache(maxsize=None)
def pyramid(scale_z=50.0):
    """32 x 32, 2000 per step towards the middle: 117 m at the top with scale_z = 50."""
    y, x = np.mgrid[0:32, 0:32]
    return (2000 * np.minimum(np.minimum(x, 31 - x), np.minimum(y, 31 - y))).astype(np.uint16), ((7, -5), (0, 0)), (1.0, 1.0, scale_z)


@functools.lru_cache(maxsize=None)
def random64():
    """64 x 64 random; texel (0, 0) is 0, so a firing solution from there has the target's height as its altitude difference."""
    data = np.random.default_rng(64).integers(0, 65536, size=(64, 64)).astype(np.uint16)
    data[0, 0] = 0
    return data, NO_BOUNDS, (1.0, 1.0, 40.0)


@functools.lru_cache(maxsize=None)
def step(axis):
    """130 x 33: z = 55 left of column 64 (axis 0) or above row 16 (axis 1), 95 from there on."""
    y, x = np.mgrid[0:33, 0:130]
    return np.where((x < 64) if axis == 0 else (y < 16), 55, 95).astype(np.uint16), NO_BOUNDS, (1.0, 1.0, Z_IS_V)


# ---- checks
def _counts(r):
    b = r["bytes"]
    return int(((b & R.HAS_HEIGHT) != 0).sum()), int(((b & R.CONTOUR) != 0).sum()), int(((b & R.MAJOR) != 0).sum())


def _check_counts(height, contour, major, exact=False):
    """At least (exact: exactly) that many pixels with a height, on a contour, on an index contour; MAJOR only on CONTOUR on HAS_HEIGHT."""
    def check(c, r):
        got = _counts(r)
        assert (got == (height, contour, major)) if exact else all(g >= w for g, w in zip(got, (height, contour, major))), (c.name, got)
        b = r["bytes"]
        assert not ((b & R.MAJOR) != 0)[(b & R.CONTOUR) == 0].any() and not ((b & R.CONTOUR) != 0)[(b & R.HAS_HEIGHT) == 0].any()
        assert not r["shades"][(b & R.HAS_HEIGHT) == 0].any() and not r["heights"][(b & R.HAS_HEIGHT) == 0].any()
    return check


def _check_boundary(px, inside):
    def check(c, r):
        assert r["px"][0] == px and r["py"][0] == 0.0, (c.name, float(r["px"][0]).hex(), float(r["py"][0]).hex())
        assert int(r["bytes"][0, 0]) == (R.HAS_HEIGHT if inside else 0), (c.name, r["bytes"])
    return check


def _check_integers(c, r):
    ow, oh = c.window
    assert np.array_equal(r["px"], np.arange(ow)) and np.array_equal(r["py"], np.arange(oh))
    # the identity with the firing solutions' height(): the bilinear z at integer coordinates is the texel's own, bit for bit
    data, _, scale = c.hm
    zs = np.float64(np.float32(scale[2])) / np.float64(0.1953125)
    want = (data[:oh, :ow].astype(np.float64) / np.float64(65535.0)) * zs
    assert np.array_equal(r["z"], want) and np.array_equal(restate(c, nearest=True)["z"], want)


def _check_half(c, r):
    assert ((r["px"] - np.floor(r["px"])) == 0.5).all() and ((r["py"] - np.floor(r["py"])) == 0.5).all()
    assert not np.array_equal(restate(c, mutant="nearest")["heights"], r["heights"])
    _check_counts((c.window[0] - 1) * (c.window[1] - 1), 0, 0, exact=True)(c, r)   # (px = W - 0.5 rounds to W: outside)


def _check_ramp(c, r):
    # by hand: z = 1000 X, L = floor((1000 X - 250) / 2500) = -1 0 0 1 1 1 2 2 3 3 3 4 4 5 5 5 for X = 0 .. 15; the pixel LEFT of a
    # step carries CONTOUR, and MAJOR (M = 2) where the level reached is even: into 0 at X = 0, into 2 at X = 5, into 4 at X = 10
    want = np.zeros(16, np.uint8) + R.HAS_HEIGHT
    want[[2, 7, 12]] |= R.CONTOUR
    want[[0, 5, 10]] |= R.CONTOUR | R.MAJOR
    assert np.array_equal(r["bytes"], np.tile(want, (4, 1))), r["bytes"][0]
    assert np.array_equal(r["level"][0], [-1, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 5])
    assert np.allclose(r["heights"][0], 1000.0 * np.arange(16), rtol=1e-7, atol=0.0)


def _check_witness(column=None, row=None, major=False):
    """CONTOUR exactly on that column or row of the window: the pixel whose only witness lies past it."""
    def check(c, r):
        want = np.zeros(r["bytes"].shape, bool)
        if column is not None:
            want[:, column] = True
        else:
            want[row, :] = True
        assert np.array_equal((r["bytes"] & R.CONTOUR) != 0, want) and np.array_equal((r["bytes"] & R.MAJOR) != 0, want & major), c.name
        assert (r["bytes"] & R.HAS_HEIGHT).all()
    return check


def _check_levels(lo, hi, major):
    """The step's two levels, and whether the pixels left of it are index contours."""
    def check(c, r):
        assert r["level"][0, 63] == lo and r["level"][0, 64] == hi, (c.name, r["level"][0, 63], r["level"][0, 64])
        _check_witness(column=63, major=major)(c, r)
    return check


def _check_no_contour(finite_levels):
    def check(c, r):
        n = _counts(r)
        assert n[0] == c.window[0] * c.window[1] and n[1] == 0 and n[2] == 0, (c.name, n)
        assert np.isfinite(r["level"]).all() == finite_levels, c.name
    return check


def _check_shades(c, r, distinct=3):
    has = (r["bytes"] & R.HAS_HEIGHT) != 0
    assert has.sum() >= 100 and len(np.unique(r["shades"][has])) >= distinct, (c.name, np.unique(r["shades"][has]))


def _check_uniform(c, r):
    has = (r["bytes"] & R.HAS_HEIGHT) != 0
    # s = lz everywhere: 0x1.6a09e667f3bcdp-1 * 255 + 0.5 = 180.8
    assert has.sum() >= 100 and (r["shades"][has] == 180).all(), np.unique(r["shades"][has])
    _check_shades(c, restate(c, exaggeration=1.0))                  # ... and not because the ground is flat


def _check_clipped(c, r):
    has = (r["bytes"] & R.HAS_HEIGHT) != 0
    s = r["shades"][has]
    assert (s == 0).sum() >= 10 and (s == 255).sum() >= 10, (c.name, np.unique(s, return_counts=True))
    _check_shades(c, r)


def _check_nothing(valid):
    def check(c, r):
        assert r["valid"] == valid and not r["bytes"].any() and not r["shades"].any() and not r["heights"].any(), c.name
    return check


def _check_column_only(column):
    def check(c, r):
        has = (r["bytes"] & R.HAS_HEIGHT) != 0
        assert has[:, column].any() and not np.delete(has, column, axis=1).any(), c.name
        assert np.isnan(r["px"][column])
    return check


def _check_den(c, r):
    other = restate(c, mutant="den")
    assert other["den"][0, 0] != r["den"][0, 0] and other["shades"][0, 0] != r["shades"][0, 0], (c.name, r["shades"], other["shades"])


@functools.lru_cache(maxsize=None)
def _den_case():
    """A pixel whose shade byte turns on the order of the sum under the square root: (1 + p p) + q q and 1 + (p p + q q) differ by an
    ulp there, and lz is the double at which s * 255 + 0.5 passes an integer for one of them only.  Found by a seeded search."""
    rng = np.random.default_rng(7)
    zs = 1.0 / 0.1953125
    for _ in range(4000):
        a, b = (int(v) for v in rng.integers(1, 65536, size=2))
        p, q = (a / 65535.0) * zs, (b / 65535.0) * zs
        d1, d2 = math.sqrt((1.0 + p * p) + q * q), math.sqrt(1.0 + (p * p + q * q))
        if d1 == d2:
            continue
        for k in range(1, 256):
            lz = ((k - 0.5) / 255.0) * d1
            for _ in range(4):
                lz = math.nextafter(lz, -math.inf)
            for _ in range(9):
                if math.floor((lz / d1) * 255.0 + 0.5) != math.floor((lz / d2) * 255.0 + 0.5) and lz / d1 <= 1.0 and lz / d2 <= 1.0:
                    hm = (np.array([[0, a], [b, 0]], np.uint16), NO_BOUNDS, (1.0, 1.0, 1.0))
                    return Case("the sum under the root, in its order", "den", hm, (0, 2, 0, 2), (2, 2), CENTRES, True,
                                R.options(light=(0.0, 0.0, lz), interval_m=0.0), _check_den)
                lz = math.nextafter(lz, math.inf)
    raise AssertionError("no pixel found")


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    D = R.options
    # ---- both sides of "has a height", on the 1 x 1 heightmap and a 1 x 1 window; py = 0 exactly.  px = 0.5 - tx at scale 1 and
    # -(0.5 - tx) at scale -1 (a mirrored viewport), so tx = 2^-54 gives the f64 neighbours of 0.5 and of -0.5 that lie inside
    for tx, px, inside in ((0.0, 0.5, False), (2.0 ** -54, 0.5 - 2.0 ** -54, True), (-2.0 ** -53, 0.5 + 2.0 ** -53, False)):
        out.append(Case("px = W - 0.5 %+g" % (px - 0.5), "inside", one(), (0, 1, 0, 1), (1, 1), (1.0, 1.0, tx, 0.5), True, D(), _check_boundary(px, inside)))
        out.append(Case("px = -0.5 %+g" % (0.5 - px), "inside", one(), (0, 1, 0, 1), (1, 1), (-1.0, 1.0, tx, 0.5), True, D(), _check_boundary(-px, inside)))
    # ---- exact placements
    out.append(Case("integer coordinates, the ramp by hand", "level", xramp(), (0, 16, 0, 4), (16, 4), CENTRES, True,
                    D(interval_m=2500.0, base_m=250.0, major_every=2), lambda c, r: (_check_integers(c, r), _check_ramp(c, r))))
    out.append(Case("integer coordinates, random", "identity", random64(), (0, 64, 0, 64), (64, 17), CENTRES, True, D(), _check_integers))
    out.append(Case("fx = fy = 0.5", "bilinear", three_five(), (0, 3, 0, 5), (3, 5), None, True, D(interval_m=0.0), _check_half))
    out.append(Case("2 x 2", "bilinear", two(), (0, 32, 0, 16), (32, 16), None, True, D(interval_m=1.0), _check_counts(24 * 12, 100, 20)))
    out.append(Case("magnified 8 x", "bilinear", random64(), (0, 512, 0, 512), (130, 33), None, True, D(interval_m=5.0), _check_counts(130 * 33, 1000, 200)))
    out.append(Case("minified 8 x", "bilinear", random64(), (0, 8, 0, 8), (17, 15), None, True, D(interval_m=50.0, major_every=1), _check_counts(64, 40, 40)))
    out.append(Case("magnified 8 x, nearest", "nearest", random64(), (0, 512, 0, 512), (65, 17), None, True, D(nearest=True, interval_m=5.0), _check_counts(65 * 17, 100, 20)))
    out.append(Case("flat", "level", flat(), (0, 64, 0, 16), (64, 16), None, True, D(interval_m=0.25), _check_counts(62 * 15, 0, 0, exact=True)))
    # ---- the tile's and the wave's edges; zoomed and panned with a scale per axis, the rectangle partly outside the larger windows
    zoom = (1.7, 0.95, -9.25, -2.5)
    for w, h in ((1, 1), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (130, 33)):
        need = (1, 0, 0) if (w, h) == (1, 1) else (w * h // 2, w * h // 20, w * h // 100)
        out.append(Case("window %d x %d" % (w, h), "window", pyramid(), (4, 56, 2, 40), (w, h), zoom, True, D(), _check_counts(*need)))
    out.append(Case("bounds offset", "window", pyramid(), (8, 56, 4, 40), (65, 33), zoom, False, D(interval_m=2.0), _check_counts(900, 40, 1)))
    out.append(Case("rectangle partly outside", "window", pyramid(), (30, 90, 10, 60), (65, 33), None, True, D(interval_m=2.0), _check_counts(35 * 23, 40, 1)))
    out.append(Case("rectangle of zero width", "inside", pyramid(), (10, 10, 0, 33), (65, 33), (1.0, 1.0, 0.5, 0.0), True, D(), _check_nothing(1)))
    out.append(Case("rectangle of zero width, nearest", "inside", pyramid(), (10, 10, 0, 33), (65, 33), (1.0, 1.0, 0.5, 0.0), True, D(nearest=True),
                    _check_column_only(10)))
    out.append(Case("viewport scale not finite", "inside", pyramid(), (4, 56, 4, 40), (65, 33), (float("inf"), 1.0, 0.0, 0.0), True, D(), _check_nothing(1)))
    out.append(Case("no minimap rectangle", "inside", pyramid(), None, (65, 33), zoom, True, D(), _check_nothing(0)))
    # ---- contours: the witness past the tile's last column, its last row, the window's last column
    whole = (0, 130, 0, 33)
    out.append(Case("witness past the tile's last column", "witness", step(0), whole, (130, 33), CENTRES, True, D(), _check_witness(column=63)))
    out.append(Case("witness past the tile's last row", "witness", step(1), whole, (130, 33), CENTRES, True, D(), _check_witness(row=15)))
    out.append(Case("witness past the window's last column", "witness", step(0), whole, (64, 33), CENTRES, True, D(), _check_witness(column=63)))
    # ---- the levels of the step 55 | 95 m: which index contours lie between them
    out.append(Case("M - 1 levels across no multiple", "level", step(0), whole, (130, 17), CENTRES, True, D(), _check_levels(5, 9, False)))
    out.append(Case("four levels across one multiple", "level", step(0), whole, (130, 17), CENTRES, True, D(base_m=20.0), _check_levels(3, 7, True)))
    out.append(Case("below the base, across none", "below base", step(0), whole, (130, 17), CENTRES, True, D(base_m=1000.0), _check_levels(-95, -91, False)))
    out.append(Case("below the base, across -95", "below base", step(0), whole, (130, 17), CENTRES, True, D(base_m=1020.0), _check_levels(-97, -93, True)))
    out.append(Case("across level 0", "below base", step(0), whole, (130, 17), CENTRES, True, D(base_m=74.0), _check_levels(-2, 2, True)))
    out.append(Case("major_every 0", "level", step(0), whole, (130, 17), CENTRES, True, D(base_m=20.0, major_every=0), _check_levels(3, 7, False)))
    out.append(Case("major_every 1", "level", step(0), whole, (130, 17), CENTRES, True, D(major_every=1), _check_levels(5, 9, True)))
    out.append(Case("interval 0", "level", step(0), whole, (130, 17), CENTRES, True, D(interval_m=0.0), _check_no_contour(False)))
    out.append(Case("interval the smallest subnormal", "level", step(0), whole, (130, 17), CENTRES, True, D(interval_m=5e-324), _check_no_contour(False)))
    out.append(Case("interval 1e300", "level", step(0), whole, (130, 17), CENTRES, True, D(interval_m=1e300), _check_no_contour(True)))
    out.append(Case("interval 1e300 about the base", "level", step(0), whole, (130, 17), CENTRES, True, D(interval_m=1e300, base_m=75.0, major_every=1),
                    _check_levels(-1, 0, True)))
    # ---- shade and paint
    cover = (0, 65, 0, 33)
    out.append(Case("shade", "shade", pyramid(), cover, (65, 33), None, True, D(), _check_shades))
    out.append(Case("negative scale", "shade", pyramid(-50.0), cover, (65, 33), None, True, D(), _check_shades))
    out.append(Case("exaggeration 0", "shade", pyramid(), cover, (65, 33), None, True, D(exaggeration=0.0), _check_uniform))
    out.append(Case("light with lz = 0", "shade", pyramid(), cover, (65, 33), None, True, D(light=(-0.6, -0.8, 0.0), exaggeration=0.2), _check_shades))
    out.append(Case("s below 0 and above 1", "shade", pyramid(), cover, (65, 33), None, True, D(light=(-3.0, -3.0, 2.0)), _check_clipped))
    out.append(Case("all weights 0", "shade", pyramid(), cover, (65, 33), None, True, D(contour=(9, 9, 9, 0), major=(9, 9, 9, 0), shade_weight=0), _check_shades))
    out.append(_den_case())
    assert len(set(c.name for c in out)) == len(out)
    return out


def by_family(family):
    return [c for c in all_cases() if c.family == family]
