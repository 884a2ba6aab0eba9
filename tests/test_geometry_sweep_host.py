"""CPU half of the geometry sweep (tests/geometry_sweep_cases.py): the case table's self-check, the conditions on the ORACLE's
outputs that keep tests/test_geometry_sweep_gpu.py honest (a scene whose marks the oracle does not see would let a broken edge
pass), the oracle's indifference to the alpha byte, the library's accept-or-refuse decision against the oracle's across every
limit, and the band rule at rh 900 / 901.  No device: smhv_map_bounds, smhv_button_bounds and smhv_debug_band_rows are host code."""
import ctypes as C

import numpy as np
import pytest

import geometry_sweep_cases as G


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


def test_case_table_states_what_the_bounds_give(built):
    G.check_table()


def test_case_table_self_check_notices_a_wrong_size_and_a_missing_layout(built):
    wrong = [c._replace(W=c.W + 1) if (c.W, c.H) == (2360, 360) else c for c in G.CASES]          # a typo in one width
    with pytest.raises(AssertionError):
        G.check_table(wrong)
    for drop in ((319, 360), (4407, 360), (568, 361), (1097, 1184), (2232, 362), (1281, 721), (1127, 1185)):
        with pytest.raises(AssertionError):
            G.check_table([c for c in G.CASES if (c.W, c.H) != drop])


@pytest.mark.parametrize("c", G.CASES, ids=G.IDS)
def test_oracle_sees_every_mark_of_the_scene(o, c):
    frames, infos, refs = G.oracle_of(c)
    qw, qh = c.rw // 2, c.rh // 2
    assert [r["map_open"] for r in refs] == [1, 0, 1]
    for f, info, ref in zip(frames, infos, refs):
        if not ref["map_open"]:
            continue
        lsd = ref["lsd"]
        assert lsd.shape == (c.rh, c.rw) and set(np.unique(lsd)) <= {0, 255}
        assert lsd[:, 0].any() and lsd[:, c.rw - 1].any() and lsd[0].any() and lsd[c.rh - 1].any()
        assert lsd[0, c.rw - 1] and lsd[c.rh - 1, 0] and lsd[c.rh - 1, c.rw - 1]                    # three corners
        assert len(info["marks"]) == 2 * len(G.boundaries(c)) >= 2
        for (r, col, reach) in info["marks"]:
            assert lsd[r, col] == 255 and lsd[r, reach] == 255, (r, col, reach)                   # the dilation crossed the boundary
        assert lsd[qh - 1].any() and lsd[qh].any() and lsd[:, qw - 1].any() and lsd[:, qw].any()
        # the marker lines that were drawn are among the oracle's
        # (find_lines skips what lies within 7 px of the infinite line through an accepted one: an ROI 8 px wide holds ONE line)
        assert ref["n_lines"] >= (2 if c.rw >= 31 else 1), ref["n_lines"]
        for (xa, ya, xb, yb, th) in info["lines"]:
            assert np.hypot(xb - xa, yb - ya) > 50
            hit = [ln for ln in ref["lines"] if _covers(ln, (xa, ya, xb, yb))]
            assert hit, ((xa, ya, xb, yb), ref["lines"])
        if c.rw > 2048:                                                                         # (each covered by an oracle line, above)
            assert any(min(d[0], d[2]) < 2048 <= max(d[0], d[2]) for d in info["lines"]) and any(min(d[0], d[2]) >= 2048 for d in info["lines"])
        assert ref["n_mask_px"] == int((lsd == 255).sum()) > 0
        # the quadrant images
        ocr = ref["ocr"]
        assert ocr.shape == (qh, qw) and (ocr[:, 0] == 0).any() and (ocr[:, qw - 1] == 0).any() and (ocr[1] == 0).any() and (ocr[qh - 1] == 0).any()
        assert ocr[2, 0] == 255 - 135 and ocr[2, qw - 1] == 255 - 135                # greys kept through a white neighbour
        if info["bar"] is not None:
            (xl, xr, yb), (m, ax, ay) = info["bar"]
            assert ref["mpx"] == m / float(xr - xl - 2), (ref["mpx"], xl, xr)
            assert o.find_scale_width(m, ax, ay, ref["scales"])[1][:3] == (xl + 1, yb, xr - 1)
        else:
            assert ref["mpx"] is None
        assert np.array_equal(ref["ui_colour"][..., :3], f[_roi(c)][..., 2::-1]) and (ref["ui_colour"][..., 3] == 255).all()
        assert (ref["ui_map"][..., 3] == 255).all()


def _roi(c):
    d = G.derive(c.W, c.H)
    return (slice(d["ry"], d["ry"] + c.rh), slice(d["rx"], d["rx"] + c.rw))


def _covers(ln, drawn):
    """An oracle line that lies along the drawn one (both ends within 4 px across) over more than 50 px of it."""
    xa, ya, xb, yb = [float(v) for v in drawn]
    L = np.hypot(xb - xa, yb - ya)
    ux, uy = (xb - xa) / L, (yb - ya) / L
    t, d = [], []
    for (x, y) in ((ln[0], ln[1]), (ln[2], ln[3])):
        t.append((float(x) - xa) * ux + (float(y) - ya) * uy)
        d.append(abs(-(float(x) - xa) * uy + (float(y) - ya) * ux))
    return max(d) <= 4 and min(max(t), L) - max(min(t), 0.0) > 50


@pytest.mark.parametrize("c", [c for c in G.CASES if c.rw <= 2049], ids=[i for i, c in zip(G.IDS, G.CASES) if c.rw <= 2049])
def test_oracle_ignores_the_alpha_byte(o, c):
    """Frame 0 carries alpha 255, frame 2 random alpha: each with the other's alpha gives the same images and record."""
    frames, infos, refs = G.oracle_of(c)
    rng = np.random.default_rng(c.W * 7 + c.H)
    for i in (0, 2):
        f = frames[i].copy()
        f[..., 3] = 255 if i == 2 else rng.integers(0, 256, f.shape[:2], dtype=np.uint8)
        assert not np.array_equal(f[..., 3], frames[i][..., 3])
        for gray in (True, False):
            a = o.process_frame(f, grayscale=gray, max_gap=G.MAX_GAP, stages=0xF, anchors=infos[i]["anchors"] or None,
                                scales_start_y=infos[i]["scales_start_y"], want_images=True)
            want_ui = refs[i]["ui_map"] if gray else refs[i]["ui_colour"]
            assert np.array_equal(a["ui_map"], want_ui)
            for k in ("lsd", "ocr", "scales", "lines"):
                assert np.array_equal(a[k], refs[i][k]), (i, k)
            assert (a["map_open"], a["n_lines"], a["mpx"], a["n_mask_px"], a["rounds"], a["steps"]) == \
                tuple(refs[i][k] for k in ("map_open", "n_lines", "mpx", "n_mask_px", "rounds", "steps"))
        assert o.find_minimap(f) == refs[i]["minimap"] and o.button_red_pixels(f) == refs[i]["red_pixels"]


def _lib_bounds(fn, W, H):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    try:
        return tuple(int(v) for v in fn(W, H))
    except smh.VisionError as e:
        assert e.code == _lib.E_GEOMETRY, (W, H, e)
        return None


def test_library_and_oracle_refuse_the_same_sizes(o):
    """smh.map_bounds / button_bounds against the oracle's decision on a dense sweep across each limit: rw 6..10 and w(H) > W at
    every m_xoff, heights down to where the ROI and its quadrant vanish, the button wider than the frame.  The library's own extra
    limit (rw + m_xoff <= 4096) is not the reference's: the oracle accepts those sizes, FrameBatch refuses them (the GPU file)."""
    import squad_mortar_helper_amd as smh
    refused = accepted = 0
    sizes = [(W, H) for H in range(355, 372) for W in range(int(0.86 * H) - 4, int(0.87 * H) + 14)]
    sizes += [(W, H) for H in range(1, 40) for W in (1, 2, 3, 7, 8, 9, 16, 40, 64)]
    sizes += [(W, H) for H in (360, 1080, 1440) for W in range(1, 12)] + [(W, 1080) for W in range(250, 270)]
    sizes += [(c.W, c.H) for c in G.CASES] + [(W, H) for W, H, _ in G.REFUSED]
    for W, H in sizes:
        want, got = o.map_bounds(W, H), _lib_bounds(smh.map_bounds, W, H)
        assert got == want, ("map", W, H, got, want)
        wb, gb = o.button_bounds(W, H), _lib_bounds(smh.button_bounds, W, H)
        assert gb == wb, ("button", W, H, gb, wb)
        refused += want is None
        accepted += want is not None
        if want is not None:
            assert want[2] >= 8 and want[3] >= 8 and want[2] // 2 >= 3 and want[3] // 2 >= 3      # no accepted ROI has a quadrant under 3 px
    assert refused >= 100 and accepted >= 100, (refused, accepted)
    for H in range(355, 372):                                           # the edge itself, at every m_xoff
        w = smh.map_bounds(2000, H)[2]
        w = 2000 - w                                                    # w(H)
        assert o.map_bounds(w + 7, H) is None and _lib_bounds(smh.map_bounds, w + 7, H) is None
        assert o.map_bounds(w + 8, H)[2] == 8 == smh.map_bounds(w + 8, H)[2]
        assert o.map_bounds(w - 1, H) is None and _lib_bounds(smh.map_bounds, w - 1, H) is None


def test_band_rule_switches_between_900_and_901_rows(built):
    """smhv_debug_band_rows (host logic): a launch that fills the chip takes 24-row bands with the tile-major mask up to rh = 900, the
    fused kernel's 58 / the plain kernel's 62 rows and bit rows only from 901 on (56 would cost a band more there); beside the search
    service 56 up to 900; a few frames: bands of 8 rows at every height."""
    from squad_mortar_helper_amd import _lib
    lib = _lib.load()

    def q(c, n, fused):
        rows, bands, tiles = C.c_uint32(), C.c_uint32(), C.c_int()
        _lib.check(lib.smhv_debug_band_rows(c.W, c.H, n, fused, C.byref(rows), C.byref(bands), C.byref(tiles)))
        assert bands.value == -(-c.rh // rows.value)
        return rows.value, bool(tiles.value)
    by_rh = {c.rh: c for c in G.HEIGHT_EDGE}
    assert sorted(by_rh) == [899, 900, 901, 902]
    for rh in (899, 900):
        assert q(by_rh[rh], 64, 1) == (24, True) and q(by_rh[rh], 64, 0) == (24, True) and q(by_rh[rh], 64, 2) == (56, True)
    for rh in (901, 902):
        assert -(-rh // 56) == 17 and -(-rh // 58) == 16 and -(-rh // 62) == 15
        assert q(by_rh[rh], 64, 1) == (58, False) and q(by_rh[rh], 64, 0) == (62, False) and q(by_rh[rh], 64, 2) == (58, False)
    for c in G.HEIGHT_EDGE:
        assert q(c, 3, 1) == (8, True) and q(c, 3, 0) == (8, True)
