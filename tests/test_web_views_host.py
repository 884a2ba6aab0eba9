"""A debug view as the remote-viewer feed's Map, on the host (no GPU): the numpy restatement of the view bytes
(tests/web_views_ref.py) against the oracle on two golden fixtures and a synthetic frame, the worst-case capacity per source, the
coverage the device tests' frame sizes give, the rule when the source switches, and the new entry points' argument checks that
need no device."""
import zlib

import numpy as np
import pytest

import fixtures as fx
import web_ref as W
import web_views_ref as V
from oracle import oracle as o


def _oracle_planes(frame, start_y):
    c = o.crop_to_map(frame, grayscale=False)
    assert c is not None
    iso = o.isolate_map_markers(c["cropped_map"])
    return dict(ui=c["ui_map"], map=c["cropped_map"], brq=c["cropped_brq"], iso=iso, mask=o.mask_marker_lines(iso), ocr=o.ocr_preprocess(c["cropped_brq"]),
                scales=o.find_scales_preprocess(c["cropped_brq"], start_y))


def _frames():
    from squad_mortar_helper_amd import synth
    out = []
    for stem in ("point_intersect_png", "full_1600x1024_png"):  # real scale bars at 1440p; a 714-column map with 303 marker pixels
        frame, e, _ = fx.load_fixture(stem)
        out.append((stem, frame, int(e.get("scales_start_y") or 0)))
    frame, info = synth.make_frame(568, 361, frame_idx=31 + 568)
    out.append(("synthetic 568 x 361", frame, info["scales_start_y"]))
    return out


@pytest.mark.parametrize("case", range(3))
def test_view_bytes_against_the_oracle(built, case):
    name, frame, start_y = _frames()[case]
    p = _oracle_planes(frame, start_y)
    rh, rw = p["ui"].shape[:2]
    assert np.array_equal(p["ui"][..., :3], p["map"])                             # the colour ui_map is the cropped map
    alpha = lambda rgb: np.dstack([rgb, np.full(rgb.shape[:2], 255, np.uint8)])
    want = {V.VIEW_LSD_PREPROCESS: alpha(p["iso"]), V.VIEW_CROPPED_BRQ: alpha(p["brq"]), V.VIEW_LSD_INPUT: alpha(np.dstack([p["mask"]] * 3)),
            V.VIEW_OCR_INPUT: alpha(np.dstack([p["ocr"]] * 3)), V.VIEW_FIND_SCALES_INPUT: alpha(np.dstack([p["scales"]] * 3))}
    for which in V.VIEWS:
        w, h, data = V.view_bytes(which, ui=p["ui"], mask=p["mask"], ocr=p["ocr"], scales=p["scales"])
        assert (w, h) == V.view_size(which, rw, rh) == (want[which].shape[1], want[which].shape[0]), (name, which)
        got = np.frombuffer(data, np.uint8).reshape(h, w, 4)
        lo = start_y if which == V.VIEW_FIND_SCALES_INPUT else 0                  # (the scales image is defined from the start row on)
        assert np.array_equal(got[lo:], want[which][lo:]), (name, which)
        assert len(data) == w * h * 4 and np.all(got[..., 3] == 255)
    # the views are no trivial images: markers survive the isolation, the mask has set and clear pixels
    assert (p["iso"].any(axis=2)).sum() >= 100 and (p["mask"] == 255).sum() >= 100 and (p["mask"] == 0).sum() >= 100, name
    # the isolated view keeps exactly the pixels the oracle's predicate keeps
    keep = np.frombuffer(V.view_bytes(V.VIEW_LSD_PREPROCESS, ui=p["ui"])[2], np.uint8).reshape(rh, rw, 4)[..., :3].any(axis=2)
    assert np.array_equal(keep, p["iso"].any(axis=2)), name


def test_worst_case_capacity_per_source():
    for rw, rh in ((986, 822), (33, 276), (142, 275), (394, 779)):
        for which in (V.VIEW_NONE,) + V.VIEWS:
            w, h = (rw, rh) if which in (V.VIEW_NONE, V.VIEW_LSD_PREPROCESS, V.VIEW_LSD_INPUT) else (rw // 2, rh // 2)
            assert V.worst_case(which, rw, rh) == 6 + 32 + ((10 + w * h * 4 + 15) // 16) * 16 + 7 + 16 * 32, (rw, rh, which)
    assert V.worst_case(V.VIEW_NONE, 986, 822) == W.worst_case(986, 822) == 3242541
    assert V.worst_case(V.VIEW_CROPPED_BRQ, 986, 822) == V.worst_case(V.VIEW_OCR_INPUT, 986, 822) == 811069
    assert V.worst_case(V.VIEW_CROPPED_BRQ, 986, 822) < V.worst_case(V.VIEW_NONE, 986, 822)   # a feed can fit the quarter and not the map


def test_the_chosen_sizes_cover_the_residues(built):
    import squad_mortar_helper_amd as smh
    cov = V.check_coverage(smh.map_bounds)
    assert cov == list(zip(V.Q_XOFF, V.BRQ_W))
    assert smh.map_bounds(347, 363)[2] == 33                                      # the 16-pixel-wide quarter
    assert {smh.map_bounds(*s)[0] % 4 for s in V.SIZES} >= {0, 1, 2, 3}           # and every lead-in of the map's own rows
    assert V.FEED_ROWS == (0, 1, 3, 8, 64)


def test_one_stored_crc_whatever_the_source():
    """NONE -> LSD_INPUT -> LSD_INPUT -> NONE on one unchanged frame: the switch sends a Map, the repeat none, the switch back one."""
    rng = np.random.default_rng(5)
    ui = rng.integers(0, 256, size=(6, 10, 4), dtype=np.uint8)
    mask = (rng.integers(0, 2, size=(6, 10)) * 255).astype(np.uint8)
    lines = np.zeros((0, 4), np.float32)
    fr = lambda vb: [(True, 0, vb, lines, False, 0.0, False, (0, 0, 0, 0))]
    none, lsd = (10, 6, ui.tobytes()), V.view_bytes(V.VIEW_LSD_INPUT, mask=mask)
    assert lsd[:2] == (10, 6) and lsd[2][:8] == bytes([mask[0, 0]] * 3 + [255] + [mask[0, 1]] * 3 + [255])
    stored, maps = None, []
    for vb in (none, lsd, lsd, none):
        r = W.feed(fr(vb), stored=stored)
        stored = r["stored"]
        maps.append(r["n_maps"])
        assert stored == zlib.crc32(vb[2])
    assert maps == [1, 1, 0, 1]


def test_argument_checks_that_need_no_device(built):
    from squad_mortar_helper_amd import _lib as L
    lib = L.load()
    assert lib.smhv_batch_feed_view(None, None, 0, 1, 0, L.VIEW_LSD_INPUT, None) == L.E_INVALID
    assert lib.smhv_feed_frame_view(None, None, None, 0, None, None, 0, L.VIEW_LSD_INPUT) != 0
    assert lib.smhv_debug_feed_gray_form(3) == L.E_INVALID
    assert lib.smhv_debug_feed_gray_form(4) == 0 and lib.smhv_debug_feed_gray_form(0) == 0
    assert (L.VIEW_NONE, L.VIEW_OCR_INPUT, L.VIEW_FIND_SCALES_INPUT, L.VIEW_LSD_PREPROCESS, L.VIEW_LSD_INPUT, L.VIEW_CROPPED_BRQ) == tuple(range(6))
    assert (V.VIEW_NONE,) + V.VIEWS == (0, 1, 2, 3, 4, 5)
