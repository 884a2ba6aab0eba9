"""CPU half of the ingest edge tests (tests/ingest_cases.py): the tables' self-checks, the oracle's into_bgra8 against pixels typed
out by hand, expected_slab_frame against rectangles written out by hand, and the oracle's duplicate rule on exactly the sequences
tests/test_ingest_edges_gpu.py feeds -- so that what the GPU file compares against is itself pinned.  No device."""
import zlib

import numpy as np
import pytest

import geometry_sweep_cases as G
import ingest_cases as I


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


def test_tables_state_what_the_bounds_and_the_launch_arithmetic_give(built):
    I.check_tables()
    I.check_decoder_sequence()


def test_table_self_check_notices_a_wrong_size_and_a_missing_purpose(built):
    with pytest.raises(AssertionError):
        I.check_tables(sizes=[r._replace(W=r.W + 1) if (r.W, r.H) == (454, 361) else r for r in I.SIZES])      # a typo in one width
    for drop in ((568, 361), (2233, 361), (454, 361), (343, 361), (3295, 1440), (2923, 1441)):
        with pytest.raises(AssertionError):
            I.check_tables(sizes=[r for r in I.SIZES if (r.W, r.H) != drop])
    with pytest.raises(AssertionError):
        I.check_tables(roi_rows=[r._replace(roi_px=r.roi_px - 1) if (r.W, r.H) == (454, 361) else r for r in I.ROI_ROWS])
    for drop in ((451, 360), (319, 360), (1365, 767), (1921, 1081)):
        with pytest.raises(AssertionError):
            I.check_tables(roi_rows=[r for r in I.ROI_ROWS if (r.W, r.H) != drop])


def test_restated_crc_plan_at_its_own_edges(built):
    p = I.crc_plan
    assert p(4) == dict(groups=1, wgs=1, G=1024, rounds=1, pad=4095, split=None)
    assert p(16 * 1024)["wgs"] == 1 and p(16 * 1024 + 4)["wgs"] == 2
    assert p(16 << 20) == dict(groups=1 << 20, wgs=1024, G=1 << 20, rounds=1, pad=0, split=None)
    q = p((16 << 20) + 4)                                              # one dword more: the first round holds that one dword
    assert (q["rounds"], q["pad"], q["split"]) == (2, (1 << 22) - 1, 4)
    big = p(3295 * 1440 * 4)
    assert (big["rounds"], big["pad"] % 4, big["split"]) == (2, 0, 4 * (3295 * 1440 - (1 << 22)))
    odd = p(2923 * 1441 * 4)
    assert (odd["rounds"], odd["pad"] % 4, odd["split"]) == (2, 1, 4 * (2923 * 1441 - (1 << 22)))
    assert p(2233 * 361 * 4)["pad"] % 4 == 3                           # an odd residue at one round: dword loads as well


# (layout, the pixels as the decoder hands them over, the BGRA bytes image 0.23's FromColor makes of them) -- typed by hand
HAND = {
    "rgba": ([(1, 2, 3, 4), (255, 0, 0, 0), (0, 255, 0, 255), (0, 0, 255, 128), (10, 20, 30, 40), (200, 100, 50, 25), (7, 7, 7, 7), (0, 0, 0, 0),
              (255, 255, 255, 255), (254, 1, 253, 2), (17, 34, 51, 68), (99, 98, 97, 96)],
             [(3, 2, 1, 4), (0, 0, 255, 0), (0, 255, 0, 255), (255, 0, 0, 128), (30, 20, 10, 40), (50, 100, 200, 25), (7, 7, 7, 7), (0, 0, 0, 0),
              (255, 255, 255, 255), (253, 1, 254, 2), (51, 34, 17, 68), (97, 98, 99, 96)]),
    "rgb": ([(1, 2, 3), (255, 0, 0), (0, 255, 0), (0, 0, 255), (10, 20, 30), (200, 100, 50), (7, 7, 7), (0, 0, 0), (255, 255, 255), (254, 1, 253),
             (17, 34, 51), (99, 98, 97)],
            [(3, 2, 1, 255), (0, 0, 255, 255), (0, 255, 0, 255), (255, 0, 0, 255), (30, 20, 10, 255), (50, 100, 200, 255), (7, 7, 7, 255), (0, 0, 0, 255),
             (255, 255, 255, 255), (253, 1, 254, 255), (51, 34, 17, 255), (97, 98, 99, 255)]),
    "l": ([0, 1, 2, 127, 128, 129, 200, 254, 255, 17, 99, 64],
          [(0, 0, 0, 255), (1, 1, 1, 255), (2, 2, 2, 255), (127, 127, 127, 255), (128, 128, 128, 255), (129, 129, 129, 255), (200, 200, 200, 255),
           (254, 254, 254, 255), (255, 255, 255, 255), (17, 17, 17, 255), (99, 99, 99, 255), (64, 64, 64, 255)]),
    "la": ([(0, 0), (1, 255), (2, 128), (127, 1), (128, 2), (129, 3), (200, 100), (254, 254), (255, 0), (17, 34), (99, 98), (64, 65)],
           [(0, 0, 0, 0), (1, 1, 1, 255), (2, 2, 2, 128), (127, 127, 127, 1), (128, 128, 128, 2), (129, 129, 129, 3), (200, 200, 200, 100),
            (254, 254, 254, 254), (255, 255, 255, 0), (17, 17, 17, 34), (99, 99, 99, 98), (64, 64, 64, 65)]),
    "bgra": ([(1, 2, 3, 4), (255, 0, 0, 0), (0, 255, 0, 255), (0, 0, 255, 128), (10, 20, 30, 40), (200, 100, 50, 25), (7, 7, 7, 7), (0, 0, 0, 0),
              (255, 255, 255, 255), (254, 1, 253, 2), (17, 34, 51, 68), (99, 98, 97, 96)],
             [(1, 2, 3, 4), (255, 0, 0, 0), (0, 255, 0, 255), (0, 0, 255, 128), (10, 20, 30, 40), (200, 100, 50, 25), (7, 7, 7, 7), (0, 0, 0, 0),
              (255, 255, 255, 255), (254, 1, 253, 2), (17, 34, 51, 68), (99, 98, 97, 96)]),
}


@pytest.mark.parametrize("layout", I.LAYOUTS)
def test_into_bgra8_on_pixels_typed_by_hand(o, layout):
    src, want = HAND[layout]
    assert len(src) == len(want) == 12
    px = np.array(src, np.uint8).reshape((3, 4) if layout == "l" else (3, 4, I.BPP[layout]))
    assert np.array_equal(o.into_bgra8(px, layout), np.array(want, np.uint8).reshape(3, 4, 4))


def test_sources_of_one_truth(o):
    """source(): each layout's pixels are cut from the truth, and what the slab must hold is the truth itself where the layout carries
    everything (rgba, bgra), the truth with alpha 255 (rgb), grey (l, la)."""
    t = I.random_truth(7, 5, 3)
    assert len(np.unique(t[..., 3])) > 8                               # (the alpha bytes are random)
    for lay in ("rgba", "bgra"):
        assert np.array_equal(I.source(t, lay)[1], t)
    px, want = I.source(t, "rgb")
    assert px.shape == (5, 7, 3) and np.array_equal(want[..., :3], t[..., :3]) and (want[..., 3] == 255).all()
    px, want = I.source(t, "la")
    assert px.shape == (5, 7, 2) and all(np.array_equal(want[..., k], t[..., 1]) for k in range(3)) and np.array_equal(want[..., 3], t[..., 3])
    px, want = I.source(t, "l")
    assert px.shape == (5, 7) and all(np.array_equal(want[..., k], t[..., 1]) for k in range(3)) and (want[..., 3] == 255).all()


def test_expected_slab_frame_on_rectangles_written_out_by_hand(built):
    """319 x 360: ROI columns 304..311 of rows 59..332 (m_xoff 0: a BGRA commit and a video commit copy the same), button columns
    231..315 of rows 343..356.  454 x 361: ROI columns 305..446 of rows 59..333; a BGRA commit copies 304..447."""
    for (W, H, rows, bgra_cols, yuv_cols, btn_rows, btn_cols) in ((319, 360, (59, 333), (304, 312), (304, 312), (343, 357), (231, 316)),
                                                                  (454, 361, (59, 334), (304, 448), (305, 447), (344, 358), (366, 451))):
        c = I.sweep_case(W, H)
        f = np.random.default_rng(W).integers(1, 256, (H, W, 4), dtype=np.uint8)      # (no zero byte: a copied pixel is never mistaken for an empty one)
        for layout, cols in (("bgra", bgra_cols), ("nv12", yuv_cols), ("i420", yuv_cols)):
            got = I.expected_slab_frame(f, c, layout)
            inside = np.zeros((H, W), bool)
            for y in range(rows[0], rows[1]):
                inside[y, cols[0]:cols[1]] = True
            for y in range(btn_rows[0], btn_rows[1]):
                inside[y, btn_cols[0]:btn_cols[1]] = True
            assert int(inside.sum()) == (rows[1] - rows[0]) * (cols[1] - cols[0]) + (btn_rows[1] - btn_rows[0]) * (btn_cols[1] - btn_cols[0])
            assert np.array_equal(got[inside], f[inside]) and not got[~inside].any(), (W, H, layout)
    # onto a position with a history: a video commit over a BGRA commit leaves the BGRA frame's columns 304 and 447
    c = I.sweep_case(454, 361)
    a, b = np.full((361, 454, 4), 11, np.uint8), np.full((361, 454, 4), 22, np.uint8)
    slab = I.expected_slab_frame(a, c, "bgra")
    I.overlay_slab_frame(slab, b, I.roi_numbers(454, 361), "nv12")
    assert (slab[59:334, 304] == 11).all() and (slab[59:334, 447] == 11).all() and (slab[59:334, 305:447] == 22).all() and not slab[59:334, 303].any()


def test_duplicate_rule_on_the_decoder_sequence(o):
    for row in I.SIZES[:4]:
        seq = I.decoder_sequence(row.W, row.H, row.W)
        keep, last = o.capture_dedupe([zlib.crc32(want.tobytes()) for _, _, _, want in seq])
        assert keep.tolist() == I.DECODER_KEEP and last == zlib.crc32(seq[-1][3].tobytes())
        for lay, px, _, want in seq:
            assert px.size == row.n_px * I.BPP[lay] and want.shape == (row.H, row.W, 4)


@pytest.mark.parametrize("row", I.LARGE, ids=["%dx%d" % (r.W, r.H) for r in I.LARGE])
def test_crc_end_cases_are_all_different_captures(o, row):
    crcs = I.check_crc_flips(row.W, row.H, 5)
    keep, last = o.capture_dedupe(crcs)
    assert keep.tolist() == I.CRC_FLIP_KEEP and last == crcs[-1]
    places = dict(I.crc_flip_places(row.n_px * 4))
    split = I.crc_plan(row.n_px * 4)["split"]
    assert (places["last byte of round 0"], places["first byte of round 1"]) == (split - 1, split) and places["last byte"] == row.n_px * 4 - 1


def test_duplicate_rule_on_the_roi_sequence_and_the_byte_outside(o):
    """The frame that differs in one byte outside both rectangles is a new capture with the outputs of the frame it was copied
    from; checked against the oracle at the narrowest ROI and at m_xoff 1."""
    for (W, H) in ((319, 360), (454, 361)):
        c = I.sweep_case(W, H)
        frames, infos, ref_of = I.roi_frames(c)
        keep, _ = o.capture_dedupe([zlib.crc32(frames[i].tobytes()) for i in I.ROI_SEQ])
        assert keep.tolist() == I.ROI_KEEP
        kw = dict(grayscale=True, max_gap=G.MAX_GAP, stages=0xF, anchors=infos[2]["anchors"] or None, scales_start_y=infos[2]["scales_start_y"], want_images=True)
        a, b = o.process_frame(frames[2], **kw), o.process_frame(frames[3], **kw)
        assert not np.array_equal(frames[2], frames[3]) and ref_of == [0, 1, 2, 2]
        assert all(np.array_equal(a[k], b[k]) for k in a) and o.button_red_pixels(frames[2]) == o.button_red_pixels(frames[3])
        closed = o.process_frame(frames[1], stages=0xF)
        assert closed["map_open"] == 0 and a["map_open"] == 1
        # what the slab keeps of a frame gives the oracle the same outputs as the frame: nothing outside the rectangles is read
        kept = o.process_frame(I.expected_slab_frame(frames[2], c, "bgra"), **kw)
        assert all(np.array_equal(a[k], kept[k]) for k in a)


def test_history_frames_are_what_the_history_test_needs(o):
    """The loud frames are open and full of marker pixels right up to the ROI's edge columns; the video frames' converted BGRA is
    open and holds marker pixels (so the outputs compared on the device are not empty)."""
    c = I.sweep_case(453, 362)
    loud, video, scenes = I.history_frames(c)
    d = I.roi_numbers(c.W, c.H)
    assert len({zlib.crc32(f.tobytes()) for f in loud}) == len(loud) and {v[0] for v in video} == {"nv12", "i420"}
    for f in loud:
        assert o.process_frame(f, stages=0x2)["map_open"] == 1          # (no line search: a mask that is white all over takes it minutes)
        assert all(o.is_any_map_marker_color(int(f[d["ry"] + 5, x, 2]), int(f[d["ry"] + 5, x, 1]), int(f[d["ry"] + 5, x, 0])) for x in (d["m_ax"], d["rx"] - 1, d["rx"] + d["rw"]))
    for f, info in scenes:                                            # the BGRA slab 2 of the reverse order: ordinary scenes, every stage has work
        ref = o.process_frame(f, stages=0xF, anchors=info["anchors"] or None, scales_start_y=info["scales_start_y"])
        assert ref["map_open"] == 1 and ref["n_lines"] >= 1 and ref["n_mask_px"] > 0 and (ref["mpx"] is not None) == bool(info["anchors"])
    assert len({zlib.crc32(f.tobytes()) for f, _ in scenes}) == len(scenes)
    for lay, tight, bgra, info in video:
        ref = o.process_frame(bgra, stages=0x3)
        assert ref["map_open"] == 1 and ref["n_mask_px"] > 0 and tight.size == c.W * c.H + 2 * ((c.W + 1) // 2) * ((c.H + 1) // 2)
