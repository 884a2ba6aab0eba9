"""The ingest queue on the device at the edges tests/ingest_cases.py lists: k_to_bgra at every n_px % 4 and across its grid-stride
limit, the queue's own CRC launch with two rounds, the ROI upload's slab image byte for byte, a slab position reused by a frame of
another layout, the smallest queue.  Every comparison is exact.  tests/test_ingest_edges_host.py pins what is compared against."""
import ctypes as C
import zlib

import numpy as np
import pytest

import geometry_sweep_cases as G
import ingest_cases as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


def _d2h(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0            # hipMemcpyDeviceToHost
    return out


def _push_bgra(q, frame, k):
    """Odd k: from pageable memory; even k: straight into the pinned staging buffer."""
    if k % 2:
        q.push(frame)
    else:
        q.acquire()[...] = frame
        q.commit()


# ---- 1. decoder layouts ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", I.SIZES, ids=I.SIZE_IDS)
def test_decoder_layouts_at_every_residue_and_across_the_grid_stride_limit(vision, o, row):
    """13 commits per size (push_pixels and acquire / commit_pixels in turn, the staging buffer filled with a guard byte before an
    acquired frame's pixels go in): the 10 accepted slab frames equal into_bgra8 over the whole frame, crc32_device of each equals
    zlib's, batch() reports the last accepted frame's CRC, the same pixels in two layouts are dropped three times."""
    import squad_mortar_helper_amd as smh
    W, H = row.W, row.H
    nb = W * H * 4
    seq = I.decoder_sequence(W, H, W + H)
    keep, last = o.capture_dedupe([zlib.crc32(want.tobytes()) for _, _, _, want in seq])
    assert keep.tolist() == I.DECODER_KEEP
    q = smh.IngestQueue(vision, W, H, slots=3, capacity=int(keep.sum()))
    try:
        for lay, px, path, _ in seq:
            if path == "push":
                q.push_pixels(px, lay)
            else:
                buf = q.acquire().reshape(-1)
                buf[:] = I.GUARD                                     # bytes behind the source's end must never show in the output
                buf[:px.size] = px.reshape(-1)
                q.commit_pixels(lay)
        ptr, n, crc = q.batch()
        assert n == int(keep.sum()) == 10 and crc == last and q.counts() == (10, 3)
        slab = _d2h(ptr, n * nb).reshape(n, H, W, 4)
        for i, (lay, want) in enumerate([(s[0], s[3]) for s, k in zip(seq, keep) if k]):
            if not np.array_equal(slab[i], want):
                bad = np.nonzero((slab[i] != want).any(axis=-1).reshape(-1))[0]
                raise AssertionError("%dx%d frame %d (%s): %d pixels differ, first %d, last %d of %d" % (W, H, i, lay, bad.size, bad[0], bad[-1], W * H))
            assert smh.crc32_device(vision, ptr + i * nb, nb) == zlib.crc32(want.tobytes()), (i, lay)
    finally:
        q.close()


# ---- 2. the queue's CRC at two rounds ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("roi_upload", [False, True], ids=["device-crc", "host-crc"])
@pytest.mark.parametrize("row", I.LARGE, ids=["%dx%d" % (r.W, r.H) for r in I.LARGE])
def test_queue_crc_with_two_rounds_tells_single_bits_apart(vision, o, row, roi_upload):
    """A frame above 16 MiB and its copies with one bit flipped at byte 0, 15, 16, either side of the boundary between the two
    rounds' spans, and the last byte: 8 commits, every copy a new capture, the repeat of the last a duplicate; the CRC batch()
    reports is zlib's of the last.  The same through a ROI-upload queue (host CRC): the same decisions."""
    import squad_mortar_helper_amd as smh
    W, H = row.W, row.H
    assert I.crc_plan(W * H * 4)["rounds"] == 2
    frame = I.random_truth(W, H, 5)
    q = smh.IngestQueue(vision, W, H, slots=3, capacity=7, roi_upload=roi_upload)
    try:
        crcs = []
        for k, (what, f) in enumerate(I.crc_flip_sequence(frame)):
            crcs.append(zlib.crc32(f.tobytes()))
            q.push(f)                                                # (copies the frame into staging before it returns)
            ptr, n, crc = q.batch()
            assert (n, crc) == (min(k + 1, 7), crcs[-1]), (what, n, hex(crc), hex(crcs[-1]))
        keep, last = o.capture_dedupe(crcs)
        assert keep.tolist() == I.CRC_FLIP_KEEP and q.counts() == (7, 1) and q.batch()[2] == last
        if not roi_upload:                                           # the slab holds the seven copies: the last differs from the base in one bit
            nb = W * H * 4
            assert smh.crc32_device(vision, ptr, nb) == crcs[0] and smh.crc32_device(vision, ptr + 6 * nb, nb) == crcs[6]
    finally:
        q.close()


# ---- 3. ROI upload: the exact slab image ---------------------------------------------------------------------------------------------

def _records_and_images(vision, c, ptr, n, per, image_frames):
    """FrameBatch.run over n frames at ptr, all stages with anchors -> (record bytes [n], dicts [n], {frame: {name: image}})."""
    import squad_mortar_helper_amd as smh
    L = smh._lib
    fb = smh.FrameBatch(vision, c.W, c.H, n)
    try:
        fb.run(ptr, n, stages=smh.STAGE_ALL, max_gap=G.MAX_GAP, anchors=smh.make_anchors(per))
        recs = fb.read_results(0, n)
        raw = [bytes(r) for r in recs]
        dicts = smh.results_to_dicts(recs)
        images = {f: dict(ui_map=fb.read_image(L.IMAGE_UI_MAP, f), lsd=fb.read_image(L.VIEW_LSD_INPUT, f), ocr=fb.read_image(L.VIEW_OCR_INPUT, f),
                          scales=fb.read_image(L.VIEW_FIND_SCALES_INPUT, f)) for f in image_frames}
    finally:
        fb.close()
    return raw, dicts, images


@pytest.mark.parametrize("row", I.ROI_ROWS, ids=I.ROI_IDS)
def test_roi_upload_leaves_exactly_the_two_rectangles(vision, o, row):
    """7 commits per size (open, its duplicate, closed, open, the same but for a byte outside both rectangles, its duplicate, open):
    the 5 accepted slab frames equal expected_slab_frame over the WHOLE frame; one FrameBatch.run over the slab gives records
    byte-equal to a run over the same frames uploaded whole, the oracle's records and the oracle's images."""
    import torch
    import squad_mortar_helper_amd as smh
    from test_geometry_sweep_gpu import _check_record
    c = I.sweep_case(row.W, row.H)
    W, H, nb = c.W, c.H, c.W * c.H * 4
    frames, infos, ref_of = I.roi_frames(c)
    _, _, refs = G.oracle_of(c)
    seq = [frames[i] for i in I.ROI_SEQ]
    keep, last = o.capture_dedupe([zlib.crc32(f.tobytes()) for f in seq])
    assert keep.tolist() == I.ROI_KEEP
    kept = [i for i, k in zip(I.ROI_SEQ, keep) if k]
    q = smh.IngestQueue(vision, W, H, slots=4, capacity=len(kept), roi_upload=True)
    try:
        for k, f in enumerate(seq):
            _push_bgra(q, f, k)
        ptr, n, crc = q.batch()
        assert n == len(kept) == 5 and crc == last and q.counts() == (5, 2)
        slab = _d2h(ptr, n * nb).reshape(n, H, W, 4)
        for i, fi in enumerate(kept):
            assert np.array_equal(slab[i], I.expected_slab_frame(frames[fi], c, "bgra")), (W, H, i)
        per = [(infos[fi]["scales_start_y"], infos[fi]["anchors"]) for fi in kept]
        raw, dicts, images = _records_and_images(vision, c, ptr, n, per, range(n))
        whole = torch.from_numpy(np.stack([frames[fi] for fi in kept])).cuda()
        raw_w, _, images_w = _records_and_images(vision, c, whole.data_ptr(), n, per, range(n))
        assert raw == raw_w
        for i, fi in enumerate(kept):
            ref, info = refs[ref_of[fi]], infos[fi]
            _check_record(dicts[i], ref, info, smh.STAGE_ALL, (W, H, i))
            if not ref["map_open"]:
                continue
            y0 = info["scales_start_y"]
            for name in ("ui_map", "lsd", "ocr"):
                assert np.array_equal(images[i][name], ref[name]) and np.array_equal(images_w[i][name], ref[name]), (W, H, i, name)
            if info["anchors"]:
                assert np.array_equal(images[i]["scales"][y0:], ref["scales"][y0:]), (W, H, i, "scales")
        del whole
    finally:
        q.close()


# ---- 4. slab history -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["bgra-then-video", "video-then-bgra"])
@pytest.mark.parametrize("row", I.HISTORY_ROWS, ids=["%dx%d" % (r.W, r.H) for r in I.HISTORY_ROWS])
def test_slab_position_reused_by_a_frame_of_another_layout(vision, row, order):
    """ROI-upload queue, 4 positions: slab 1 in one layout, reset(), slab 2 in the other at the same positions.  A BGRA commit
    copies whole quads, a video commit exactly the ROI.  BGRA then video: slab 1 holds frames of marker colour from edge to edge,
    so the up-to-three columns either side of a video frame's ROI still hold marker pixels.  Video then BGRA: slab 2 holds
    ordinary scenes.  In both orders the slab is, byte for byte, the second layout's rectangles over the first's, and slab 2's
    records (all stages, with anchors) and every image the API reads (ui_map, mask, ocr, scales) are those of the same frames --
    the converted ones for video -- uploaded whole: nothing depends on what stands beside the ROI.  The video rectangles are
    yuv_ref.to_bgra's."""
    import torch
    import squad_mortar_helper_amd as smh
    c = I.sweep_case(row.W, row.H)
    W, H, nb = c.W, c.H, c.W * c.H * 4
    d = I.roi_numbers(W, H)
    loud, video, scenes = I.history_frames(c)
    n = len(loud)
    first, second = ("bgra", "video") if order == "bgra-then-video" else ("video", "bgra")
    bgra = loud if first == "bgra" else [f for f, _ in scenes]        # (loud where it leaves the stale columns, scenes where every stage runs on it)

    def feed(q, what):
        for k in range(n):
            if what == "bgra":
                _push_bgra(q, bgra[k], k)
            elif k % 2:
                q.push_pixels(video[k][1], video[k][0], **I.YUV_KW)
            else:
                q.acquire().reshape(-1)[:video[k][1].size] = video[k][1]
                q.commit(video[k][0], **I.YUV_KW)
    q = smh.IngestQueue(vision, W, H, slots=3, capacity=n, roi_upload=True)
    try:
        feed(q, first)
        assert q.batch()[1] == n
        q.reset()
        feed(q, second)
        ptr, got_n, _ = q.batch()
        assert got_n == n and q.counts() == (2 * n, 0)
        slab = _d2h(ptr, n * nb).reshape(n, H, W, 4)
        rows, roi = slice(d["ry"], d["ry"] + d["rh"]), slice(d["rx"], d["rx"] + d["rw"])
        for k in range(n):
            lay, _, conv, _ = video[k]
            want = np.zeros((H, W, 4), np.uint8)
            for what in (first, second):
                I.overlay_slab_frame(want, bgra[k] if what == "bgra" else conv, d, "bgra" if what == "bgra" else lay)
            assert np.array_equal(slab[k], want), (W, H, order, k)
            if second == "video":                                     # the rectangles are the restated conversion's, the columns beside them stale
                assert np.array_equal(slab[k][rows, roi], conv[rows, roi])
                assert np.array_equal(slab[k][rows, d["m_ax"]:d["rx"]], loud[k][rows, d["m_ax"]:d["rx"]]) and d["rx"] > d["m_ax"]
            else:
                assert np.array_equal(slab[k], I.expected_slab_frame(bgra[k], c, "bgra"))      # a BGRA commit covers all a video commit wrote
        direct = [video[k][2] for k in range(n)] if second == "video" else bgra
        infos = [v[3] for v in video] if second == "video" else [i for _, i in scenes]
        per = [(i["scales_start_y"], i["anchors"]) for i in infos]
        raw, dicts, images = _records_and_images(vision, c, ptr, n, per, range(n))
        whole = torch.from_numpy(np.stack(direct)).cuda()
        raw_w, dicts_w, images_w = _records_and_images(vision, c, whole.data_ptr(), n, per, range(n))
        assert all(r["map_open"] == 1 and r["n_mask_px"] > 0 for r in dicts_w)
        assert raw == raw_w, (W, H, order)
        for k in range(n):
            for name in ("ui_map", "lsd", "ocr", "scales"):
                assert np.array_equal(images[k][name], images_w[k][name]), (W, H, order, k, name)
        del whole
    finally:
        q.close()


# ---- 5. the smallest queue ---------------------------------------------------------------------------------------------------------------

def test_smallest_queue_keeps_a_frame_queued_behind_a_full_slab(vision):
    """slots = 2, capacity = 1: a new frame behind a full slab stays queued, reset() then batch() delivers it; with both staging
    slots holding a queued frame a further push is refused with SMHV_E_STATE and loses nothing."""
    import squad_mortar_helper_amd as smh
    W, H = I.SMALLEST
    nb = W * H * 4
    A, B, Cc, D = [I.random_truth(W, H, 90 + i) for i in range(4)]
    crc = lambda f: zlib.crc32(f.tobytes())                           # noqa: E731
    q = smh.IngestQueue(vision, W, H, slots=2, capacity=1)
    try:
        q.push(A)
        q.push(B)
        ptr, n, last = q.batch()
        assert (n, last, q.counts()) == (1, crc(A), (1, 0)) and np.array_equal(_d2h(ptr, nb), A.reshape(-1))
        assert q.batch()[1:] == (1, crc(A))                          # (asking again changes nothing: B is still queued)
        q.push(Cc)                                                    # A's staging slot is free: C is queued behind B
        with pytest.raises(smh.VisionError) as e:
            q.push(D)
        assert e.value.code == smh._lib.E_STATE and q.counts() == (1, 0)
        q.reset()
        ptr, n, last = q.batch()
        assert (n, last, q.counts()) == (1, crc(B), (2, 0)) and np.array_equal(_d2h(ptr, nb), B.reshape(-1))
        q.reset()
        q.push(Cc)                                                    # a duplicate of the queued C: resolved behind it, dropped
        ptr, n, last = q.batch()
        assert (n, last, q.counts()) == (1, crc(Cc), (3, 1)) and np.array_equal(_d2h(ptr, nb), Cc.reshape(-1))
        q.reset()
        assert q.batch()[1:] == (0, crc(Cc))
    finally:
        q.close()
