"""NV12 / I420 frames on the device: smhv_yuv_to_bgra_device and the ingest queue's two video layouts against the restatement of
the header's arithmetic (tests/yuv_ref.py), byte for byte, and through the pipeline against the CPU oracle."""
import ctypes as C
import zlib

import numpy as np
import pytest

import yuv_cases as yc
import yuv_ref as yr
from oracle import oracle as o

pytestmark = pytest.mark.gpu

GUARD = 0xCD
KW1 = dict(matrix="709", full_range=False, chroma="nearest")
KW2 = dict(matrix="601", full_range=True, chroma="bilinear")


def _d2h(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0            # hipMemcpyDeviceToHost
    return out


def _lines(r):
    return np.array([[l.x0, l.y0, l.x1, l.y1] for l in r.lines[:r.n_lines]], np.float32).reshape(-1, 4)


# ---- 1. the conversion ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chroma", ["nearest", "bilinear"])
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_conversion_equals_the_restatement_in_every_layout_and_alignment(vision, layout, chroma):
    """Every case x shape x pitch x source offset x output offset; n = 1 and 3 and the four table rows take turns so that every
    (case, shape, pitch) meets each of them.  The output buffer carries a guard pattern: nothing but the frames may change."""
    import torch
    from squad_mortar_helper_amd import yuv
    st = torch.cuda.Stream()
    calls = 0
    with torch.cuda.stream(st):
        dsrc = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        dout = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        assert dsrc.data_ptr() % 256 == 0 and dout.data_ptr() % 256 == 0
        for ci, case in enumerate(yc.CASES):
            for (w, h) in yc.SHAPES:
                fb = w * h * 4
                for pi, pk in enumerate(yc.PITCHES):
                    srcs = {n: yc.source(case, w, h, layout, pk, n) for n in (1, 3)}
                    for so in yc.SRC_OFFSETS:
                        matrix, full = yr.ROWS[(so + pi + ci) % 4]
                        px = yuv.pixels(layout, matrix, full, chroma)
                        for oi, oo in enumerate(yc.OUT_OFFSETS):
                            n = 3 if (so + oi) % 2 else 1
                            src, lay = srcs[n]
                            dsrc[so:so + src.size].copy_(torch.from_numpy(src.copy()), non_blocking=False)
                            stride = fb + 20 if n > 1 else 0
                            total = oo + (fb + 20) * (n - 1) + fb + 64
                            dout[:total].fill_(GUARD)
                            yuv.yuv_to_bgra(vision, dsrc.data_ptr() + so, n, w, h, px, layout=None if (pk == "tight" and n == 1) else lay,
                                            out_ptr=dout.data_ptr() + oo, out_stride=stride, stream=st.cuda_stream)
                            got = dout[:total].cpu().numpy()
                            want = np.full(total, GUARD, np.uint8)
                            for f in range(n):
                                want[oo + f * (fb + 20):oo + f * (fb + 20) + fb] = yc.expected(case, w, h, f, matrix, full, chroma).reshape(-1)
                            if not np.array_equal(got, want):
                                bad = np.nonzero(got != want)[0]
                                raise AssertionError("%s %dx%d pitch %s src+%d out+%d n=%d %s/%s: %d bytes differ, first at %d (frame bytes %d)"
                                                     % (case, w, h, pk, so, oo, n, matrix, full, bad.size, bad[0] - oo, fb))
                            calls += 1
    assert calls == len(yc.CASES) * len(yc.SHAPES) * len(yc.PITCHES) * len(yc.SRC_OFFSETS) * len(yc.OUT_OFFSETS)


# ---- 2. the rectangle form -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1024, 768), (1366, 768), (1365, 767)])
def test_roi_only_writes_the_two_rectangles_of_the_full_conversion_and_nothing_else(vision, size):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import yuv
    import geometry_sweep_cases as gs
    W, H = size
    assert any((c.W, c.H) == (1365, 767) for c in gs.CASES)         # the odd x odd size is one of the geometry sweep's
    x, y, rw, rh = smh.map_bounds(W, H)
    bx, by, bw, bh = smh.button_bounds(W, H)
    Y, U, V = yc.planes("random", W, H)
    rng = np.random.default_rng(W)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for k, (layout, chroma) in enumerate((("nv12", "nearest"), ("nv12", "bilinear"), ("i420", "nearest"), ("i420", "bilinear"))):
            matrix, full = yr.ROWS[k]
            full_bgra = yr.to_bgra(Y, U, V, matrix, full, chroma)
            yp, up = yc.pitches(("tight", "+1", "+3", "256")[k], W, H, layout)
            src, lay = yr.pack(Y, U, V, layout, y_pitch=yp, uv_pitch=up, gap=k)
            pre = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            dsrc = torch.from_numpy(np.concatenate([np.zeros(k, np.uint8), src])).cuda()
            dout = torch.from_numpy(pre).cuda()
            yuv.yuv_to_bgra(vision, dsrc.data_ptr() + k, 1, W, H, yuv.pixels(layout, matrix, full, chroma), layout=lay, out_ptr=dout.data_ptr(), roi_only=True,
                            stream=st.cuda_stream)
            got = dout.cpu().numpy()
            want = pre.copy()
            want[y:y + rh, x:x + rw] = full_bgra[y:y + rh, x:x + rw]
            want[by:by + bh, bx:bx + bw] = full_bgra[by:by + bh, bx:bx + bw]
            assert np.array_equal(got[y:y + rh, x:x + rw], want[y:y + rh, x:x + rw]), (layout, chroma, "map ROI")
            assert np.array_equal(got[by:by + bh, bx:bx + bw], want[by:by + bh, bx:bx + bw]), (layout, chroma, "button")
            assert np.array_equal(got, want), (layout, chroma, "outside the rectangles")


# ---- 3. / 4. the ingest queue ----------------------------------------------------------------------------------------------------

def _sequence():
    """[(layout, keywords, committed bytes, the BGRA the pipeline must see)]: repeats in NV12 and I420, BGRA commits between them,
    both colour descriptions, and a frame that differs from its predecessor in one Y byte outside both rectangles."""
    W, H = yc.VIDEO_W, yc.VIDEO_H
    a, b, c = yc.VIDEO_SEEDS

    def video(seed, layout, kw):
        Y, U, V = yc.video_frame(seed, kw["matrix"], kw["full_range"])
        return (layout, kw, yr.pack_tight(Y, U, V, layout), yc.video_bgra(seed, kw["matrix"], kw["full_range"], kw["chroma"]))
    Ya, Ua, Va = yc.video_frame(a)
    Yo = Ya.copy()
    Yo[0, 0] ^= 1                                                   # (0, 0) lies outside the map ROI and the button
    outside = ("nv12", KW1, yr.pack_tight(Yo, Ua, Va, "nv12"), yr.to_bgra(Yo, Ua, Va))
    bgra_b = yc.video_bgra(b)
    seq = [video(a, "nv12", KW1), video(a, "nv12", KW1), outside, outside, video(b, "i420", KW1), ("bgra", {}, bgra_b.reshape(-1), bgra_b),
           video(b, "i420", KW1), video(b, "i420", KW2), video(b, "i420", KW2), video(c, "nv12", KW2), video(c, "nv12", KW2), video(a, "i420", KW1)]
    assert W * H * 4 == bgra_b.size
    return seq


def _feed(q, seq):
    for k, (layout, kw, data, _) in enumerate(seq):
        if k % 2:
            q.push(data.reshape(q.h, q.w, 4)) if layout == "bgra" else q.push_pixels(data, layout, **kw)
        else:
            q.acquire().reshape(-1)[:data.size] = data
            q.commit(layout, **kw)


def _run_slab(vision, ptr, n):
    import squad_mortar_helper_amd as smh
    fb = smh.FrameBatch(vision, yc.VIDEO_W, yc.VIDEO_H, n)
    fb.run(ptr, n, stages=0x3)
    recs = fb.read_results(0, n)
    uis = [fb.read_image(smh._lib.IMAGE_UI_MAP, i) for i in range(n)]
    fb.close()
    return recs, uis


def _check_against_oracle(recs, uis, want):
    found = 0
    for r, ui, f in zip(recs, uis, want):
        ref = o.process_frame(np.ascontiguousarray(f), grayscale=True, max_gap=15, stages=0x3, want_images=True)
        assert r.map_open == ref["map_open"] == 1 and np.array_equal(_lines(r), ref["lines"]) and np.array_equal(ui, ref["ui_map"])
        found += len(ref["lines"])
    assert found >= 1


def test_plain_queue_converts_in_front_of_the_crc(vision):
    import squad_mortar_helper_amd as smh
    W, H = yc.VIDEO_W, yc.VIDEO_H
    nb = W * H * 4
    seq = _sequence()
    crcs = [zlib.crc32(f.tobytes()) for _, _, _, f in seq]         # of the CONVERTED bytes
    keep, last = o.capture_dedupe(crcs)
    want = [f for (_, _, _, f), k in zip(seq, keep) if k]
    assert keep.tolist() == [True, False, True, False, True, False, False, True, False, True, False, True]   # (the BGRA of b repeats b)
    q = smh.IngestQueue(vision, W, H, slots=3, capacity=8)
    _feed(q, seq)
    ptr, n, crc = q.batch()
    assert n == len(want) and crc == last and q.counts() == (len(want), len(seq) - len(want))
    for i, f in enumerate(want):
        assert np.array_equal(_d2h(ptr + i * nb, nb), f.reshape(-1)), i
        assert smh.crc32_device(vision, ptr + i * nb, nb) == zlib.crc32(f.tobytes())
    recs, uis = _run_slab(vision, ptr, n)
    _check_against_oracle(recs, uis, want)
    q.close()


def test_roi_upload_queue_hashes_the_committed_bytes_and_converts_the_packed_rows(vision):
    import squad_mortar_helper_amd as smh
    W, H = yc.VIDEO_W, yc.VIDEO_H
    nb = W * H * 4
    x, y, rw, rh = smh.map_bounds(W, H)
    bx, by, bw, bh = smh.button_bounds(W, H)
    seq = _sequence()
    crcs = [zlib.crc32(d.tobytes()) for _, _, d, _ in seq]         # of the COMMITTED bytes
    keep, last = o.capture_dedupe(crcs)
    assert keep.tolist() == [True, False, True, False, True, True, True, True, False, True, False, True]
    # (the frame with one Y byte changed outside both rectangles is new; so is the BGRA of b after b, and b after it, where the plain
    # queue saw the same pixels three times)
    want = [(lay, f) for (lay, _, _, f), k in zip(seq, keep) if k]
    q = smh.IngestQueue(vision, W, H, slots=4, capacity=8, roi_upload=True)
    _feed(q, seq)
    ptr, n, crc = q.batch()
    assert n == len(want) and crc == last and q.counts() == (len(want), len(seq) - len(want))
    for i, (lay, f) in enumerate(want):
        got = _d2h(ptr + i * nb, nb).reshape(H, W, 4)
        assert np.array_equal(got[y:y + rh, x:x + rw], f[y:y + rh, x:x + rw]) and np.array_equal(got[by:by + bh, bx:bx + bw], f[by:by + bh, bx:bx + bw]), i
        if lay != "bgra":                                           # (a BGRA commit copies whole quads: up to 3 more columns)
            rest = got.copy()
            rest[y:y + rh, x:x + rw] = 0
            rest[by:by + bh, bx:bx + bw] = 0
            assert not rest.any(), i
    recs, uis = _run_slab(vision, ptr, n)
    _check_against_oracle(recs, uis, [f for _, f in want])
    # the records equal the plain queue's: the same sequence through a plain queue, frames matched by the pixels they hold (the
    # plain queue drops the BGRA of b and the b after it, which are the same pixels as the b before them)
    p = smh.IngestQueue(vision, W, H, slots=3, capacity=8)
    _feed(p, seq)
    pptr, pn, _ = p.batch()
    conv = [zlib.crc32(f.tobytes()) for _, _, _, f in seq]
    pkeep, _ = o.capture_dedupe(conv)
    assert pn == int(pkeep.sum())
    precs, puis = _run_slab(vision, pptr, pn)
    plain = {c: (bytes(r), ui) for c, r, ui in zip([c for c, k in zip(conv, pkeep) if k], precs, puis)}
    for i, c in enumerate([c for c, k in zip(conv, keep) if k]):
        assert bytes(recs[i]) == plain[c][0] and np.array_equal(uis[i], plain[c][1]), i
    p.close()
    # a full slab: the surplus stays queued in its staging slots, nothing is lost -- with YUV commits
    q.reset()
    Ya, Ua, Va = yc.video_frame(yc.VIDEO_SEEDS[0])
    base = yr.pack_tight(Ya, Ua, Va, "i420")
    more = []
    for i in range(8 + 4):
        m = base.copy()
        m[0] = (int(base[0]) + 1 + i) % 256                       # Y of pixel (0, 0): every frame differs from the one before it
        more.append(m)
        q.push_pixels(m, "i420", chroma="bilinear")
    with pytest.raises(smh.VisionError) as ei:
        q.push_pixels(base, "i420")
    assert ei.value.code == smh._lib.E_STATE
    assert q.batch()[1] == 8
    q.reset()
    ptr, n, crc = q.batch()
    assert n == 4 and crc == zlib.crc32(more[-1].tobytes())
    Yl = Ya.copy()
    Yl[0, 0] = more[-1][0]
    last_bgra = yr.to_bgra(Yl, Ua, Va, chroma="bilinear")
    got = _d2h(ptr + 3 * nb, nb).reshape(H, W, 4)
    assert np.array_equal(got[y:y + rh, x:x + rw], last_bgra[y:y + rh, x:x + rw])
    q.acquire()
    with pytest.raises(smh.VisionError):                            # the four image-decoder layouts still need the plain queue
        q.commit_pixels("rgb")
    q.commit("nv12")
    q.close()


# ---- 5. converted frames feed the per-call path and a pipeline ---------------------------------------------------------------

def test_converted_frames_feed_load_frame_device_and_a_pipeline(vision):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import yuv
    W, H = yc.VIDEO_W, yc.VIDEO_H
    nb = W * H * 4
    seeds = yc.VIDEO_SEEDS
    src = np.concatenate([yr.pack_tight(*yc.video_frame(s), "nv12") for s in seeds])
    dsrc = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    frames = yuv.yuv_to_bgra(vision, dsrc.data_ptr(), len(seeds), W, H, yuv.pixels("nv12", chroma="bilinear"))
    want = [yc.video_bgra(s, chroma="bilinear") for s in seeds]
    assert np.array_equal(frames.cpu().numpy(), np.stack(want))
    n = len(seeds)
    fb = smh.FrameBatch(vision, W, H, n)
    fb.run(frames.data_ptr(), n, stages=0x3)
    plain = bytes(fb.read_results(0, n))
    recs = fb.read_results(0, n)
    for r, s in zip(recs, seeds):
        ref = yc.video_oracle(s, chroma="bilinear")
        assert r.map_open == 1 and np.array_equal(_lines(r), ref["lines"]) and len(ref["lines"]) >= 1
    p = smh.Pipeline(vision, W, H, n, depth=3)
    slot = p.submit(frames.data_ptr(), n, stages=0x3)
    p.wait()
    assert bytes(p.slots[slot].read_results(0, n)) == plain
    p.close()
    fb.close()
    vision.load_frame_device(frames.data_ptr() + 1 * nb, W, H)
    ui, roi = vision.crop_to_map(True)
    vision.isolate_map_markers(); vision.mask_marker_lines()
    ref = yc.video_oracle(seeds[1], chroma="bilinear")
    assert np.array_equal(ui, ref["ui_map"]) and np.array_equal(vision.find_marker_lines(15), ref["lines"])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_leave_the_output_untouched(vision):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib, yuv
    w, h = 64, 8
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((w * h * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = yuv.pixels("nv12")
    bad = [
        dict(pixels=7), dict(pixels=3), dict(pixels=5 | 1 << 11), dict(pixels=6 | 1 << 20),           # unknown layout, a decoder layout, unknown bits
        dict(layout=dict(y_pitch=w - 1)), dict(layout=dict(uv_pitch=w - 1)), dict(pixels=yuv.pixels("i420"), layout=dict(uv_pitch=w // 2 - 1)),   # short pitches
        dict(w=0), dict(h=0), dict(n=0),
        dict(out_stride=w * h * 4 - 4), dict(out_stride=w * h * 4 + 2), dict(out_off=2),
        dict(n=2, layout=dict(frame_stride=w * h)),                                                     # the second frame would start inside the first
        dict(layout=dict(v_offset=5)),                                                                  # NV12's V is not a plane of its own
        dict(src=0), dict(out=0), dict(flags=2),
    ]
    lib = _lib.load()
    for b in bad:
        lay = yuv.yuv_layout(**b["layout"]) if "layout" in b else None
        rc = lib.smhv_yuv_to_bgra_device(vision._ctx, C.c_void_p(b.get("src", src.data_ptr())), C.byref(lay) if lay is not None else None, b.get("n", 1), b.get("w", w),
                                         b.get("h", h), b.get("pixels", ok), C.c_void_p(b["out"] if "out" in b else out.data_ptr() + b.get("out_off", 0)),
                                         b.get("out_stride", 0), b.get("flags", 0), None)
        assert rc == _lib.E_INVALID, b
    with pytest.raises(smh.VisionError) as ei:
        yuv.yuv_to_bgra(vision, src.data_ptr(), 1, w, h, 5 | 1 << 12, out_ptr=out.data_ptr())
    assert ei.value.code == _lib.E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    # ... and the same call with good arguments works
    yuv.yuv_to_bgra(vision, src.data_ptr(), 1, w, h, ok, out_ptr=out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[w * h * 4:] == GUARD).all() and np.array_equal(got[:w * h * 4].reshape(h, w, 4), yr.to_bgra(np.zeros((h, w), np.uint8), np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8)))
    # the queue refuses the same words
    q = smh.IngestQueue(vision, yc.VIDEO_W, yc.VIDEO_H, slots=2, capacity=2)
    q.acquire()
    for word in (7, 5 | 1 << 11, 1 | 1 << 8):
        assert lib.smhv_ingest_commit_pixels(q._q, word) == _lib.E_INVALID
    q.commit()
    q.close()
