"""Video frames out on the device: smhv_bgra_to_yuv_device and smhv_batch_video against the restatement of the header's outbound
arithmetic (tests/yuv_out_ref.py), byte for byte, fill bytes included."""
import ctypes as C

import numpy as np
import pytest

import yuv_cases as yc
import yuv_out_cases as oc
import yuv_out_ref as yo
import yuv_ref as yr

pytestmark = pytest.mark.gpu

GUARD = oc.FILL
W, H, N = 1024, 768, 4
CLOSED = 2                                    # the frame of the batch whose map is closed


def _word(layout, matrix, full):
    from squad_mortar_helper_amd import yuv
    return yuv.pixels(layout, matrix, full)


def _members(lay):
    return {k: lay[k] for k in ("y_pitch", "uv_pitch", "u_offset", "v_offset", "frame_stride")}


def _tight(imgs, layout, matrix, full, rgba=True):
    """The restated tight frames of RGBA (or BGRA) images, one row per frame."""
    return np.stack([yo.pack_tight(*yo.convert(i, matrix, full, rgba), layout) for i in imgs])


# ---- 1. the conversion ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_conversion_equals_the_restatement_in_every_layout_and_alignment(vision, layout):
    """Every case x shape x the four table rows x BGRA / RGBA; the destination layouts and source placements (oc.variants) take
    turns so that every (case, shape) meets each of them.  The destination carries a guard pattern before, between and behind
    the planes' rows: nothing but the samples may change."""
    import torch
    from squad_mortar_helper_amd import yuv
    st = torch.cuda.Stream()
    calls, seen = 0, set()
    with torch.cuda.stream(st):
        dsrc = torch.empty(1 << 18, dtype=torch.uint8, device="cuda")
        dout = torch.empty(1 << 18, dtype=torch.uint8, device="cuda")
        assert dsrc.data_ptr() % 256 == 0 and dout.data_ptr() % 256 == 0
        for ci, case in enumerate(oc.CASES):
            for si, (w, h) in enumerate(oc.SHAPES):
                vs = oc.variants(w, h, layout)
                for k, ((matrix, full), rgba) in enumerate([(r, o) for r in yo.ROWS for o in (False, True)]):
                    vi = (ci + si + k) % oc.N_VARIANTS
                    v = vs[vi]
                    seen.add((case, w, h, vi))
                    n = v["n"]
                    src, pitch, stride = oc.source(case, w, h, n, v["src_pitch"], v["src_gap"])
                    frames = [oc.expected(case, w, h, f, matrix, full, rgba) for f in range(n)]
                    want, lay = yo.pack(frames, layout, base=v["base"], tail=64, fill=GUARD, **(v["members"] or {}))
                    so = v["src_off"]
                    dsrc[so:so + src.size].copy_(torch.from_numpy(src))
                    dout[:want.size].fill_(GUARD)
                    mem = None if v["members"] is None else dict(v["members"])
                    yuv.bgra_to_yuv(vision, dsrc.data_ptr() + so, n, w, h, _word(layout, matrix, full), rgba=rgba, src_pitch=pitch if v["src_pitch"] else 0,
                                    src_stride=stride if (v["src_gap"] or n > 1) else 0, layout=mem, out_ptr=dout.data_ptr() + v["base"], stream=st.cuda_stream)
                    got = dout[:want.size].cpu().numpy()
                    if not np.array_equal(got, want):
                        bad = np.nonzero(got != want)[0]
                        raise AssertionError("%s %dx%d variant %d %s/%s rgba=%s: %d bytes differ, first at %d (base %d, layout %s)"
                                             % (case, w, h, vi, matrix, full, rgba, bad.size, bad[0], v["base"], lay))
                    calls += 1
    assert calls == len(oc.CASES) * len(oc.SHAPES) * 8
    assert all((case, w, h, vi) in seen for case in oc.CASES for (w, h) in oc.SHAPES for vi in range(oc.N_VARIANTS))


def test_tensor_form_returns_tight_frames(vision):
    import torch
    from squad_mortar_helper_amd import yuv
    w, h, n = 33, 31, 3
    src, _, _ = oc.source("random", w, h, n, 0, 0)
    d = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    for layout in ("nv12", "i420"):
        out = yuv.bgra_to_yuv(vision, d.data_ptr(), n, w, h, _word(layout, "601", True))
        assert out.shape == (n, yo.tight_bytes(w, h)) and out.dtype == torch.uint8
        want = np.stack([yo.pack_tight(*oc.expected("random", w, h, f, "601", True, False), layout) for f in range(n)])
        assert np.array_equal(out.cpu().numpy(), want), layout


# ---- 2. round trip on the device -----------------------------------------------------------------------------------------------

def test_round_trip_on_the_device_equals_the_restatements_composition(vision):
    import torch
    from squad_mortar_helper_amd import yuv
    for (w, h) in [(33, 31), (130, 6), (64, 8), (5, 7)]:
        for k, (matrix, full) in enumerate(yo.ROWS):
            layout = ("nv12", "i420")[k & 1]
            for case in ("blocks", "random"):
                img = oc.image(case, w, h)
                d = torch.from_numpy(img.copy()).cuda()
                torch.cuda.synchronize()
                word = _word(layout, matrix, full)
                frames = yuv.bgra_to_yuv(vision, d.data_ptr(), 1, w, h, word)
                back = yuv.yuv_to_bgra(vision, frames.data_ptr(), 1, w, h, word)
                Y, U, V = oc.expected(case, w, h, 0, matrix, full, False)
                want = yr.to_bgra(Y, U, V, matrix, full, "nearest")
                got = back.cpu().numpy()[0]
                assert np.array_equal(got, want), (w, h, matrix, full, case)
                if case == "blocks":                               # flat 2 x 2 blocks come back within the bound of the host test
                    lim = 2 if (not full or matrix == "601") else 1
                    assert np.abs(got[..., :3].astype(int) - img[..., :3]).max() <= lim, (w, h, matrix, full)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_leave_the_output_untouched(vision):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib, yuv
    w, h = 64, 8
    src = torch.zeros(w * h * 4 * 2 + 64, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = yuv.pixels("nv12")
    i420 = yuv.pixels("i420")
    bad = [
        dict(pixels=7), dict(pixels=3), dict(pixels=0), dict(pixels=5 | 1 << 11), dict(pixels=6 | 1 << 20),     # unknown layout, other layouts, unknown bits
        dict(pixels=5 | 1 << 10), dict(pixels=6 | 7 << 8),                                                    # the chroma bit must be 0 on output
        dict(layout=dict(y_pitch=w - 1)), dict(layout=dict(uv_pitch=w - 1)), dict(pixels=i420, layout=dict(uv_pitch=w // 2 - 1)),   # short pitches
        dict(w=0), dict(h=0), dict(n=0),
        dict(src_pitch=w * 4 - 4), dict(src_pitch=w * 4 + 2), dict(src_off=2), dict(src_stride=w * h * 4 + 2), dict(n=2, src_stride=w * h * 4 - 4),
        dict(n=2, layout=dict(frame_stride=w * h)),                                                           # the second frame would start inside the first
        dict(layout=dict(v_offset=5)),                                                                        # NV12's V is not a plane of its own
        dict(src=0), dict(out=0), dict(flags=2), dict(flags=1 << 31),
    ]
    lib = _lib.load()
    for b in bad:
        lay = yuv.yuv_layout(**b["layout"]) if "layout" in b else None
        rc = lib.smhv_bgra_to_yuv_device(vision._ctx, C.c_void_p(b["src"] if "src" in b else src.data_ptr() + b.get("src_off", 0)), b.get("src_pitch", 0),
                                         b.get("src_stride", 0), b.get("n", 1), b.get("w", w), b.get("h", h), b.get("flags", 0), b.get("pixels", ok),
                                         C.c_void_p(b["out"] if "out" in b else out.data_ptr()), C.byref(lay) if lay is not None else None, None)
        assert rc == _lib.E_INVALID, b
    with pytest.raises(smh.VisionError) as ei:
        yuv.bgra_to_yuv(vision, src.data_ptr(), 1, w, h, yuv.pixels("nv12", chroma="bilinear"), out_ptr=out.data_ptr())
    assert ei.value.code == _lib.E_INVALID
    assert lib.smhv_bgra_to_yuv_device(None, C.c_void_p(src.data_ptr()), 0, 0, 1, w, h, 0, ok, C.c_void_p(out.data_ptr()), None, None) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    # ... and the same call with good arguments works: black in limited range is Y 16, U = V = 128
    yuv.bgra_to_yuv(vision, src.data_ptr(), 1, w, h, ok, out_ptr=out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    nb = yo.tight_bytes(w, h)
    assert (got[:w * h] == 16).all() and (got[w * h:nb] == 128).all() and (got[nb:] == GUARD).all()


# ---- 4. the ui_map of a batch -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames(vision):
    """Four synthetic 1024 x 768 screenshots on the device, frame CLOSED with the map closed."""
    import torch
    from squad_mortar_helper_amd import synth
    f = np.stack([synth.make_frame(W, H, yc.VIDEO_SEEDS[i % 3] + 10 * (i // 3), n_lines=2, map_open=i != CLOSED)[0] for i in range(N)])
    d = torch.from_numpy(f).cuda()
    torch.cuda.synchronize()
    yield d
    del d


@pytest.fixture(scope="module")
def open_frames(frames):
    """The same with frame CLOSED replaced by an open one (a copy of the last frame)."""
    import torch
    d = frames.clone()
    d[CLOSED] = frames[N - 1]
    torch.cuda.synchronize()
    yield d
    del d


def _ui_images(fb):
    import squad_mortar_helper_amd as smh
    return [fb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)]


def _check_ui_video(fb, want_imgs, what):
    """video("ui_map") in both layouts and two colour rows against the restatement of the images."""
    rw, rh = fb.roi[2:]
    for layout, (matrix, full) in (("nv12", ("709", False)), ("i420", ("601", True))):
        got = fb.video("ui_map", _word(layout, matrix, full)).cpu().numpy()
        want = _tight(want_imgs, layout, matrix, full)
        assert got.shape == (N, yo.tight_bytes(rw, rh)) and np.array_equal(got, want), (what, layout)


def test_batch_ui_map_colour_then_grey_reads_the_form_that_is_current(vision, frames, open_frames):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib, yuv
    fb = smh.FrameBatch(vision, W, H, N)
    try:
        with pytest.raises(smh.VisionError) as ei:                     # no run has produced a ui_map
            fb.video("ui_map", _word("nv12", "709", False))
        assert ei.value.code == _lib.E_STATE
        # a colour run with every map open: every frame in the RGBA slab
        fb.run(open_frames.data_ptr(), N, stages=0x3, grayscale=False)
        assert [r["map_open"] for r in smh.results_to_dicts(fb.read_results(0, N))] == [1] * N
        state = fb.ui_state()
        got_before = fb.video("ui_map", _word("nv12", "709", False)).cpu().numpy()
        assert fb.ui_state() == state == (0, False)
        colour = _ui_images(fb)
        assert all(c.any() for c in colour)
        assert any(not np.array_equal(c[..., 0], c[..., 1]) for c in colour)          # really colour
        assert np.array_equal(got_before, _tight(colour, "nv12", "709", False))
        _check_ui_video(fb, colour, "colour")
        # a grey run that finds frame CLOSED closed: the open frames now lie in the luma plane, the closed one keeps its colour image in
        # the RGBA slab -- one launch reads both forms
        fb.run(frames.data_ptr(), N, stages=0x3, grayscale=True)
        assert [r["map_open"] for r in smh.results_to_dicts(fb.read_results(0, N))] == [int(i != CLOSED) for i in range(N)]
        state = fb.ui_state()
        assert state == (N, False)                                     # the RGBA slab is owed and nobody holds it
        got = {lay: fb.video("ui_map", _word(lay, m, f)).cpu().numpy() for lay, m, f in (("nv12", "709", False), ("i420", "601", True))}
        assert fb.ui_state() == state                                  # no expansion, no switch to eager RGBA
        # a sub-range into a pitched destination on a stream of the caller's
        import torch
        rw, rh = fb.roi[2:]
        lay = yo.resolve(rw, rh, "i420", n=2, y_pitch=rw + 3, uv_pitch=(rw + 1) // 2 + 1, frame_stride=0)
        lay = yo.resolve(rw, rh, "i420", n=2, y_pitch=rw + 3, uv_pitch=(rw + 1) // 2 + 1, frame_stride=lay["frame_end"] + 5)
        dst = torch.full((1 + lay["total"] + 32,), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert fb.video("ui_map", _word("i420", "709", True), first=1, n=2, out_ptr=dst.data_ptr() + 1, layout=_members(lay), stream=st.cuda_stream) is None
        st.synchronize()
        assert fb.ui_state() == state
        grey = _ui_images(fb)                                          # (this read makes the RGBA slab: the state moves now)
        assert fb.ui_state() == (0, False)
        assert np.array_equal(grey[CLOSED], colour[CLOSED])
        for i, g in enumerate(grey):
            if i != CLOSED:
                assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2]) and not np.array_equal(g, colour[i])
        assert np.array_equal(got["nv12"], _tight(grey, "nv12", "709", False)) and np.array_equal(got["i420"], _tight(grey, "i420", "601", True))
        want, _ = yo.pack([yo.convert(g, "709", True, True) for g in grey[1:3]], "i420", base=1, tail=32, fill=GUARD, **_members(lay))
        assert np.array_equal(dst.cpu().numpy(), want)
        # the open frames' Y is the grey formula of the luma byte and their chroma the constant 128
        Y, U, V = yo.unpack_tight(got["i420"][0], rw, rh, "i420")
        assert np.array_equal(Y, yo.grey(grey[0][..., 0], "601", True)) and (U == 128).all() and (V == 128).all()
        # after the expansion the same bytes come from the RGBA slab
        _check_ui_video(fb, grey, "grey, expanded")
        # a caller that holds d_ui: grey runs write RGBA themselves from now on; the same bytes again
        assert fb.device_ptrs()["ui"]
        assert fb.ui_state() == (0, True)
        fb.run(frames.data_ptr(), N, stages=0x3, grayscale=True)
        smh.results_to_dicts(fb.read_results(0, N))
        assert fb.ui_state() == (0, True)
        _check_ui_video(fb, grey, "grey, eager")
        assert fb.ui_state() == (0, True)
        assert all(np.array_equal(a, b) for a, b in zip(_ui_images(fb), grey))
        # refusals of the batch call
        lib = _lib.load()
        one = C.c_void_p(dst.data_ptr())
        for args in ((2, 0, 1, 5), (_lib.VIDEO_UI_MAP, 0, 0, 5), (_lib.VIDEO_UI_MAP, N, 1, 5), (_lib.VIDEO_UI_MAP, 0, N + 1, 5), (_lib.VIDEO_UI_MAP, 0, 1, 5 | 1 << 10),
                     (_lib.VIDEO_UI_MAP, 0, 1, 7)):
            assert lib.smhv_batch_video(fb._b, args[0], args[1], args[2], args[3], one, None, None) == _lib.E_INVALID, args
        assert lib.smhv_batch_video(fb._b, _lib.VIDEO_UI_MAP, 0, 1, 5, None, None, None) == _lib.E_INVALID
        assert lib.smhv_batch_video(fb._b, _lib.VIDEO_RENDER, 0, 1, 5, one, None, None) == _lib.E_STATE          # this batch has not rendered
    finally:
        fb.close()


# ---- 5. the render slab ----------------------------------------------------------------------------------------------------------

def test_batch_render_as_video(vision, frames):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    fb = smh.FrameBatch(vision, W, H, N)
    try:
        fb.run(frames.data_ptr(), N, stages=0x3, grayscale=False)
        with pytest.raises(smh.VisionError) as ei:                     # before any render
            fb.video("render", _word("nv12", "709", False))
        assert ei.value.code == _lib.E_STATE
        rw, rh = fb.roi[2:]
        for k, (ow, oh) in enumerate(((65, 33), (128, 64))):
            vp = smh.MapViewport.calc(ow, oh, rw, rh, k, (0.4, 0.6), (3.0, -2.0))
            fb.render(vp, ow, oh, markers=True, background=(10, 200, 90, 255))
            layout, (matrix, full) = ("nv12", "i420")[k], yo.ROWS[k + 1]
            got = fb.video("render", _word(layout, matrix, full)).cpu().numpy()
            imgs = [fb.read_render(f) for f in range(N)]
            assert imgs[0].shape == (oh, ow, 4) and len({i.tobytes() for i in imgs}) > 1
            assert got.shape == (N, yo.tight_bytes(ow, oh)) and np.array_equal(got, _tight(imgs, layout, matrix, full)), (ow, oh)
            part = fb.video("render", _word(layout, matrix, full), first=1, n=2).cpu().numpy()
            assert np.array_equal(part, got[1:3])
    finally:
        fb.close()


# ---- 6. a pipeline slot ----------------------------------------------------------------------------------------------------------

def test_pipeline_slot_after_wait_gives_the_plain_batch_bytes(vision, frames):
    import squad_mortar_helper_amd as smh
    word = _word("nv12", "709", False)
    fb = smh.FrameBatch(vision, W, H, N)
    p = smh.Pipeline(vision, W, H, N, depth=2)
    try:
        for gray in (False, True):
            fb.run(frames.data_ptr(), N, stages=0x3, grayscale=gray)
            smh.results_to_dicts(fb.read_results(0, N))
            plain = fb.video("ui_map", word).cpu().numpy()
            slot = p.submit(frames.data_ptr(), N, stages=0x3, grayscale=gray)
            p.wait(slot)
            sb = p.slots[slot]
            state = sb.ui_state()
            got = sb.video("ui_map", word).cpu().numpy()
            assert sb.ui_state() == state
            assert plain.any() and np.array_equal(got[[i for i in range(N) if i != CLOSED]], plain[[i for i in range(N) if i != CLOSED]]), gray
            assert np.array_equal(got, _tight([sb.read_image(smh._lib.IMAGE_UI_MAP, f) for f in range(N)], "nv12", "709", False)), gray
    finally:
        p.close()
        fb.close()
