"""Scale labels: text on the device (csrc/smh_labeltext.hip) against the restatement (tests/label_text_ref.py), every byte of every
record, on every way the code is reached: smhv_label_text per call, smhv_batch_label_text on a plain batch (cases mixed with a
closed frame, n below the batch's capacity) and on a pipeline slot's batch after wait, and VisionState.process(label_reader=atlas).
mpx is compared == with smhv_scale_labels_anchors on the host, given the meters the device read; smhv_batch_run_label_anchors
leaves the records smhv_batch_run leaves when the host hands it the same anchors; every error return enqueues nothing."""
import ctypes as C

import numpy as np
import pytest

import label_text_cases as LC
import label_text_ref as LT
import scale_label_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(built):
    """{size: [dict(case, frame, want)]}: every case's frame and its scale-label restatement, computed once; a closed frame second in
    every group."""
    groups = {}
    for c in LC.cases():
        groups.setdefault(c["size"], []).append(dict(case=c, frame=LC.frame_of(c), want=LC.want_of(c)))
    for size, entries in groups.items():
        entries.insert(1, dict(case=None, frame=SC.closed_frame(size), want=None))
    return groups


@pytest.fixture(scope="module")
def atlases(vision):
    """The device atlas of a restatement atlas, made once each."""
    import squad_mortar_helper_amd as smh
    made = {}

    def get(atlas):
        if id(atlas) not in made:
            made[id(atlas)] = (atlas, smh.GlyphAtlas.from_templates(vision, LC.lib_templates(atlas), atlas.num, atlas.den))
        return made[id(atlas)][1]
    yield get
    for _, a in made.values():
        a.close()


def _check(rec, sl_rec, want, atlas, ctx):
    """One frame's text record against the restatement under `atlas`; sl_rec: the device's own scale labels of the frame."""
    import squad_mortar_helper_amd as smh
    fr = LT.read_frame(want, atlas)
    assert bytes(rec) == LT.pack_frame(fr), (ctx, fr)
    labels = [sl_rec.label[i] for i in range(sl_rec.n)]
    an, mpx = smh.scale_labels_anchors(labels, [rec.label[i].meters for i in range(rec.n)])
    assert rec.n == sl_rec.n and bool(rec.has) == (mpx is not None) and rec.mpx == (mpx or 0.0), ctx
    assert bytes(rec.anchors) == bytes(an), ctx
    return fr


def _d2h(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0            # hipMemcpyDeviceToHost
    return out


def _upload(entries):
    import torch
    d = torch.from_numpy(np.stack([e["frame"] for e in entries])).cuda()
    torch.cuda.synchronize()
    return d


def _group_atlases(entries):
    seen, out = set(), []
    for e in entries:
        if e["case"] is not None and id(e["case"]["atlas"]) not in seen:
            seen.add(id(e["case"]["atlas"]))
            out.append(e["case"]["atlas"])
    return out


@pytest.mark.parametrize("size", LC.SIZES, ids=lambda s: "%dx%d" % s)
def test_plain_batch(vision, world, atlases, size):
    """One batch of capacity n + 2 run over n frames; the texts under every atlas of the group in turn: a case's record is checked
    under its own atlas, the closed frame and the frames without labels under every one, and every frame under the first."""
    import torch
    import squad_mortar_helper_amd as smh
    entries = world[size]
    n, s = len(entries), torch.cuda.current_stream().cuda_stream
    d = _upload(entries)
    fb = smh.FrameBatch(vision, size[0], size[1], n + 2)
    fb.run(d.data_ptr(), n, stages=smh.STAGE_OCR, stream=s)
    fb.scale_labels(d.data_ptr(), n, stream=s)
    sl, _ = fb.read_scale_labels(0, n, crops=False)
    for k, atlas in enumerate(_group_atlases(entries)):
        fb.label_text(atlases(atlas), n, stream=s)
        recs = fb.read_label_text(0, n)
        for i, e in enumerate(entries):
            own = e["case"] is not None and e["case"]["atlas"] is atlas
            if own or k == 0 or e["want"] is None or e["want"]["header"][0] == 0:
                fr = _check(recs[i], sl[i], e["want"], atlas, (size, k, e["case"]["name"] if e["case"] else "closed"))
                if own:
                    LC.check_expect(e["case"], fr)
    d_text, d_anchors = fb.label_text_ptr()
    assert d_text and d_anchors
    tight = _d2h(d_anchors, 44 * n)                                  # the anchors, tightly packed: the records' own (the last atlas')
    assert tight.tobytes() == b"".join(bytes(r.anchors) for r in recs)
    assert _d2h(d_text, LT.REC_BYTES * n).tobytes() == bytes(recs)
    fb.close()
    del d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("size", (LC.SIZES[0], LC.SIZES[2]), ids=lambda s: "%dx%d" % s)
def test_pipeline_slot(vision, world, atlases, size):
    """A pipeline slot's batch after smhv_pipeline_wait, on the slot's stream, under the group's first atlas."""
    import torch
    import squad_mortar_helper_amd as smh
    entries = world[size]
    n = len(entries)
    atlas = _group_atlases(entries)[0]
    d = _upload(entries)
    p = smh.Pipeline(vision, size[0], size[1], n, depth=2)
    for _ in range(2):
        slot = p.submit(d.data_ptr(), n, stages=smh.STAGE_ALL)
        p.wait(slot)
        fb = p.slots[slot]
        fb.scale_labels(d.data_ptr(), n, stream=p.stream_of(slot))
        fb.label_text(atlases(atlas), n, stream=p.stream_of(slot))
        sl, _ = fb.read_scale_labels(0, n, crops=False)
        recs = fb.read_label_text(0, n)
        for i, e in enumerate(entries):
            _check(recs[i], sl[i], e["want"], atlas, (size, "slot", slot, i))
    p.close()
    del d
    torch.cuda.empty_cache()


def test_per_call(vision, world, atlases):
    """smhv_label_text after load_frame / crop_to_map / ocr_preprocess / scale_labels, every case in turn on one context."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    for size, entries in sorted(world.items()):
        for e in entries:
            vision.load_frame(e["frame"])
            if vision.crop_to_map() is None:
                assert e["want"] is None
                continue
            atlas = e["case"]["atlas"]
            vision.ocr_preprocess()
            with pytest.raises(smh.VisionError) as ei:              # the labels of this frame have not been found yet
                vision.label_text(atlases(atlas))
            assert ei.value.code == L.E_STATE
            sl, _ = vision.scale_labels(crops=False)
            rec = vision.label_text(atlases(atlas))
            LC.check_expect(e["case"], _check(rec, sl, e["want"], atlas, (size, "per call", e["case"]["name"])))


def test_process_with_an_atlas_as_the_reader(vision, world, atlases):
    """VisionState.process(label_reader=GlyphAtlas): the device's texts go through parse_ocr_labels, find_scales_preprocess and
    calc_meters_to_px_ratio; every label taken has its bar, so the ratio is the text record's mpx."""
    import squad_mortar_helper_amd as smh
    st = smh.VisionState()
    some = 0
    for size, entries in sorted(world.items()):
        for e in entries:
            if e["case"] is not None and not e["case"]["name"].startswith(("frame_", "strip_", "parse_")):
                continue
            res = st.process(vision, e["frame"], label_reader=atlases(e["case"]["atlas"] if e["case"] else LC.FONT1))
            if e["want"] is None:
                assert res is None
                continue
            fr = LT.read_frame(e["want"], e["case"]["atlas"])
            assert res.meters_to_px_ratio == (fr["mpx"] if fr["has"] else None), (e["case"]["name"], res.meters_to_px_ratio, fr["mpx"])
            some += fr["has"]
    st.close()
    assert some >= 15


@pytest.mark.parametrize("size", LC.SIZES[1:], ids=lambda s: "%dx%d" % s)
def test_run_label_anchors_is_batch_run_with_the_same_anchors(vision, world, atlases, size):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    entries = world[size]
    n, s = len(entries), torch.cuda.current_stream().cuda_stream
    atlas = _group_atlases(entries)[0]
    d = _upload(entries)
    fb = smh.FrameBatch(vision, size[0], size[1], n)
    fb.run(d.data_ptr(), n, stages=smh.STAGE_OCR, stream=s)
    fb.scale_labels(d.data_ptr(), n, stream=s)
    fb.label_text(atlases(atlas), n, stream=s)
    fb.run_label_anchors(d.data_ptr(), n, stages=smh.STAGE_ALL, stream=s)
    on_device = bytes(fb.read_results(0, n))
    recs = fb.read_label_text(0, n)
    res = fb.read_results(0, n)
    for i in range(n):
        assert bool(res[i].has_mpx) == bool(recs[i].has) and res[i].mpx == recs[i].mpx, (size, i, res[i].mpx, recs[i].mpx)
    assert sum(r.has for r in recs) >= 3
    anchors = (L.Anchors * n)()
    for i in range(n):
        C.memmove(C.addressof(anchors[i]), C.addressof(recs[i].anchors), C.sizeof(L.Anchors))
    fb.run(d.data_ptr(), n, stages=smh.STAGE_ALL, anchors=anchors, stream=s)
    assert bytes(fb.read_results(0, n)) == on_device
    fb.close()
    del d
    torch.cuda.empty_cache()


def test_error_returns_enqueue_nothing(vision, world, atlases):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    lib = L.load()
    entries = world[SC.SMALL][:4]
    size = SC.SMALL
    d = _upload(entries)
    atlas = atlases(LC.FONT1)

    def refused(code, fn, *args, **kw):
        with pytest.raises(smh.VisionError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, (fn, args)

    fb = smh.FrameBatch(vision, size[0], size[1], 4)
    refused(L.E_STATE, fb.read_label_text, 0, 1)
    refused(L.E_STATE, fb.label_text_ptr)
    refused(L.E_STATE, fb.label_text, atlas, 4)                      # no scale labels at all
    refused(L.E_STATE, fb.run_label_anchors, d.data_ptr(), 4)        # no label text at all
    fb.run(d.data_ptr(), 4, stages=smh.STAGE_OCR)
    fb.scale_labels(d.data_ptr(), 3)
    refused(L.E_STATE, fb.label_text, atlas, 4)                      # ... or over fewer frames
    fb.label_text(atlas, 3)
    before = bytes(fb.read_label_text(0, 4))
    assert before[3 * LT.REC_BYTES:] == bytes(LT.REC_BYTES)          # (the fourth frame's record: as the slab was made)
    results = bytes(fb.read_results(0, 4))
    refused(L.E_INVALID, fb.label_text, atlas, 0)
    refused(L.E_INVALID, fb.label_text, atlas, 5)
    with pytest.raises(smh.VisionError) as ei:
        L.check(lib.smhv_batch_label_text(fb._b, None, 3, None))     # a null atlas
    assert ei.value.code == L.E_INVALID
    refused(L.E_STATE, fb.label_text, atlas, 4)
    refused(L.E_STATE, fb.run_label_anchors, d.data_ptr(), 4)        # the texts cover three frames
    refused(L.E_INVALID, fb.run_label_anchors, d.data_ptr(), 0)
    refused(L.E_INVALID, fb.run_label_anchors, d.data_ptr(), 5)
    refused(L.E_INVALID, fb.run_label_anchors, 0, 3)
    refused(L.E_INVALID, fb.run_label_anchors, d.data_ptr() + 1, 3)
    refused(L.E_INVALID, fb.run_label_anchors, d.data_ptr(), 3, stages=0)
    refused(L.E_INVALID, fb.read_label_text, 3, 2)
    assert bytes(fb.read_label_text(0, 4)) == before and bytes(fb.read_results(0, 4)) == results
    sl, _ = fb.read_scale_labels(0, 3, crops=False)
    recs = fb.read_label_text(0, 3)
    for i in range(3):
        _check(recs[i], sl[i], entries[i]["want"], LC.FONT1, ("after errors", i))
    fb.close()
    # the atlas itself
    good = LC.lib_templates(LC.FONT1)
    bad = L.GlyphTemplate()
    C.memmove(C.addressof(bad), C.addressof(good[0]), C.sizeof(bad))
    bad.rows[0] = 0
    refused(L.E_INVALID, smh.GlyphAtlas.from_templates, vision, [])
    refused(L.E_INVALID, smh.GlyphAtlas.from_templates, vision, good * 3)
    refused(L.E_INVALID, smh.GlyphAtlas.from_templates, vision, good[:2] + [bad])
    refused(L.E_INVALID, smh.GlyphAtlas.from_templates, vision, good, accept_den=0)
    # per call: before scale_labels on this frame, and after the next frame's ocr_preprocess
    vision.load_frame(entries[0]["frame"])
    assert vision.crop_to_map() is not None
    refused(L.E_STATE, vision.label_text, atlas)
    vision.ocr_preprocess()
    refused(L.E_STATE, vision.label_text, atlas)
    vision.scale_labels(crops=False)
    vision.label_text(atlas)
    vision.ocr_preprocess()
    refused(L.E_STATE, vision.label_text, atlas)
    del d
    torch.cuda.empty_cache()


def test_an_atlas_learned_through_the_library(vision, world):
    """GlyphAtlas.from_labels on what a reader saw of glorious.png reads the other strips (the learning helper end to end)."""
    import squad_mortar_helper_amd as smh
    by = {e["case"]["name"]: e for e in world[SC.BIG] if e["case"] is not None}
    src = by["strip_glorious_by_albasrah_png"]
    seen = []
    vision.load_frame(src["frame"])
    assert vision.crop_to_map() is not None
    vision.ocr_preprocess()
    rec, cells = vision.scale_labels()
    for i, text in enumerate(SC.STRIPS["glorious_png"]["texts"]):
        seen.append((cells[i], rec.label[i], text))
    atlas = smh.GlyphAtlas.from_labels(vision, seen)
    assert sorted(set(atlas.codes)) == ["0", "1", "3", "9", "m"]
    for stem in ("albasrah_png", "difficult_png", "in_mortar_png"):
        e = by["strip_%s_by_glorious" % stem]
        vision.load_frame(e["frame"])
        assert vision.crop_to_map() is not None
        vision.ocr_preprocess()
        sl, _ = vision.scale_labels(crops=False)
        got = vision.label_text(atlas)
        assert [smh.entry_text(got.label[i]) for i in range(got.n)] == e["case"]["expect"]["texts"], stem
        assert bytes(got) == LT.pack_frame(LT.read_frame(e["want"], e["case"]["atlas"])), stem
    atlas.close()
