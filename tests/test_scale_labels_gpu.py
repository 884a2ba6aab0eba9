"""Scale labels on the device (csrc/smh_scalelabels.hip) against the pixel-based restatement (tests/scale_labels_ref.py), byte for
byte -- headers, labels and crops -- on every way the code is reached: smhv_batch_scale_labels on a plain batch and on a pipeline
slot's batch, smhv_scale_labels on the per-call path, and VisionState.process(label_reader=).  The frames are every synthetic
case of tests/scale_label_cases.py, the label strips of the reference's screenshots and the `full` fixtures, grouped by frame
size into one batch each, with a closed frame among the open ones.  The record's meters per pixel after a SMHV_STAGE_SCALES run
with the anchors derived from the device's labels is bit-equal to smhv_scale_labels_anchors' ratio."""
import numpy as np
import pytest

import fixtures as F
import scale_label_cases as SC
import scale_labels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def world(o):
    """{size: [dict(name, frame, want, texts)]}: want = the restatement of the frame (None: the map is closed), computed once;
    texts = what a reader types for the frame's labels, in order (the strips' and the screenshots' read by eye, "100m", "200m",
    ... on synthetic frames)."""
    groups = {}

    def add(name, size, frame, texts=None):
        want = R.of_frame(frame)
        if texts is None and want is not None:
            texts = ["%dm" % (100 * (k + 1)) for k in range(want["header"][0])]
        groups.setdefault(size, []).append(dict(name=name, frame=frame, want=want, texts=texts))

    for c in SC.cases():
        add(c["name"], c["size"], SC.frame_of(c["V"], c["size"]))
        if c["name"] == "nine_labels":
            add("closed", SC.SMALL, SC.closed_frame(SC.SMALL))          # a closed frame between open ones
    for stem, entry in sorted(SC.STRIPS.items()):
        add("strip_" + stem, SC.BIG, SC.strip_frame(stem), entry["texts"])
    for stem in F.FULL_STEMS:
        frame, entry, _ = F.load_fixture(stem)
        add("full_" + stem, (entry["W"], entry["H"]), frame, ["300m", "900m"] if "intersect" in stem else None)
    assert groups[SC.SMALL][-1]["name"] != "closed" and any(e["want"] is None for e in groups[SC.SMALL])
    return groups


def _label_tuple(lb):
    return (lb.left, lb.top, lb.right, lb.bottom, lb.bar_left, lb.bar_y, lb.bar_right, lb.width)


def _check(rec, cells, want, ctx):
    """One frame's record and cells (uint8 [>= n, 32, 128]) against the restatement."""
    if want is None:
        assert bytes(rec) == bytes(288), ctx
        return
    n = want["header"][0]
    assert (rec.n, rec.n_found, rec.n_words, rec.n_runs, rec.flags) == want["header"], (ctx, want["header"])
    assert tuple(rec.reserved) == (0, 0, 0), ctx
    for i in range(R.MAX_LABELS):
        assert _label_tuple(rec.label[i]) == (want["labels"][i] if i < n else (0,) * 8), (ctx, i, want["labels"])
    assert np.array_equal(cells[:n], want["crops"]), ctx


def _upload(entries):
    import torch
    d = torch.from_numpy(np.stack([e["frame"] for e in entries])).cuda()
    torch.cuda.synchronize()
    return d


def _sizes():
    return sorted({c["size"] for c in SC.cases()} | {(F.MANIFEST[s]["W"], F.MANIFEST[s]["H"]) for s in F.FULL_STEMS})


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "%dx%d" % s)
def test_plain_batch(vision, world, size):
    """The same batch object twice: the frames in reverse order, then in order (nothing of the first run is left in the second);
    then STAGE_ALL with the anchors the labels give: the records' meters per pixel are smhv_scale_labels_anchors' ratios."""
    import torch
    import squad_mortar_helper_amd as smh
    entries = world[size]
    n, s = len(entries), torch.cuda.current_stream().cuda_stream
    d = _upload(entries)
    rev = d.flip(0).contiguous()
    fb = smh.FrameBatch(vision, size[0], size[1], n)
    for frames, order, tag in ((rev, entries[::-1], "reversed"), (d, entries, "in order")):
        fb.run(frames.data_ptr(), n, stages=smh.STAGE_OCR, stream=s)
        fb.scale_labels(frames.data_ptr(), n, stream=s)
        recs, cells = fb.read_scale_labels(0, n)
        for i, e in enumerate(order):
            _check(recs[i], cells[i], e["want"], (size, tag, e["name"]))
    per_frame, ratios = [], []
    for i, e in enumerate(entries):
        labels = [recs[i].label[k] for k in range(recs[i].n)]
        meters = [int(t[:-1]) if t.endswith("m") else 0 for t in (e["texts"] or [])]
        an, ratio = smh.scale_labels_anchors(labels, meters)
        per_frame.append((an.scales_start_y, [tuple(an.scales[k]) for k in range(an.n)]))
        ratios.append(ratio)
    assert sum(r is not None for r in ratios) >= (0 if size == (1280, 1024) else 1)      # (the two screenshots of that size show no labels)
    fb.run(d.data_ptr(), n, stages=smh.STAGE_ALL, anchors=smh.make_anchors(per_frame), stream=s)
    for i, (r, e) in enumerate(zip(fb.read_results(0, n), entries)):
        assert r.map_open == (e["want"] is not None), e["name"]
        assert bool(r.has_mpx) == (ratios[i] is not None) and r.mpx == (ratios[i] or 0.0), (e["name"], r.mpx, ratios[i])
    # the family's pass has left the batch's own planes alone: the ocr plane a read returns is the oracle's
    from oracle import oracle as o
    k = max(range(n), key=lambda i: entries[i]["want"]["header"][0] if entries[i]["want"] is not None else -1)   # a frame with labels, where there is one
    P = o.ocr_preprocess(o.crop_to_map(entries[k]["frame"], True)["cropped_brq"])
    assert np.array_equal(fb.read_image(smh.DebugView.OCR_INPUT, k), P)
    scales = fb.read_image(smh.DebugView.FIND_SCALES_INPUT, k)
    fb.scale_labels(d.data_ptr(), n, stream=s)
    assert np.array_equal(fb.read_image(smh.DebugView.FIND_SCALES_INPUT, k), scales) and np.array_equal(fb.read_image(smh.DebugView.OCR_INPUT, k), P)
    _check(fb.read_scale_labels(k, 1)[0][0], fb.read_scale_labels(k, 1)[1][0], entries[k]["want"], (size, "after STAGE_ALL"))
    fb.close()
    del d, rev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "%dx%d" % s)
def test_pipeline_slot(vision, world, size):
    """A pipeline slot's batch after smhv_pipeline_wait, on the slot's stream."""
    import torch
    import squad_mortar_helper_amd as smh
    entries = world[size]
    n = len(entries)
    d = _upload(entries)
    p = smh.Pipeline(vision, size[0], size[1], n, depth=2)
    for _ in range(2):
        slot = p.submit(d.data_ptr(), n, stages=smh.STAGE_ALL)
        p.wait(slot)
        fb = p.slots[slot]
        fb.scale_labels(d.data_ptr(), n, stream=p.stream_of(slot))
        recs, cells = fb.read_scale_labels(0, n)
        for i, e in enumerate(entries):
            _check(recs[i], cells[i], e["want"], (size, "slot", slot, e["name"]))
    p.close()
    del d
    torch.cuda.empty_cache()


def test_state_errors(vision, world):
    import torch
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    entries = world[SC.SMALL][:3]
    d = _upload(entries)
    fb = smh.FrameBatch(vision, SC.SMALL[0], SC.SMALL[1], 3)
    with pytest.raises(smh.VisionError) as ei:
        fb.read_scale_labels(0, 1)
    assert ei.value.code == L.E_STATE
    with pytest.raises(smh.VisionError) as ei:                      # no run at all
        fb.scale_labels(d.data_ptr(), 3)
    assert ei.value.code == L.E_STATE
    fb.run(d.data_ptr(), 3, stages=smh.STAGE_UI_MAP | smh.STAGE_MARKERS)
    with pytest.raises(smh.VisionError) as ei:                      # the last run had no STAGE_OCR
        fb.scale_labels(d.data_ptr(), 3)
    assert ei.value.code == L.E_STATE
    fb.run(d.data_ptr(), 2, stages=smh.STAGE_OCR)
    with pytest.raises(smh.VisionError) as ei:                      # ... or covered fewer frames
        fb.scale_labels(d.data_ptr(), 3)
    assert ei.value.code == L.E_STATE
    for bad in ((0, 1), (d.data_ptr() + 1, 1), (d.data_ptr(), 0), (d.data_ptr(), 4)):
        with pytest.raises(smh.VisionError) as ei:
            fb.scale_labels(*bad)
        assert ei.value.code == L.E_INVALID
    fb.scale_labels(d.data_ptr(), 2)
    recs, cells = fb.read_scale_labels(0, 2)
    for i in range(2):
        _check(recs[i], cells[i], entries[i]["want"], ("after errors", i))
    assert all(v != 0 for v in fb.scale_labels_ptr())
    fb.close()
    vision.load_frame(entries[0]["frame"])
    assert vision.crop_to_map() is not None
    with pytest.raises(smh.VisionError) as ei:                      # per call: before ocr_preprocess
        vision.scale_labels()
    assert ei.value.code == L.E_STATE
    del d
    torch.cuda.empty_cache()


def test_per_call(vision, world):
    """smhv_scale_labels after load_frame / crop_to_map / ocr_preprocess, every frame in turn on one context."""
    for size, entries in sorted(world.items()):
        for e in entries:
            vision.load_frame(e["frame"])
            if vision.crop_to_map() is None:
                assert e["want"] is None, e["name"]
                continue
            assert e["want"] is not None, e["name"]
            vision.ocr_preprocess()
            rec, cells = vision.scale_labels()
            assert len(cells) == rec.n
            _check(rec, cells, e["want"], (size, "per call", e["name"]))
            rec2, none = vision.scale_labels(crops=False)
            assert none is None and bytes(rec2) == bytes(rec)


def test_process_with_a_label_reader(vision, world, o):
    """VisionState.process(label_reader=): the reader is shown the restatement's crops and boxes, and what it types goes through
    parse_ocr_labels, find_scales_preprocess and calc_meters_to_px_ratio: the oracle's meters per pixel on the same anchors."""
    import squad_mortar_helper_amd as smh
    st = smh.VisionState()
    some = 0
    for size, entries in sorted(world.items()):
        for e in entries:
            seen = []

            def reader(crop, box, e=e, seen=seen):
                seen.append((crop.copy(), tuple(int(v) for v in box)))
                return e["texts"][len(seen) - 1]
            res = st.process(vision, e["frame"], label_reader=reader)
            if e["want"] is None:
                assert res is None and not seen, e["name"]
                continue
            want = e["want"]
            assert [b for _, b in seen] == [p[:4] for p in want["labels"]], e["name"]
            assert all(np.array_equal(c, w) for (c, _), w in zip(seen, want["crops"])), e["name"]
            hits = [dict(text=t, left=p[0], top=p[1], right=p[2], bottom=p[3]) for p, t in zip(want["labels"], e["texts"])]
            scales, start_y = smh.parse_ocr_labels(hits)
            mpx = None
            if scales:
                brq = o.crop_to_map(e["frame"], True)["cropped_brq"]
                mpx = o.calc_meters_to_px_ratio(scales, o.find_scales_preprocess(brq, start_y))
            assert res.meters_to_px_ratio == mpx and (res.meters_to_px_ratio is None) == (mpx is None), (e["name"], res.meters_to_px_ratio, mpx)
            some += mpx is not None
    st.close()
    assert some >= 20
