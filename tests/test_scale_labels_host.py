"""Scale labels without a GPU: the structs' layout against a C program compiled from the header, the restatement
(tests/scale_labels_ref.py) against boxes and bars found on the reference's screenshots, on the strips cut from them and on every
synthetic case's own expectation (tests/scale_label_cases.py), and the host function smhv_scale_labels_anchors against
parse_ocr_labels and the oracle's calc_meters_to_px_ratio."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fixtures as F
import scale_label_cases as SC
import scale_labels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# box / bar (left, y, right) on the whole screenshot
FULL_IMAGE = {
    "point_intersect_png": [((576, 421, 612, 432), (537, 443, 615)), ((576, 452, 612, 463), (378, 474, 615))],
    "points_intersect_png": [((577, 421, 612, 432), (539, 443, 615)), ((577, 452, 612, 463), (381, 474, 615))],
}
GLORIOUS = [((578, 390, 612, 401), (555, 411, 615)), ((577, 421, 612, 432), (429, 443, 615)), ((577, 453, 612, 463), (54, 474, 615))]
MPX = {"point_intersect_png": 3.8218111002921127, "points_intersect_png": 3.896761133603239}


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


def test_struct_layouts_and_constants_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    lab = ["left", "top", "right", "bottom", "bar_left", "bar_y", "bar_right", "width"]
    fr = ["n", "n_found", "n_words", "n_runs", "flags", "reserved", "label"]
    body = "".join('  O(smhv_scale_label, %s);\n' % f for f in lab) + "".join('  O(smhv_scale_label_frame, %s);\n' % f for f in fr)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   '#define Z(t) printf(#t " %zu\\n", sizeof(t))\n'
                   'int main(void) {\n  Z(smhv_scale_label); Z(smhv_scale_label_frame);\n' + body +
                   '  printf("consts %u %u %u %u %u %u %u\\n", SMHV_MAX_SCALE_LABELS, SMHV_LABEL_MAX_RUNS, SMHV_LABEL_CROP_W, SMHV_LABEL_CROP_H,\n'
                   '         SMHV_LABELS_RUNS_OVERFLOW, SMHV_LABEL_CROP_BYTES, SMHV_LABEL_FRAME_CROP_BYTES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("consts") else ("consts", ln[7:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["smhv_scale_label"]) == 32 == C.sizeof(L.ScaleLabel)
    assert int(got["smhv_scale_label_frame"]) == 288 == C.sizeof(L.ScaleLabelFrame)
    for f in lab:
        assert int(got["smhv_scale_label." + f]) == getattr(L.ScaleLabel, f).offset, f
    for f in fr:
        assert int(got["smhv_scale_label_frame." + f]) == getattr(L.ScaleLabelFrame, f).offset, f
    assert got["consts"].split() == [str(v) for v in (L.MAX_SCALE_LABELS, L.LABEL_MAX_RUNS, L.LABEL_CROP_W, L.LABEL_CROP_H, L.LABELS_RUNS_OVERFLOW, 4096, 32768)]
    assert (R.MAX_LABELS, R.MAX_RUNS, R.CROP_W, R.CROP_H, R.RUNS_OVERFLOW) == (L.MAX_SCALE_LABELS, L.LABEL_MAX_RUNS, L.LABEL_CROP_W, L.LABEL_CROP_H, L.LABELS_RUNS_OVERFLOW)


def test_gap_of_the_pinned_widths():
    assert [R.gap(w) for w in (180, 197, 357, 657, 1314)] == [1, 1, 2, 4, 8]
    assert R.gap(1) == 1 and R.gap(240) == 2 and R.gap(239) == 1      # 1.5 rounds away from zero
    assert [SC.geometry(s)[4:6] for s in (SC.SMALL, SC.MID, SC.BIG, SC.HUGE)] == [(180, 292), (357, 389), (657, 548), (1314, 1096)]


def test_smear_is_the_gap_rule_pixel_by_pixel():
    """smear against the rule spelled out on one row at a time: the pixels between two neighbouring foreground pixels are filled
    when there are at most g of them."""
    rng = np.random.default_rng(5)
    for g in (1, 2, 4, 8):
        fg = rng.random((40, 97)) < 0.2
        fg[0] = False
        fg[1, [0, 96]] = True
        want = fg.copy()
        for y in range(fg.shape[0]):
            xs = np.flatnonzero(fg[y])
            for a, b in zip(xs[:-1], xs[1:]):
                if b - a - 1 <= g:
                    want[y, a:b] = True
        assert np.array_equal(R.smear(fg, g), want), g


@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c["name"])
def test_cases_say_what_they_are_for(o, case):
    """Every synthetic case's expectation, worked by hand, holds on the restatement of its frame."""
    f = SC.frame_of(case["V"], case["size"])
    res = R.of_frame(f)
    assert res is not None
    n, n_found, n_words, n_runs, flags = res["header"]
    e = case["expect"]
    assert n_found == e["n_found"] and n == min(n_found, R.MAX_LABELS), res["header"]
    assert n_words == e["n_words"], res["header"]
    assert flags == e.get("flags", 0)
    if "n_runs" in e:
        assert n_runs == e["n_runs"], res["header"]
    if "boxes" in e:
        assert [p[:4] for p in res["all"]] == [tuple(b) for b in e["boxes"]], res["all"]
    assert res["crops"].shape == (n, R.CROP_H, R.CROP_W)
    P = o.ocr_preprocess(o.crop_to_map(f, True)["cropped_brq"])
    for (l, t, r, b, bl, by, br, wd), cell in zip(res["labels"], res["crops"]):
        assert br > bl and wd == br - bl >= 10 and b <= by
        assert np.array_equal(cell[:b - t, :r - l], P[t:b, l:r]) and (cell[b - t:] == 255).all() and (cell[:, r - l:] == 255).all()
        assert (cell[:b - t, :r - l] != 255).any()


def test_closed_frame_is_closed(o):
    assert R.of_frame(SC.closed_frame(SC.SMALL)) is None


@pytest.mark.parametrize("stem", F.FULL_STEMS)
def test_full_fixtures(o, stem):
    """The two screenshots with scale labels give exactly their two labels with the bars the reference finds from the hand-read
    anchors; the "Training" box of the legend has a dark block under it, whose bar wraps: excluded.  The other six give none."""
    frame, entry, _ = F.load_fixture(stem)
    res = R.of_frame(frame)
    want = FULL_IMAGE.get(stem, [])
    assert [(p[:4], p[4:7]) for p in res["all"]] == want, res["all"]
    assert res["header"][:2] == (len(want), len(want)) and res["header"][4] == 0
    if want:
        brq = o.crop_to_map(frame, True)["cropped_brq"]
        P, S0 = o.ocr_preprocess(brq), o.find_scales_preprocess(brq, 0)
        boxes = R.components(R.smear(P != 255, R.gap(P.shape[1])))
        if stem == "point_intersect_png":
            training = (504, 492, 564, 508)
            assert training in boxes
            bar = o.find_scale_width(1, (training[0] + training[2]) // 2, training[3], S0)
            assert bar is not None and bar[1][2] < bar[1][0]
        # the bars are the ones the manifest's hand-read anchors find (those sit in the same column, a row lower)
        for (box, b), a, per in zip(want, entry["anchors"], entry["per_anchor"]):
            assert tuple(per["bar"][:3]) == b and a[1] == (box[0] + box[2]) // 2 and 0 <= a[2] - box[3] <= 2


@pytest.mark.parametrize("stem", sorted(SC.STRIPS))
def test_strips_keep_the_screenshots_proposals(o, stem):
    """A strip pasted into a frame of the tests' own gives the proposals of the whole screenshot (recorded by make_label_strips.py)."""
    res = R.of_frame(SC.strip_frame(stem))
    want = [tuple(p) for p in SC.STRIPS[stem]["proposals"]]
    assert [p[:7] for p in res["all"]] == want
    assert len(SC.STRIPS[stem]["texts"]) == len(want) == res["header"][0]
    if stem == "glorious_png":
        assert [(p[:4], p[4:7]) for p in res["all"]] == GLORIOUS


def _hits_of(smh, L, res, texts):
    labels = [L.ScaleLabel(*p) for p in res["labels"]]
    return labels, smh.scale_label_hits(labels, texts)


@pytest.mark.parametrize("stem", sorted(FULL_IMAGE))
def test_end_to_end_meters_per_pixel(o, stem):
    """"300m" and "900m", typed in, through scale_label_hits, parse_ocr_labels and the oracle's calc_meters_to_px_ratio: the
    manifest's meters per pixel, exactly; smhv_scale_labels_anchors gives the same double and the same anchors."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    frame, entry, _ = F.load_fixture(stem)
    res = R.of_frame(frame)
    labels, hits = _hits_of(smh, L, res, ["300m", "900m"])
    scales, start_y = smh.parse_ocr_labels(hits)
    assert [s[0] for s in scales] == [300, 900] and [s[1:] for s in scales] == [((p[0] + p[2]) // 2, p[3]) for p in res["labels"]]
    assert start_y == res["labels"][0][3]
    brq = o.crop_to_map(frame, True)["cropped_brq"]
    mpx = o.calc_meters_to_px_ratio(scales, o.find_scales_preprocess(brq, start_y))
    assert mpx == MPX[stem]
    an, ratio = smh.scale_labels_anchors(labels, [300, 900])
    assert ratio == MPX[stem]
    assert (an.n, an.scales_start_y) == (2, start_y) and [tuple(an.scales[i]) for i in range(2)] == scales


def test_strip_texts_give_plausible_ratios(o):
    """The texts read by eye off the strips, through the same path: every strip's labels agree on the meters per pixel within 4 %
    (they are bars of one map at one zoom), and what is no label ("8", ")") is dropped by parse_ocr_labels."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    for stem, entry in sorted(SC.STRIPS.items()):
        frame = SC.strip_frame(stem)
        res = R.of_frame(frame)
        labels, hits = _hits_of(smh, L, res, entry["texts"])
        scales, start_y = smh.parse_ocr_labels(hits)
        assert [m for m, _, _ in scales] == [int(t[:-1]) for t in entry["texts"] if t.endswith("m")], stem
        brq = o.crop_to_map(frame, True)["cropped_brq"]
        mpx = o.calc_meters_to_px_ratio(scales, o.find_scales_preprocess(brq, start_y))
        meters = [int(t[:-1]) if t.endswith("m") else 0 for t in entry["texts"]]
        an, ratio = smh.scale_labels_anchors(labels, meters)
        assert ratio == mpx and an.scales_start_y == start_y, stem
        each = [m / float(lb.width) for m, lb in zip(meters, labels) if m]
        assert max(each) / min(each) < 1.04, (stem, each)


def test_anchors_follow_the_reference_filter(built):
    """smhv_scale_labels_anchors against parse_ocr_labels on random label lists: zeros skipped, duplicates dropped but counted for
    scales_start_y, nothing looked at after the third distinct value, the ladder's mean summed in order."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(0, 9))
        labels, meters = [], []
        for i in range(n):
            l, t = int(rng.integers(0, 500)), int(rng.integers(0, 400))
            bl = int(rng.integers(0, 300))
            wd = int(rng.integers(10, 300))
            labels.append(L.ScaleLabel(l, t, l + int(rng.integers(3, 129)), t + int(rng.integers(3, 33)), bl, t + 40, bl + wd, wd))
            meters.append(int(rng.choice([0, 0, 100, 300, 900, 1200])))
        hits = smh.scale_label_hits(labels, ["%dm" % m if m else "x" for m in meters])
        scales, start_y = smh.parse_ocr_labels(hits)
        an, ratio = smh.scale_labels_anchors(labels, meters)
        assert an.n == len(scales) and [tuple(an.scales[i]) for i in range(an.n)] == scales, trial
        assert an.scales_start_y == (start_y if scales else 0)
        if not scales:
            assert ratio is None
            continue
        by_m = {}
        for lb, m in zip(labels, meters):
            by_m.setdefault(m, lb)
        r = [m / float(by_m[m].width) for m, _, _ in scales]
        want = r[0] if len(r) == 1 else ((r[0] + r[1]) / 2.0 if len(r) == 2 else (r[0] + r[1] + r[2]) / 3.0)
        assert ratio == want, trial
    with pytest.raises(smh.VisionError):
        smh.scale_labels_anchors([L.ScaleLabel(0, 0, 10, 10, 50, 12, 40, 0)], [100])      # a record without a bar


def test_prims_are_the_ocr_overlays(built):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib as L
    labels = [L.ScaleLabel(576, 421, 612, 432, 537, 443, 615, 78)]
    a = smh.scale_label_prims(labels, 657, 548)
    b = smh.ocr_box_prims([(576, 421, 612, 432, 100.0)], 657, 548)
    assert len(a) == 1 and a == b and a[0][:4] == (576.0 + 657, 421.0 + 548, 612.0 + 657, 432.0 + 548)
