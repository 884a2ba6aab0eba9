"""The scale-bar scan on the host: the oracle's find_scale_width / calc_meters_to_px_ratio against the sequential restatement
of mpx_ratio.rs (tests/scale_ref.py) on every case of tests/scale_cases.py, the fixed list's None / found pattern as worked
out by hand, and the case frames' way back to their scales images.  The GPU tests (test_scale_gpu.py) compare the device
with the oracle on the same cases."""
import numpy as np
import pytest

import scale_cases as S
import scale_ref as R


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


def _same(o, img, rows, anchor, ctx):
    """oracle == restatement for one anchor: ratio with ==, and the bar."""
    m, x, y = anchor
    got, want = o.find_scale_width(m, x, y, img), R.find_scale_width(m, x, y, rows)
    if want is None:
        assert got is None, (ctx, got)
    else:
        assert got is not None, (ctx, want)
        ratio, dbg = got[0], tuple(int(v) for v in got[1])
        assert ratio == want[0] and dbg == (want[1][0], want[1][1], want[1][2], want[1][1]), (ctx, got, want)
    return want


def _same_ladder(o, img, rows, anchors, ctx):
    got, (want, _) = o.calc_meters_to_px_ratio(anchors, img), R.calc_meters_to_px_ratio(anchors, rows)
    assert got == want and (got is None) == (want is None), (ctx, got, want)
    return want


@pytest.mark.parametrize("size", [S.BIG, S.SMALL])
def test_fixed_cases_oracle_equals_restatement_and_the_hand_written_pattern(o, size):
    import squad_mortar_helper_amd as smh
    _, _, rw, rh = smh.map_bounds(*size)
    assert (rw // 2, rh // 2) == S.QUADRANT[size]
    assert R.max_scale_y_offset(S.QUADRANT[size][0]) == {S.BIG: 21, S.SMALL: 6}[size]
    cases = S.fixed_cases(size)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) and S.NONE_NAMES <= set(names)
    if size == S.BIG:
        assert len(cases) == 70 and len(names) - len(S.NONE_NAMES) == 58
    by_hand = 0
    for c in cases:
        want = _same(o, c["img"], c["img"].tolist(), c["anchor"], (size, c["name"]))
        assert (want is None) == (c["name"] in S.NONE_NAMES), (size, c["name"], want)
        assert _same_ladder(o, c["img"], c["img"].tolist(), [c["anchor"]], (size, c["name"])) == (want[0] if want else None)
        bar = S.expected_bar(size, c)
        if bar is not None:
            by_hand += 1
            width = (bar[2] - bar[0]) % (1 << 32)
            assert want is not None and want[1] == bar and want[0] == c["anchor"][0] / float(width), (size, c["name"], want, bar)
    assert by_hand >= len(cases) - len(S.NONE_NAMES) - 1      # (every success but anchor_column_black, whose bar depends on the size)
    wrap = next(c for c in cases if c["name"] == "anchor_on_two_wide_tick")
    assert o.find_scale_width(*wrap["anchor"], wrap["img"])[0] == wrap["anchor"][0] / 4294967295.0


def test_ladder_outcomes_and_the_order_of_the_sum(o):
    img, calls = S.ladder()
    rows = img.tolist()
    a, b, c = [m / float(w) for m, w in zip(S.LADDER_METERS, S.LADDER_WIDTHS)]
    # the guard that keeps the case sharp: the index-order mean is not the reversed-order one
    assert ((a + b) + c) / 3.0 == S.LADDER_MEAN
    assert ((c + b) + a) / 3.0 != S.LADDER_MEAN and ((a + c) + b) / 3.0 != S.LADDER_MEAN and ((b + c) + a) / 3.0 != S.LADDER_MEAN
    assert len(calls) == 12 and [len(x) for x in calls] == [3] * 8 + [2] * 4
    outcomes = set()
    for anchors in calls:
        single = [_same(o, img, rows, an, ("ladder", an)) for an in anchors]
        ok = tuple(s is not None for s in single)
        assert ok == tuple(an[2] != 3 for an in anchors)
        outcomes.add(ok)
        want = _same_ladder(o, img, rows, anchors, ("ladder", anchors))
        hits = [s[0] for s in single if s is not None]
        if len(hits) == 3:
            assert want == S.LADDER_MEAN
        elif len(hits) == 2:
            assert want == (hits[0] + hits[1]) / 2.0
        else:
            assert want == (hits[0] if hits else None)
    assert len(outcomes) == 12


def test_random_images_oracle_equals_restatement(o, capsys):
    images, stats = S.random_images()
    with capsys.disabled():
        print("\nscale-bar random set: %d of %d anchors succeed (share %.3f), %d distinct widths"
              % (stats["found"], stats["anchors"], stats["share"], stats["distinct_widths"]))
    assert 0.3 <= stats["share"] <= 0.7 and stats["distinct_widths"] >= 64
    found = 0
    for k, (img, anchors) in enumerate(images):
        rows = img.tolist()
        for j, an in enumerate(anchors):
            found += _same(o, img, rows, an, ("random", k, j)) is not None
        for j in range(0, len(anchors), 3):
            _same_ladder(o, img, rows, anchors[j:j + 3], ("random", k, j))
    assert found == stats["found"]


def test_case_frames_lead_back_to_their_scales_images(o):
    """crop_to_map + find_scales_preprocess(0) of every distinct case frame is the scales image the frame was built from."""
    todo = []
    for size in (S.BIG, S.SMALL):
        seen = set()
        for c in S.fixed_cases(size):
            if id(c["img"]) not in seen:
                seen.add(id(c["img"]))
                todo.append((size, c["img"], c["name"]))
    todo.append((S.BIG, S.ladder()[0], "ladder"))
    todo += [(S.BIG, img, "random %d" % k) for k, (img, _) in enumerate(S.random_images()[0])]
    for i, (size, img, name) in enumerate(todo):
        crop = o.crop_to_map(S.frame_of(img, size, i))
        assert crop is not None, name
        assert np.array_equal(o.find_scales_preprocess(crop["cropped_brq"], 0), img), (size, name)
