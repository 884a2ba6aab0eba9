"""The search service's sampler of a ray's first batches (csrc/smh_lsd.hip, win2_issue), on the CPU: the bit-address identity it
rests on, and the expectations of the cases of tests/sampler_cases.py on the oracle (what tests/test_sampler_gpu.py runs on the
device is what it says it is)."""
import numpy as np

import sampler_cases as S
from oracle import oracle as o

PITCH_WORDS = 6           # LSD_W2_PITCH: a window row is 6 words = 192 bits


def test_bit_address_identity():
    """ba = yi * 192 + xi: the word is (ba >> 5) words from the window's origin and the bit is ba & 31 -- what win2_raw computes as
    yi * 24 + ((xi >> 3) & ~3) bytes and xi & 31 -- for every row and column a window can see, negative ones included."""
    yi = np.arange(-80, 2201, dtype=np.int64)[:, None]
    xi = np.arange(-80, 4201, dtype=np.int64)[None, :]
    ba = yi * (32 * PITCH_WORDS) + xi
    assert np.array_equal((ba >> 5) << 2, yi * (4 * PITCH_WORDS) + ((xi >> 3) & ~3))
    assert np.array_equal(ba & 31, np.broadcast_to(xi & 31, ba.shape))
    assert np.abs(ba).max() < 1 << 23                       # v_mad_i32_i24 takes it
    # ... and it is the pitch being whole words that makes it one: a pitch of 190 bits breaks both halves
    bad = yi * 190 + xi
    assert not np.array_equal(bad & 31, np.broadcast_to(xi & 31, bad.shape))


def test_cases_are_what_they_say():
    ref = S.reference()
    assert [c.name for c in S.cases()] == ["edges", "corners", "half", "steps", "window"] + ["gap_%d" % T for T in S.GAPS]
    assert sorted(g for g, _ in S.groups()) == sorted(set(S.GAPS))
    for R in ref.values():
        assert R.rounds > 0 and R.n_mask_px > 0 and R.mask.shape == (S.RH, S.RW), R.case.name

    # edges / corners: white within 4 px of every edge and corner, and a line found from there
    m = ref["edges"].mask == 255
    assert m[:4].any() and m[-4:].any() and m[:, :4].any() and m[:, -4:].any() and len(ref["edges"].lines) >= 4
    m = ref["corners"].mask == 255
    assert m[:4, :4].any() and m[:4, -4:].any() and m[-4:, :4].any() and m[-4:, -4:].any() and len(ref["corners"].lines) >= 4
    # a candidate d <= 4 px from an edge: its ray at angle t to the edge's normal leaves at step ~ d / cos t -- there are rays
    # among the 3600 that leave inside the first 8, 16, 32 and 64 steps and not inside the half of it
    t = np.deg2rad(np.arange(3600) * 0.1)
    leave = np.ceil(4.0 / np.maximum(np.cos(t), 1e-9))
    for k in (8, 16, 32, 64):
        assert ((leave > k // 2) & (leave <= k)).any(), k

    # half-integer start points
    starts = ref["half"].lines[:, :2]
    assert len(starts) >= 2 and (starts[:, 0] % 1 == 0.5).any() and (starts[:, 1] % 1 == 0.5).any(), starts

    # steps: down from the first candidate's centre (x, y0 + 1) white to step a - 1, black for 16 steps, white again
    R = ref["steps"]
    for a, x in S.STEP_BARS:
        cy = S.STEP_Y0 + 1
        px, py = int(x), S.STEP_Y0 - 1                      # the bar's first pixel in raster order (the dilation adds a row on top)
        assert R.mask[py, px] == 255 and o.get_centre(R.mask, float(px), float(py)) == (float(x), float(cy)), (a, o.get_centre(R.mask, float(px), float(py)))
        col = R.mask[:, x] == 255
        assert col[cy:cy + a].all() and not col[cy + a:cy + a + 16].any() and col[cy + a + 16], a
    assert [a for a, _ in S.STEP_BARS] == [64, 49, 50, 51]

    # gap_T: the same with a gap of T + 1 behind steps 8, 16, 24, 32; the dashes T apart make a line
    for T in S.GAPS:
        R = ref["gap_%d" % T]
        assert R.case.max_gap == T and len(R.lines) >= 1
        for a, x in S.GAP_BARS:
            cy = S.GAP_Y0 + 1
            col = R.mask[:, x] == 255
            assert col[cy:cy + a].all() and not col[cy + a:cy + a + T + 1].any() and col[cy + a + T + 1], (T, a)

    # window: two candidates' neighbourhoods inside one kept window (192 columns from a word boundary, 135 + 24 rows), the third outside
    ys, xs = np.nonzero(ref["window"].mask == 255)
    near, far = xs < 100, xs > 200
    assert near.any() and far.any() and (near | far).all()
    assert np.ptp(ys[near]) <= 24 and np.ptp(xs[near]) < 32 and xs[far].min() - xs[near].min() > 192
    assert ref["window"].rounds >= 3 and len(ref["window"].lines) == 0
