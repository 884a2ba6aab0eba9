"""CPU half of the varying-size pipeline tests (tests/pipeline_size_cases.py): the sequences' self-assertions at every depth the
GPU file uses, on the library's band rule and on the ORACLE's outputs for the frames; the mode controller's bucket restated; the
slot model against a case walked by hand; and the mutant check -- a slot that kept a stale record, dropped a submission's last
frame or ignored the rotation would show another record than the true slot at an index the GPU file reads.  No device."""
import zlib

import numpy as np
import pytest

import pipeline_size_cases as P


@pytest.fixture(scope="module")
def o(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", params=P.SIZES, ids=P.SIZE_IDS)
def size(request, built):
    return request.param


def test_frames_are_what_the_model_assumes(size):
    frames, infos, refs = P.oracle_of(size)
    assert frames.shape == (P.K, size.H, size.W, 4)
    assert [r["map_open"] for r in refs] == [0 if i in P.CLOSED else 1 for i in range(P.K)]
    assert [refs[i]["red_pixels"] for i in P.CLOSED] == [3, 5]                         # the two closed frames' records differ too
    assert len({P.record_key(r) for r in refs}) == P.K
    opened = [r for r in refs if r["map_open"]]
    assert all(r["n_mask_px"] > 0 and r["n_lines"] >= 1 for r in opened)
    assert len({r["lsd"].tobytes() for r in opened}) == len(opened) and len({r["ui_map"].tobytes() for r in opened}) == len(opened)


@pytest.mark.parametrize("depth", P.DEPTHS)
def test_sequence_reaches_what_it_is_there_for(size, depth):
    _, _, refs = P.oracle_of(size)
    P.check_sequence(size, depth, refs)


@pytest.mark.parametrize("depth", P.DEPTHS)
def test_mutant_slot_models_are_told_apart(size, depth):
    _, _, refs = P.oracle_of(size)
    found = P.mutants_are_told_apart(size, depth, refs)
    assert set(found) == {"stale", "drop_last", "unrotated"} and all(v > 0 for v in found.values()), found


def test_sequence_self_check_notices_a_sequence_that_proves_nothing(size):
    """The same n every time, or the same rotation every time, fails the self-check."""
    _, _, refs = P.oracle_of(size)
    real = P.sequence(size, 4)
    for bad in ([(size.M, r) for _, r in real], [(n, 0) for n, _ in real], [(n, (3 * (j // 4)) % P.K) for j, (n, _) in enumerate(real)]):
        with pytest.raises(AssertionError):
            P.check_sequence(size, 4, refs, bad)
    P.check_sequence(size, 4, refs, real)


def test_slot_model_on_a_case_walked_by_hand():
    """One slot of 6, frames 1 and 4 closed: 5 frames at rotation 0, then 2 at rotation 1, then 4 at rotation 2."""
    open_of = [True, False, True, True, False, True]
    m = P.SlotModel(6, open_of)
    m.submit(5, 0)
    assert m.rec == [0, 1, 2, 3, 4, None] and m.img == [(0, 5), None, (2, 5), (3, 5), None, None] and m.hwm == 5
    m.submit(2, 1)                                                     # frames 1 (closed), 2: index 0 keeps frame 0's images
    assert m.rec == [1, 2, 2, 3, 4, None] and m.img == [(0, 5), (2, 2), (2, 5), (3, 5), None, None] and m.hwm == 5
    assert m.image_indices(2) == [0, 1, 2, 4] and m.cover == [(1, 2), (2, 2), (2, 5), (3, 5), (4, 5), None]
    m.submit(4, 2)                                                     # frames 2, 3, 4 (closed), 5
    assert m.rec == [2, 3, 4, 5, 4, None] and m.img == [(2, 4), (3, 4), (2, 5), (5, 4), None, None]
    # the mutants on the same walk
    for mutant, want in (("stale", [0, 3, 4, 5, 4, None]), ("drop_last", [2, 3, 4, 3, None, None]), ("unrotated", [0, 1, 2, 3, 4, None])):
        k = P.SlotModel(6, open_of, mutant)
        for n, rot in ((5, 0), (2, 1), (4, 2)):
            k.submit(n, rot)
        assert k.rec == want, (mutant, k.rec)


def test_restated_same_shape():
    ss = lambda a, b, st=(0xF, 0xF), gap=(15, 15): P.same_shape(a, st[0], gap[0], b, st[1], gap[1])   # noqa: E731
    assert ss(20, 24) and ss(24, 20) and ss(24, 24) and ss(4, 5) and ss(1, 1)
    assert not ss(19, 24) and not ss(24, 3) and not ss(1, 2) and not ss(3, 4) and ss(16, 20) and not ss(16, 21)
    assert not ss(24, 24, st=(0xF, 0x3)) and not ss(24, 24, gap=(15, 16))
    assert all(ss(a, b) for a in range(20, 25) for b in range(20, 25))                 # the adaptive test's first phase is ONE workload


def test_adaptive_sequence(built):
    for settle in (26 * 6 + 52,):
        P.check_adaptive_sequence(6, settle)
    _, _, refs = P.oracle_of(P.ADAPTIVE)
    seq, settle = P.adaptive_sequence(6, 26 * 6 + 52)
    open_of = [bool(r["map_open"]) for r in refs]
    keys = [P.record_key(r) for r in refs]
    true = P.run_model(P.ADAPTIVE, 6, open_of, seq=seq)
    for mutant in ("stale", "drop_last", "unrotated"):
        other = P.run_model(P.ADAPTIVE, 6, open_of, mutant, seq=seq)
        assert any(t[3][i] != m[3][i] and (t[3][i] is None or m[3][i] is None or keys[t[3][i]] != keys[m[3][i]]) for t, m in zip(true, other) for i in range(P.ADAPTIVE.M)), mutant


def test_capture_sequences_give_slabs_of_one_six_full_and_two(o):
    frames, _, _ = P.oracle_of(P.ADAPTIVE)
    crcs = [zlib.crc32(f.tobytes()) for f in frames]
    assert len(set(crcs)) == P.K
    kept = P.check_capture_slabs(P.ADAPTIVE.M, crcs, o.capture_dedupe)
    assert sum(len(c) for c in P.capture_slabs(P.ADAPTIVE.M)) - sum(len(k) for k in kept) == 3 - 1 + 3 + 24 + 2
    assert all(a != b for k in kept for a, b in zip(k, k[1:]))
    assert any(i in P.CLOSED for i in kept[1]) and np.array_equal(frames[kept[0][0]], frames[0])
