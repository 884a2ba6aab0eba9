"""CPU half of the long-call and layout tests of the remote-viewer feed (tests/web_long_cases.py): the tables' self-checks, the
unique frames' properties on the ORACLE's outputs, every named sequence's check and every capacity cut's frames_done on
tests/web_ref.py's feed(), the continuation property on the reference alone, and the mutant check -- a feed that forgot the
stored CRC at a chunk's start, did not take it from a chunk that ends on closed frames, lost the layout over a chunk without an
open frame, rounded frames_done to the chunk or looked for the cut in the first chunk only gives another result than feed() on
the sequence named for that rule.  No device."""
import numpy as np
import pytest

import web_long_cases as L
import web_ref as W


@pytest.fixture(scope="module")
def uniq(built):
    """web_ref.feed's input for the four unique frames, grey and colour, from the oracle."""
    c = L.LONG_CASE
    _, _, refs = L.unique_oracle()
    return {gray: [L.ref_frame(r, gray, c.rw, c.rh) for r in refs] for gray in (True, False)}


def test_tables_hold_what_they_are_there_for(built):
    L.check_long_case()
    L.check_sweep()
    c = L.LONG_CASE
    assert L.items_per_map(c.rw, c.rh) == 3 and L.items_per_map(8, 274) == 1 and L.items_per_map(4096, 274) == 274
    assert L.copy_passes(7, 986, 822) == 1                                               # what the suite fed until now: seven 1080p Maps, one pass
    assert L.copy_passes(L.N_LONG, 8, 274) == 2                                          # (the narrowest ROI would still give two)
    for name, m in L.MASTERS.items():
        assert len(m) == L.N_LONG and set(m.tolist()) <= {L.X, L.Y, L.Z, L.CLOSED}, name
    assert set(L.MUTANTS.values()) <= set(L.SEQ_NAMES) | set(L.CUT_NAMES)
    assert set(L.SEQ_NAMES) == {"edge_same", "edge_diff", "closed_tail", "closed_chunk", "closed_first_chunk", "all_maps", "lengths", "snapshot_long"}
    assert len(L.CUTS) == 4 and len(L.MUTANTS) == 5


def test_unique_frames_are_what_the_sequences_assume(built):
    frames, per, refs = L.unique_oracle()
    assert frames.shape == (4, L.LONG_CASE.H, L.LONG_CASE.W, 4) and [len(p[1]) for p in per] == [0, 1, 1, 0]
    L.check_unique(refs)


def test_flip_spots_and_flipped_frames(built):
    """The spots sit where they are meant to, and on the oracle every flipped frame's ui_map differs from the base's in that pixel alone."""
    assert L.flip_spots(L.FLIP_CASES[0]) == [(r, col) for r in (0, 273) for col in (0, 3, 251, 252, 255)]           # K = 1, 64 lanes, m_xoff 0
    assert L.flip_spots(L.FLIP_CASES[1]) == [(r, col) for r in (0, 274) for col in (0, 6, 254, 255)]                # K = 2: lane 32 holds column 255 alone
    for c in L.FLIP_CASES:
        _, _, refs = L.flipped_oracle(c)
        spots = L.flip_spots(c)
        assert len(refs) == 1 + len(spots) and all(r["map_open"] for r in refs)
        for key in ("ui_map", "ui_colour"):
            for k, (py, px) in enumerate(spots):
                assert np.argwhere(np.any(refs[1 + k][key] != refs[0][key], axis=2)).tolist() == [[py, px]], (c, key, k)


@pytest.mark.parametrize("gray", [False, True], ids=["colour", "grey"])
@pytest.mark.parametrize("name", L.SEQ_NAMES)
def test_every_sequence_is_there_for_what_it_says(uniq, name, gray):
    seq = L.SEQUENCES[name]
    fr = L.master_ref(seq.master, uniq[gray])
    seq.check(L.run_reference(seq, fr), fr)


@pytest.mark.parametrize("cut", L.CUTS, ids=L.CUT_NAMES)
def test_every_cut_and_its_continuation(uniq, cut):
    """frames_done of every cut, and feeding on from first + frames_done reproduces the uncut messages and the stored CRC."""
    fr = L.master_ref("mixed", uniq[True])
    first = L.check_cut(cut, fr)
    cap = L.cut_capacity(cut, fr)
    assert first["bytes_used"] <= cap
    parts, msgs, stored = L.rounds_of(fr, cap)
    uncut = W.feed(fr)
    assert parts[0] == first and len(parts) >= 2 and sum(p["frames_done"] for p in parts) == L.N_LONG
    assert msgs == uncut["messages"] and stored == uncut["stored"]


@pytest.mark.parametrize("rule", sorted(L.MUTANTS))
def test_every_mutant_is_told_apart(uniq, rule):
    assert L.mutant_is_told_apart(rule, uniq[True]) and L.mutant_is_told_apart(rule, uniq[False]), rule


def test_mutants_change_one_rule_only(uniq):
    """On a call of one chunk without a cut every mutant is web_ref.feed."""
    fr = L.master_ref("mixed", uniq[True])[:L.B - 1]
    want = W.feed(fr)
    for rule in L.MUTANTS:
        assert L.mutant_feed(rule)(fr) == want, rule
    # and the two cut mutants fail the cut's own check
    for rule in ("done_rounded_to_chunk", "cut_in_first_chunk_only"):
        with pytest.raises(AssertionError):
            L.check_cut(L.CUTS[2], L.master_ref("mixed", uniq[True]), L.mutant_feed(rule))
