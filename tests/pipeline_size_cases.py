"""Submissions of VARYING size through one pipeline: what real callers do (an ingest slab holds however many captures were no
duplicates) and what a slot of a pipeline must get right -- the streaming pass's band height, whether the tile-major mask is
written, the items the search service is given, the high-water marks of the lazy mask and ui_map, and what the slot holds at
indices >= n -- all depend on n, and a slot sees a large submission, then a small one, then a large one with other content.

Four rows of tests/geometry_sweep_cases.py, six distinct frames each (two of them closed; the oracle runs once each), a sequence
of n per pipeline depth, every submission the frames in another rotation -- and a MODEL of a slot (SlotModel) that says which
frame's record and which frame's images every index must show after every submission.  The cases assert on the oracle's own
outputs that a stale record, a dropped last frame or an unrotated frame order would be noticed.  Pure numpy plus the library's
host-only helpers (smhv_map_bounds, smhv_debug_band_rows); the oracle is imported by oracle_of() only."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import geometry_sweep_cases as G

K = 6                                           # distinct frames per size
CLOSED = (1, 4)                                 # their indices: three apart, so no rotation step but 0 and 3 lands closed on closed
USES = 4                                        # submissions per slot
Size = namedtuple("Size", "W H M why")
SIZES = [
    Size(568, 361, 48, "m_quads 65; tiny, the workhorse"),
    Size(1118, 1182, 32, "rh 900; the last height with the tile-major mask at any n"),
    Size(1097, 1184, 32, "rh 901; tile-major mask only while the bands are whole tile rows: 32 frames is the fewest with full-height bands"),
    Size(1921, 1081, 22, "frames 4 bytes off a 16-byte boundary; 22 frames is the fewest with 24-row bands"),
]
SIZE_IDS = ["%dx%d" % (s.W, s.H) for s in SIZES]
ADAPTIVE = Size(568, 361, 24, "the adaptive pipeline at depth 6")
DEPTHS = (2, 3, 4, 6)


def sweep_case(s):
    return next(c for c in G.CASES if (c.W, c.H) == (s.W, s.H))


def band_rows(s, n, fused):
    """(rows per band, tile-major mask written) of a streaming launch over n frames: fused 1 = a plain run and a batch-granular
    pipeline of depth < 3, 2 = beside the search service.  Host logic of the library."""
    from squad_mortar_helper_amd import _lib
    rows, bands, tiles = C.c_uint32(), C.c_uint32(), C.c_int()
    _lib.check(_lib.load().smhv_debug_band_rows(s.W, s.H, n, fused, C.byref(rows), C.byref(bands), C.byref(tiles)))
    return rows.value, bool(tiles.value)


def cycle_of(s):
    """The five sizes a slot's submissions cycle through: M, 1, M - 1, the smallest n whose bands differ from one frame's, the
    largest n below M - 1 whose bands differ from M frames'."""
    M = s.M
    one, full = band_rows(s, 1, 1), band_rows(s, M, 1)
    a = next((n for n in range(2, M - 1) if band_rows(s, n, 1) != one), 2)
    b = next((n for n in range(M - 2, 1, -1) if band_rows(s, n, 1) != full and n != a), M // 2)
    return [M, 1, M - 1, a, b]


def sequence(s, depth):
    """[(n, rotation)] of USES x depth submissions: submission j goes to slot j % depth; the slot's u-th use takes entry (u + slot)
    of the cycle, and the frames rotated one further than its previous use (two further than the submission before it)."""
    cyc = cycle_of(s)
    return [(cyc[(j // depth + j % depth) % len(cyc)], (2 * (j % depth) + j // depth) % K) for j in range(USES * depth)]


def frame_of(i, rot):
    """Which of the K frames stands at index i of a submission with rotation rot (the device buffer holds the frames with period
    K, a rotation is a pointer offset of `rot` frames)."""
    return (i + rot) % K


def same_shape(n_a, st_a, gap_a, n_b, st_b, gap_b):
    """The mode controller's bucket, restated (smh_runtime.cpp): stages and gap exactly, frames within 25 %."""
    if st_a != st_b or gap_a != gap_b:
        return False
    lo, hi = min(n_a, n_b), max(n_a, n_b)
    return hi * 4 <= lo * 5


# ---- the slot model --------------------------------------------------------------------------------------------------------------

class SlotModel:
    """What one slot must hold.  rec[i]: the frame whose record index i shows (None: never written); img[i]: (frame, n of the
    submission that wrote it) of the images at index i -- a closed frame writes its record and keeps the older images; cover[i]: (frame,
    n) of the newest submission that covered index i, open or closed: the tile-major mask's `written` flag follows THAT one (the
    button test clears it for every frame of a run, the streaming pass sets it again for the open frames whose bands are whole tile
    rows), so a frame found closed reads "bit rows only" over its older, still valid bit rows.
    mutant: None, "stale" (index 0 of a submission keeps what it held), "drop_last" (a submission writes n - 1 frames),
    "unrotated" (frame order without the rotation)."""

    def __init__(self, M, open_of, mutant=None):
        self.M, self.open_of, self.mutant = M, open_of, mutant
        self.rec = [None] * M
        self.img = [None] * M
        self.cover = [None] * M
        self.hwm = 0

    def submit(self, n, rot):
        rot = 0 if self.mutant == "unrotated" else rot
        for i in range(n - 1 if self.mutant == "drop_last" else n):
            if self.mutant == "stale" and i == 0 and self.rec[0] is not None:
                continue
            f = frame_of(i, rot)
            self.rec[i] = f
            self.cover[i] = (f, n)
            if self.open_of[f]:
                self.img[i] = (f, n)
        self.hwm = max(self.hwm, n)

    def image_indices(self, n):
        """The indices whose images a test reads after a submission of n frames: 0, n - 1, n and the high-water mark - 1."""
        return sorted({0, n - 1, min(n, self.M - 1), self.hwm - 1})


def run_model(s, depth, open_of, mutant=None, seq=None):
    """-> [(slot, n, rot, rec copy, img copy)] per submission."""
    slots = [SlotModel(s.M, open_of, mutant) for _ in range(depth)]
    out = []
    for j, (n, rot) in enumerate(sequence(s, depth) if seq is None else seq):
        m = slots[j % depth]
        m.submit(n, rot)
        out.append((j % depth, n, rot, list(m.rec), list(m.img)))
    return out


def record_key(ref):
    """What of an oracle output reaches the record: enough to tell any two of a size's frames apart."""
    return (ref["map_open"], ref["red_pixels"], ref["n_lines"], ref["lines"].tobytes(), ref["n_mask_px"], ref["rounds"], ref["mpx"])


def check_sequence(s, depth, refs, seq=None):
    """The purpose of sequence(s, depth) -- or of `seq` in its place -- asserted: on the band rule and on the oracle's refs."""
    seq = sequence(s, depth) if seq is None else seq
    M = s.M
    ns = [n for n, _ in seq]
    assert {1, M, M - 1} <= set(ns) and all(1 <= n <= M for n in ns), ns
    for fused in (1, 2):
        assert len({band_rows(s, n, fused)[0] for n in ns}) >= 2, (s, fused, ns)          # band heights differ
    if (s.W, s.H) == (1097, 1184):
        for fused in (1, 2):
            assert {band_rows(s, n, fused)[1] for n in ns} == {True, False}                # both sides of the change of `tiles`
            assert band_rows(s, M, fused)[0] == 58 and band_rows(s, M - 1, fused)[0] < 58  # M is the fewest with full-height bands
    keys = [record_key(r) for r in refs]
    open_of = [bool(r["map_open"]) for r in refs]
    assert len(set(keys)) == K and [i for i in range(K) if not open_of[i]] == list(CLOSED)
    for slot in range(depth):
        uses = [seq[j] for j in range(slot, len(seq), depth)]
        assert len(uses) == USES
        steps = [b[0] - a[0] for a, b in zip(uses, uses[1:])]
        assert any(d > 0 for d in steps) and any(d < 0 for d in steps), (slot, uses)       # larger-then-smaller and smaller-then-larger
        closed_on_open = open_on_closed = False
        for (na, ra), (nb, rb) in zip(uses, uses[1:]):
            for i in range(min(na, nb)):
                fa, fb = frame_of(i, ra), frame_of(i, rb)
                assert keys[fa] != keys[fb], (slot, i, fa, fb)                             # a stale record is never the fresh one
                closed_on_open |= open_of[fa] and not open_of[fb]
                open_on_closed |= open_of[fb] and not open_of[fa]
        assert closed_on_open and open_on_closed, slot
    for (_, ra), (_, rb) in zip(seq, seq[1:]):
        assert ra != rb                                                                     # every submission another rotation


def mutants_are_told_apart(s, depth, refs):
    """For each mutant slot model, some index some test reads shows another record (by the oracle's refs) than the true model's."""
    keys = [record_key(r) for r in refs]
    open_of = [bool(r["map_open"]) for r in refs]
    true = run_model(s, depth, open_of)
    found = {}
    for mutant in ("stale", "drop_last", "unrotated"):
        other = run_model(s, depth, open_of, mutant)
        found[mutant] = sum(1 for t, m in zip(true, other) for i in range(s.M)
                            if (None if t[3][i] is None else keys[t[3][i]]) != (None if m[3][i] is None else keys[m[3][i]]))
    return found


# ---- frames --------------------------------------------------------------------------------------------------------------------------

def make_frames(s):
    """Six frames of the size's sweep scene: seeds apart, frames 1 and 4 closed -- with 3 and 5 red pixels in the button, so that
    even the two closed frames' records differ -> (uint8 [K, H, W, 4], [info])."""
    import squad_mortar_helper_amd as smh
    c = sweep_case(s)
    bx, by, bw, bh = smh.button_bounds(s.W, s.H)
    made = []
    for i in range(K):
        f, info = G.make_frame(c, 5000 + 10 * G.CASES.index(c) + i, open_=i not in CLOSED, random_alpha=bool(i % 2))
        if i in CLOSED:
            f[by, bx:bx + 3 + 2 * CLOSED.index(i), :3] = G.BUTTON_RED
        made.append((f, info))
    return np.stack([m[0] for m in made]), [m[1] for m in made]


@functools.lru_cache(maxsize=None)
def oracle_of(s):
    """(frames, infos, refs) as geometry_sweep_cases.oracle_of gives them, for make_frames(s); computed once per size."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as o
    frames, infos = make_frames(s)

    def one(i):
        ref = o.process_frame(frames[i], grayscale=True, max_gap=G.MAX_GAP, stages=0xF, anchors=infos[i]["anchors"] or None,
                              scales_start_y=infos[i]["scales_start_y"], want_images=True)
        ref["red_pixels"] = o.button_red_pixels(frames[i])
        ref["minimap"] = None
        return ref
    with ThreadPoolExecutor(K) as ex:
        refs = list(ex.map(one, range(K)))
    return frames, infos, refs


# ---- the adaptive pipeline's two phases ---------------------------------------------------------------------------------------------------

def adaptive_sequence(depth, settle):
    """Phase 1: `settle` submissions with n cycling through 20..24 (one bucket); phase 2: 4 x depth submissions alternating 24 with
    3, 5, 7, ... (across buckets).  Rotations as in sequence()."""
    M = ADAPTIVE.M
    ns = [20 + (j * 3) % 5 for j in range(settle)]
    small = [3, 5, 7, 2, 1, 9]
    ns += [M if (j + j // depth) % 2 == 0 else small[(j // 2) % len(small)] for j in range(4 * depth + 1)]   # (a slot gets both kinds in turn)
    return [(n, (2 * (j % depth) + j // depth) % K) for j, n in enumerate(ns)], settle


def check_adaptive_sequence(depth, settle):
    seq, _ = adaptive_sequence(depth, settle)
    p1, p2 = [n for n, _ in seq[:settle]], [n for n, _ in seq[settle:]]
    assert set(p1) == {20, 21, 22, 23, 24} and all(same_shape(a, 0xF, 15, b, 0xF, 15) for a in p1 for b in p1)
    crossing = sum(not same_shape(a, 0xF, 15, b, 0xF, 15) for a, b in zip(p2, p2[1:]))
    assert 4 * crossing >= 3 * (len(p2) - 1) and {24, 3, 5} <= set(p2), p2                      # across buckets nearly every time
    for slot in range(depth):
        mine = [n for j, (n, _) in enumerate(seq) if j >= settle and j % depth == slot]
        assert 24 in mine and min(mine) <= 9, (slot, mine)
    for slot in range(depth):                                        # each slot sees different n in phase 1 already, and both directions in all
        uses = [seq[j][0] for j in range(slot, len(seq), depth)]
        steps = [b - a for a, b in zip(uses, uses[1:])]
        assert len(set(uses[:settle // depth])) >= 2 and any(d > 0 for d in steps) and any(d < 0 for d in steps), (slot, uses)
    for slot in range(depth):
        uses = [seq[j] for j in range(slot, len(seq), depth)]
        assert all(ra != rb for (_, ra), (_, rb) in zip(uses, uses[1:]))


# ---- end to end: capture sequences whose duplicate pattern gives slabs of different n -------------------------------------------------------

def capture_slabs(M):
    """[[frame index per capture]] per slab for a queue of capacity M: a slab of ONE frame (three captures of the same), a short
    one, a FULL one (every capture twice), a short one that begins with a duplicate of the slab before."""
    full = [(i + 1) % K for i in range(M) for _ in (0, 1)]           # (begins with frame 1: the slab before ends with frame 0)
    return [[0, 0, 0], [0, 1, 1, 2, 3, 3, 4, 5, 0], full, [full[-1], 2, 2, 4]]


def check_capture_slabs(M, crcs, dedupe):
    """dedupe = oracle.capture_dedupe; crcs[i] = CRC of frame i -> [[kept frame index]] per slab; asserts the slab sizes."""
    last, kept = 0, []
    for caps in capture_slabs(M):
        keep, last = dedupe([crcs[i] for i in caps], last)
        kept.append([i for i, k in zip(caps, keep) if k])
    assert [len(k) for k in kept] == [1, 6, M, 2], [len(k) for k in kept]
    assert kept[1] == [1, 2, 3, 4, 5, 0] and kept[3] == [2, 4] and kept[2][0] == 1 and kept[2][-1] == M % K
    return kept
