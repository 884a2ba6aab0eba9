"""The ingest queue at the edges of its kernels: frame sizes for k_to_bgra's four pixels per thread and its grid-stride limit, for
the queue's own CRC launch with two rounds, and for the ROI upload's two rectangles -- with the builders the tests share.

Every size is a row of tests/geometry_sweep_cases.py (one odd x odd size above the grid-stride limit is added here, its derived
numbers written out the same way); check_tables() holds each row to smh.map_bounds / button_bounds and to the launch arithmetic
RESTATED below, so a typo in a size, or a change of a limit in the library, fails here instead of testing something else.  Pure
numpy plus the library's host-only bounds helpers; the oracle is imported inside the functions that need it."""
import zlib
from collections import namedtuple

import numpy as np

import squad_mortar_helper_amd as smh
import geometry_sweep_cases as G

# ---- the launch arithmetic, restated (smh_misc.hip: launch_to_bgra; smh_runtime.cpp: crc_plan; k_crc32) -------------------------
TO_BGRA_GRID_PX = 2048 * 256 * 4            # workgroups x threads x pixels per thread of ONE trip of k_to_bgra's grid-stride loop
CRC_BS, CRC_MAX_WGS = 1024, 1024
GUARD = 0xA7                                # what the acquire path fills the staging buffer with before the pixels go in
LAYOUTS = ("rgba", "rgb", "l", "la", "bgra")
BPP = {"bgra": 4, "rgba": 4, "rgb": 3, "l": 1, "la": 2}


def crc_plan(nbytes):
    """-> dict(groups, wgs, G, rounds, pad, split): groups of 16 bytes, at most 1024 workgroups of 1024 threads, rounds =
    ceil(groups / G); the message is right-aligned in the last round behind `pad` virtual zero dwords; `split` = the first byte
    of round 1's span (None with one round)."""
    assert nbytes % 4 == 0
    nd = nbytes // 4
    groups = (nd + 3) // 4
    wgs = max(1, min(CRC_MAX_WGS, -(-groups // CRC_BS)))
    Gt = wgs * CRC_BS
    rounds = max(1, -(-groups // Gt))
    pad = rounds * Gt * 4 - nd
    split = (Gt * 4 - pad) * 4 if rounds > 1 else None
    return dict(groups=groups, wgs=wgs, G=Gt, rounds=rounds, pad=pad, split=split)


# ---- the size table ----------------------------------------------------------------------------------------------------------
SizeRow = namedtuple("SizeRow", "W H n_px residue trips rounds why")
# (W, H, n_px, n_px % 4, trips of k_to_bgra's loop, CRC rounds, why)
_SIZES = [
    (568, 361, 205048, 0, 1, 1, "n_px % 4 == 0: every thread stores a whole quad"),
    (2233, 361, 806113, 1, 1, 1, "n_px % 4 == 1: the last thread holds ONE pixel; with 3-byte pixels its source ends 1 byte into a dword"),
    (454, 361, 163894, 2, 1, 1, "n_px % 4 == 2"),
    (343, 361, 123823, 3, 1, 1, "n_px % 4 == 3: with 3-byte pixels the last pixel straddles two dwords"),
    (3295, 1440, 4744800, 0, 3, 2, "above the grid-stride limit (three trips) and above 16 MiB: the queue's CRC launch takes two rounds, pad % 4 == 0"),
    (2923, 1441, 4212043, 3, 3, 2, "odd x odd above both limits: a ragged last quad in the loop's third trip; two CRC rounds with pad % 4 == 1 (dword loads)"),
]
SIZES = [SizeRow(*t) for t in _SIZES]
SIZE_IDS = ["%dx%d" % (r.W, r.H) for r in SIZES]
LARGE = [r for r in SIZES if r.rounds == 2]
ADDED = (2923, 1441)                        # the one size that is not a row of the geometry sweep: rx 1219, ry 237, rw 1677, rh 1097

# ---- the ROI rows: (W, H, m_ax, roi_px, button rectangle, why) ------------------------------------------------------------------
RoiRow = namedtuple("RoiRow", "W H m_ax roi_px button why")
_ROI = [
    (451, 360, 304, 140, (363, 343, 85, 14), "residues: m_xoff 0 with W % 4 == 3: the quads are the ROI's own columns"),
    (454, 361, 304, 144, (366, 344, 85, 14), "residues: m_xoff 1 with W % 4 == 2: one column before and one behind the ROI travel with it"),
    (453, 362, 304, 144, (365, 345, 85, 14), "residues: m_xoff 2 with W % 4 == 1: two columns before and two behind"),
    (454, 362, 304, 144, (366, 345, 85, 14), "residues: m_xoff 2 with W % 4 == 2, rw % 4 == 1: two before, one behind"),
    (319, 360, 304, 8, (231, 343, 85, 14), "the narrowest ROI: two quads"),
    (1365, 767, 648, 704, (1178, 732, 181, 29), "odd x odd, m_xoff 1: rows 4 bytes off a 16-byte boundary"),
    (1921, 1081, 912, 992, (1658, 1032, 255, 41), "odd x odd, m_xoff 3: three columns before, three behind"),
]
ROI_ROWS = [RoiRow(*t) for t in _ROI]
ROI_IDS = ["%dx%d" % (r.W, r.H) for r in ROI_ROWS]
HISTORY_ROWS = [r for r in ROI_ROWS if (r.W, r.H) in ((453, 362), (1365, 767), (1921, 1081))]      # m_xoff 2, 1, 3
SMALLEST = (319, 360)


def sweep_case(W, H):
    return next(c for c in G.CASES if (c.W, c.H) == (W, H))


def roi_numbers(W, H):
    """m_ax, roi_px and the rectangles from the library's bounds: what a BGRA commit of a ROI-upload queue copies."""
    rx, ry, rw, rh = smh.map_bounds(W, H)
    m_ax = rx & ~3
    m_quads = (rw + (rx - m_ax) + 3) // 4
    return dict(rx=rx, ry=ry, rw=rw, rh=rh, m_ax=m_ax, roi_px=min(4 * m_quads, W - m_ax), button=tuple(smh.button_bounds(W, H)))


def check_tables(sizes=None, roi_rows=None):
    sizes = SIZES if sizes is None else sizes
    roi_rows = ROI_ROWS if roi_rows is None else roi_rows
    sweep = {(c.W, c.H) for c in G.CASES}
    for r in sizes:
        assert (r.W, r.H) in sweep or (r.W, r.H) == ADDED, r
        smh.map_bounds(r.W, r.H)                                      # (raises where the library refuses the size)
        plan = crc_plan(r.W * r.H * 4)
        assert (r.n_px, r.residue, r.trips, r.rounds) == (r.W * r.H, r.W * r.H % 4, -(-r.W * r.H // TO_BGRA_GRID_PX), plan["rounds"]), (r, plan)
    assert tuple(smh.map_bounds(*ADDED)) == (1219, 237, 1677, 1097) and ADDED[0] % 2 == 1 and ADDED[1] % 2 == 1
    small = [r for r in sizes if r.n_px <= TO_BGRA_GRID_PX]
    assert {r.residue for r in small} == {0, 1, 2, 3} and all(r.trips == 1 and r.rounds == 1 for r in small)
    big = [r for r in sizes if r.n_px > TO_BGRA_GRID_PX]
    assert any((r.W, r.H) == (3295, 1440) and r.n_px == 4744800 and r.residue == 0 and r.n_px * 4 > 16 << 20 for r in big)
    assert any(r.W % 2 and r.H % 2 and r.residue in (1, 3) for r in big)
    assert all(r.trips >= 2 and r.rounds == 2 for r in big)          # (the loop's second trip, the CRC's second round)
    assert any(crc_plan(r.n_px * 4)["pad"] % 4 != 0 for r in big if r.residue % 2) and any(crc_plan(r.n_px * 4)["pad"] % 4 == 0 for r in big)
    assert crc_plan(16 << 20)["rounds"] == 1 and crc_plan((16 << 20) + 4)["rounds"] == 2          # (the limit itself)
    # ---- the ROI rows ----
    for r in roi_rows:
        assert (r.W, r.H) in sweep, r
        d = roi_numbers(r.W, r.H)
        c = sweep_case(r.W, r.H)
        assert (d["m_ax"], d["roi_px"], d["button"]) == (r.m_ax, r.roi_px, r.button), (r, d)
        assert d["m_ax"] + d["roi_px"] <= r.W and d["m_ax"] <= d["rx"] and d["m_ax"] + d["roi_px"] >= d["rx"] + d["rw"]
        assert d["rx"] - d["m_ax"] == c.m_xoff and (d["roi_px"] == 4 * c.m_quads or d["m_ax"] + d["roi_px"] == r.W)
    have = {(r.W, r.H) for r in roi_rows}
    assert have >= {(c.W, c.H) for c in G.CASES if c.why.startswith("residues")} | {(319, 360), (1365, 767), (1921, 1081)}
    assert {sweep_case(r.W, r.H).m_xoff for r in roi_rows} == {0, 1, 2, 3}
    assert any(r.roi_px > roi_numbers(r.W, r.H)["rw"] + sweep_case(r.W, r.H).m_xoff for r in roi_rows)   # columns BEHIND the ROI travel too
    assert all(sweep_case(r.W, r.H).m_xoff for r in HISTORY_ROWS) and len(HISTORY_ROWS) == 3


# ---- builders -------------------------------------------------------------------------------------------------------------------

def expected_slab_frame(frame, c, layout):
    """What a ROI-upload queue leaves of `frame` (BGRA uint8 [c.H, c.W, 4]; for a video layout the CONVERTED frame) in a slab position
    that held zeros: the button rectangle and the map ROI -- whole quads from m_ax on for a BGRA commit (the host packs the columns
    the streaming pass loads), exactly rx .. rx + rw for an NV12 / I420 commit (the conversion writes the rectangle)."""
    d = roi_numbers(c.W, c.H)
    out = np.zeros((c.H, c.W, 4), np.uint8)
    overlay_slab_frame(out, frame, d, layout)
    return out


def overlay_slab_frame(slab, frame, d, layout):
    """The same onto a position with a history: `slab` is changed in place."""
    bx, by, bw, bh = d["button"]
    x0, x1 = (d["m_ax"], d["m_ax"] + d["roi_px"]) if layout == "bgra" else (d["rx"], d["rx"] + d["rw"])
    slab[d["ry"]:d["ry"] + d["rh"], x0:x1] = frame[d["ry"]:d["ry"] + d["rh"], x0:x1]
    slab[by:by + bh, bx:bx + bw] = frame[by:by + bh, bx:bx + bw]


def random_truth(W, H, seed):
    """A BGRA frame of random bytes, the alpha bytes included."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 4), dtype=np.uint8)


def source(truth, layout):
    """The pixels a decoder would hand over in `layout`, cut from one BGRA truth -> (pixels, the BGRA the slab must hold: the
    oracle's into_bgra8 of those pixels).  "l" / "la" take the truth's green channel as their luma."""
    from oracle import oracle as o
    px = {"bgra": truth, "rgba": truth[..., [2, 1, 0, 3]], "rgb": truth[..., [2, 1, 0]], "l": truth[..., 1], "la": truth[..., [1, 3]]}[layout]
    px = np.ascontiguousarray(px)
    return px, o.into_bgra8(px, layout)


# the decoder sequence of one size: (layout, truth index, path); "=" + layout: the BGRA bytes that layout's pixels become, as BGRA
DECODER_SEQ = [("rgba", 0, "push"), ("bgra", 0, "acquire"), ("rgb", 0, "push"), ("rgb", 1, "acquire"), ("l", 0, "push"), ("l", 1, "acquire"),
               ("la", 0, "push"), ("la", 1, "acquire"), ("=la", 1, "push"), ("rgba", 1, "acquire"), ("bgra", 1, "push"), ("bgra", 0, "acquire"),
               ("bgra", 1, "push")]
DECODER_KEEP = [True, False, True, True, True, True, True, True, False, True, False, True, True]


def decoder_sequence(W, H, seed):
    """-> [(layout, pixels, path, expected BGRA)] of DECODER_SEQ over two random truths: every layout enters by both paths and ends
    up in the slab from both, and the same pixels in two layouts meet three times."""
    truths = [random_truth(W, H, seed), random_truth(W, H, seed + 1)]
    out = []
    for lay, t, path in DECODER_SEQ:
        if lay.startswith("="):
            want = source(truths[t], lay[1:])[1]
            out.append(("bgra", want, path, want))
        else:
            px, want = source(truths[t], lay)
            out.append((lay, px, path, want))
    return out


def check_decoder_sequence():
    by_path = {(lay.lstrip("="), path) for (lay, _, path), k in zip(DECODER_SEQ, DECODER_KEEP) if k}
    assert by_path == {(lay, p) for lay in LAYOUTS for p in ("push", "acquire")}, by_path
    assert DECODER_KEEP.count(False) == 3 and [p for _, _, p in DECODER_SEQ] == ["push", "acquire"] * 6 + ["push"]


# ---- CRC end cases ----------------------------------------------------------------------------------------------------------------

def crc_flip_places(nbytes):
    """[(what, byte index)] of the single-bit flips for a frame whose CRC launch takes two rounds."""
    plan = crc_plan(nbytes)
    assert plan["rounds"] == 2 and 16 < plan["split"] - 1 and plan["split"] < nbytes - 1
    return [("byte 0", 0), ("byte 15", 15), ("byte 16", 16), ("last byte of round 0", plan["split"] - 1), ("first byte of round 1", plan["split"]),
            ("last byte", nbytes - 1)]


def crc_flip_sequence(frame):
    """Yields (what, frame) -- the base frame, then each flipped copy, then the last one again; the SAME array is handed out every
    time (flipped in place, restored afterwards), so the consumer must have copied it before asking for the next."""
    flat = frame.reshape(-1)
    yield "base", frame
    what = "base"
    for what, i in crc_flip_places(flat.size):
        flat[i] ^= 0x10
        yield what, frame
        if what != "last byte":
            flat[i] ^= 0x10
    yield "last byte again", frame
    flat[flat.size - 1] ^= 0x10


CRC_FLIP_KEEP = [True] * 7 + [False]


def check_crc_flips(W, H, seed):
    """All the CRCs are distinct (zlib), so the reference's duplicate rule accepts every copy -> the CRCs in order."""
    frame = random_truth(W, H, seed)
    before = frame.copy()
    crcs = [zlib.crc32(f.tobytes()) for _, f in crc_flip_sequence(frame)]
    assert np.array_equal(frame, before)
    assert len(crcs) == 8 and len(set(crcs[:7])) == 7 and crcs[7] == crcs[6]
    return crcs


# ---- the ROI-upload sequence of one case ------------------------------------------------------------------------------------------
ROI_SEQ = [0, 0, 1, 2, 3, 3, 0]                 # indices into roi_frames(): open, the same, CLOSED, open, the same but for one byte outside, dup, open
ROI_KEEP = [True, False, True, True, True, False, True]


def roi_frames(c):
    """-> (frames [4], infos [4], ref index [4]): the sweep's three frames of the case (open, closed, open with random alpha) and
    a copy of the third that differs in one byte OUTSIDE both rectangles -- a new capture for the reference, the same outputs."""
    frames, infos = G.make_frames(c)
    d = roi_numbers(c.W, c.H)
    bx, by, bw, bh = d["button"]
    assert d["ry"] > 0 and by > 0                                     # (row 0 is above both rectangles)
    outside = frames[2].copy()
    outside[0, 0, 0] ^= 1
    return list(frames) + [outside], list(infos) + [infos[2]], [0, 1, 2, 2]


# ---- slab history -------------------------------------------------------------------------------------------------------------------
YUV_KW = dict(matrix="709", full_range=False, chroma="nearest")


def history_frames(c, n=4):
    """-> (loud [n], video [n], scenes [n]): `loud` = BGRA frames of marker colour from edge to edge with the button open (what a
    stale column beside the ROI would have to hold to be noticed: a marker pixel the dilation reaches from) -- slab 1 of the order
    BGRA then video; `video` = [(layout, tight bytes, converted BGRA, info)] -- the sweep's scene through the test-only forward
    converter, NV12 and I420 in turn; `scenes` = [(BGRA frame, info)] -- other seeds of the sweep's scene with random alpha: the
    BGRA slab 2 of the order video then BGRA, which every stage runs on."""
    import yuv_ref as yr
    rng = np.random.default_rng(c.W + c.H)
    loud, video, scenes = [], [], []
    bx, by, bw, bh = smh.button_bounds(c.W, c.H)
    for i in range(n):
        scenes.append(G.make_frame(c, 7100 + i, random_alpha=True))
        f = np.empty((c.H, c.W, 4), np.uint8)
        f[..., :3] = (G.GREEN, G.PURPLE, G.TEAL)[i % 3]
        f[by:by + bh, bx:bx + bw, :3] = G.BUTTON_RED
        f[..., 3] = rng.integers(0, 256, (c.H, c.W), dtype=np.uint8)
        loud.append(f)
        scene, info = G.make_frame(c, 7000 + i)
        Y, U, V = yr.forward(scene, "709", False)
        lay = ("nv12", "i420")[i % 2]
        video.append((lay, yr.pack_tight(Y, U, V, lay), yr.to_bgra(Y, U, V, **YUV_KW), info))
    return loud, video, scenes
