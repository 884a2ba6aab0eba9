"""The crafted line-search cases (tests/lsd_cases.py; their expectations are asserted on the oracle by tests/test_lsd_cases_host.py)
through all three implementations of find_lines, byte-exact against the oracle -- lines, n_lines, rounds, n_mask_px, and the sample
count under exact statistics; the lsd image too on the per-call path:

  k_lsd           the per-call trait path (VisionState.process), every case, statistics culled and exact
  k_lsd_tile      FrameBatch, all cases of a size and gap threshold in one batch: the default, smhv_debug_lsd_classic (k_lsd again, batched),
                  the tile store capped at 4 tiles (every frame overflows it), 256 threads per workgroup, late helpers, and the frames in
                  reversed order (heavy frames change position)
  k_lsd_service   a frame-granular pipeline of depth 3 with each of its help switches, the walk over the bit rows, and the tile store
                  capped at 4: four submissions per statistics mode, every slot identical and equal to the oracle

Sizes: 1024 x 768 and 1920 x 1080 carry every case, 2560 x 1440 (compact tile index, no tile-major mask from the pass, k_lsd's
non-ROWS modes) 24 of them, 3440 x 1440 the cases around ROI column 2048."""
import numpy as np
import pytest

import lsd_cases as C

pytestmark = pytest.mark.gpu

SIZE_IDS = {C.SMALL: "768p", C.HD: "1080p", C.QHD: "1440p", C.WIDE: "ultrawide"}


@pytest.fixture(scope="module")
def groups():
    """size -> [(max_gap, [Ref], frames on the device)]: the oracle's answers once per session (lsd_cases.reference), a size's frames uploaded
    when a test first asks for them and freed when the module is done."""
    import torch
    held = {}

    def get(size):
        if size not in held:
            refs = {R.case.name: R for R in C.reference(size)}
            held[size] = [(gap, [refs[c.name] for c in cs], torch.from_numpy(np.stack([C.frame(c, *size) for c in cs])).cuda()) for gap, cs in C.groups(size)]
        return held[size]

    yield get
    held.clear()
    torch.cuda.empty_cache()


def _check(got, refs, exact, tag):
    """tag: a callable giving what goes into the message (evaluated on failure only)."""
    assert len(got) == len(refs)
    for g, R in zip(got, refs):
        name = R.case.name
        assert g["n_lines"] == len(R.lines) and np.array_equal(g["lines"], R.lines), (name, g["lines"], R.lines) + tag()
        assert g["rounds"] == R.rounds and g["n_mask_px"] == R.n_mask_px, (name, g["rounds"], R.rounds, g["n_mask_px"], R.n_mask_px) + tag()
        if exact:
            assert g["ray_steps"] == R.steps, (name, g["ray_steps"], R.steps) + tag()


PER_CALL = [(size, family) for size in C.SIZES for family in C.FAMILIES if any(c.family == family for c in C.cases_at(size))]


@pytest.mark.parametrize("size,family", PER_CALL, ids=["%s-%s" % (SIZE_IDS[s_], f) for s_, f in PER_CALL])
def test_per_call_trait_path(vision, groups, size, family):
    import squad_mortar_helper_amd as smh
    n = 0
    for gap, refs, d in groups(size):
        for i, R in enumerate(refs):
            if R.case.family != family:
                continue
            st = smh.VisionState(grayscale_map=True, max_gap=gap)
            try:
                res = st.process(vision, d[i].cpu().numpy())
                name = R.case.name
                assert np.array_equal(vision.lsd_image(), R.mask), name
                assert res.markers.shape == R.lines.shape and np.array_equal(res.markers, R.lines), (name, res.markers, R.lines)
                r_fast, s_fast = vision.lsd_stats(gap, exact=False)
                r_exact, s_exact = vision.lsd_stats(gap, exact=True)
                assert r_fast == r_exact == R.rounds and s_exact == R.steps and s_fast <= s_exact, (name, r_fast, r_exact, R.rounds, s_fast, s_exact, R.steps)
            finally:
                st.close()
            n += 1
    assert n


BATCH_VARIANTS = ("default", "classic", "tile_cap_4", "threads_256", "helpers", "reversed")


@pytest.mark.parametrize("variant", BATCH_VARIANTS)
@pytest.mark.parametrize("size", C.SIZES, ids=SIZE_IDS.get)
def test_frame_batch(vision, groups, size, variant):
    import torch
    import squad_mortar_helper_amd as smh
    lib = smh._lib.load()
    groups = groups(size)
    fb = smh.FrameBatch(vision, size[0], size[1], max(len(refs) for _, refs, _ in groups))
    s = torch.cuda.current_stream().cuda_stream
    try:
        lib.smhv_debug_lsd_classic(int(variant == "classic"))
        lib.smhv_debug_lsd_tile_cap(4 if variant == "tile_cap_4" else 0)
        lib.smhv_debug_lsd_threads(256 if variant == "threads_256" else 0)
        extra = smh.STAGE_LSD_HELPERS if variant == "helpers" else 0
        for gap, refs, d in groups:
            if variant == "reversed":
                refs, d = refs[::-1], d.flip(0).contiguous()
            for exact in (0, smh.STAGE_EXACT_STATS):
                fb.run(d.data_ptr(), len(refs), stages=smh.STAGE_MARKERS | exact | extra, max_gap=gap, stream=s)
                _check(smh.results_to_dicts(fb.read_results(0, len(refs))), refs, exact, lambda: (variant, gap, bool(exact)))
    finally:
        lib.smhv_debug_lsd_classic(0)
        lib.smhv_debug_lsd_tile_cap(0)
        lib.smhv_debug_lsd_threads(0)
        fb.close()


SERVICE_VARIANTS = ("plain", "no_team_help", "no_remote_help", "help_first", "walk_bit_rows", "tile_cap_4")


@pytest.mark.parametrize("variant", SERVICE_VARIANTS)
@pytest.mark.parametrize("size", C.SIZES, ids=SIZE_IDS.get)
def test_search_service(vision, groups, size, variant):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    lib = _lib.load()
    flags = {"no_team_help": _lib.PIPE_NO_TEAM_HELP, "no_remote_help": _lib.PIPE_NO_REMOTE_HELP, "help_first": _lib.PIPE_HELP_FIRST,
             "walk_bit_rows": _lib.PIPE_WALK_BIT_ROWS}.get(variant, 0)
    groups = groups(size)
    try:
        lib.smhv_debug_lsd_tile_cap(4 if variant == "tile_cap_4" else 0)      # (read when the pipeline is created)
        pipe = smh.Pipeline(vision, size[0], size[1], max(len(refs) for _, refs, _ in groups), 3, search="frame", flags=flags)
    finally:
        lib.smhv_debug_lsd_tile_cap(0)
    try:
        for gap, refs, d in groups:
            n = len(refs)
            for exact in (0, smh.STAGE_EXACT_STATS):
                slots = [pipe.submit(d.data_ptr(), n, stages=smh.STAGE_MARKERS | exact, max_gap=gap) for _ in range(4)]
                pipe.wait()
                recs = {s_: pipe.slots[s_].read_results(0, n) for s_ in sorted(set(slots))}
                tag = lambda: (variant, gap, bool(exact), pipe.search_stats())          # the service's counters, on failure only
                for s_, r in recs.items():
                    _check(smh.results_to_dicts(r), refs, exact, tag)
                first = bytes(recs[slots[0]])
                assert all(bytes(r) == first for r in recs.values()), tag()             # (beside the oracle comparison: every slot the same bytes)
    finally:
        pipe.close()
